/* pair_kernels.hip — hand-written CDNA4 (gfx950/MI355X) fp64 pair kernels for
 * SkellySim's hydrodynamic hot path.
 *
 * Built from scratch for MI355X; the math restates the reference
 * (flatironinstitute/SkellySim) formula by formula:
 *   Stokeslet            src/core/kernels.cu:62-76
 *   Stresslet (DL)       src/core/kernels.cu:29-54
 *   Regularized Oseen    src/core/kernels.cpp:85-131
 *   Rotlet               src/core/kernels.cpp:206-242
 *
 * Design (nothing shared with the reference's CUDA driver, kernels.cu:80-123,
 * which used 32-thread blocks and accumulated into global memory every tile):
 *   - 256-thread blocks (4 wave64s), TPT targets per thread held in VGPRs;
 *     velocity accumulates in registers and is written once.
 *   - Sources reach the pair loop through scalar registers. Every lane of
 *     a wave works on the same source, so a source is wave-uniform data: a
 *     pack kernel (pack_sources, one launch ahead of pair_driver) writes the
 *     launch's sources into the workspace as packed records {r[3], f[SRCDIM],
 *     g[AUXDIM]}, and the pair loop reads them with scalar loads whose
 *     addresses derive from kernel arguments, blockIdx and loop counters
 *     only. Each source-consuming fp64 op has exactly one source operand,
 *     which it takes straight from an SGPR pair: no LDS, no barrier and no
 *     vector-side memory instruction in the loop. K::GROUP records are
 *     loaded at a time, two groups in flight (the loads of the next group
 *     issue before the arithmetic of the current one). The record buffer is
 *     padded by one group so that a whole group may be read past the last
 *     source; it is rebuilt on every call (strengths change every call) and
 *     only ever read by the pair kernel.
 *   - fp64 rsqrt: raw v_rsq_f64 + one 3-op Newton step that returns
 *     R = 2/sqrt(x) (see rsq_x2). The factor 2 (and its powers R^3 = 8/r^3,
 *     R^5 = 32/r^5) never costs a pair-loop instruction: where it is global
 *     the host divides Params::scale by K::ACC_FOLD (launch_params);
 *     stokeslet and oseen,
 *     which mix R and R^3, read a second copy g = f/4 of the strength for
 *     the dot product so that every accumulator is exactly 2x the plain
 *     sum. All rescalings are powers of two -> results are bit-identical
 *     to the 4-op form (for values that stay normal fp64).
 *   - The r^2==0 mask (reference: kernels.cu:39,70) is off the fast path.
 *     Each slice is walked in CHUNK-source pieces: a wave saves its
 *     accumulators, runs the chunk unmasked (a coincident pair gives
 *     rsq(0) = inf, 0*inf = NaN, so the accumulator goes NaN), tests the
 *     accumulators, and only if some lane saw a NaN (wave-uniform branch)
 *     restores them and reruns the chunk masked - same arithmetic, same
 *     source order, so the result does not depend on which path ran. A
 *     NaN that comes from the inputs takes the rerun once per chunk and
 *     stays NaN. Regularized oseen turns r = 0 into a finite 1/reg, so it
 *     tracks min(high dword of r^2) per chunk instead (one b32 op a pair).
 *     skelly_set_pair_fastpath(0) runs the masked path everywhere; by
 *     default small launches (under 128 chunks a block) stay masked too,
 *     see g_pair_fastpath.
 *   - Accumulation order per target is source order, fixed ->
 *     bit-reproducible for a given shard layout and slice count.
 *   - Source-split launches: gridDim.y source slices accumulate partials
 *     that a second kernel reduces in fixed slice order (deterministic).
 *     The slice count comes from the launch planner of pair_plan.hpp: every
 *     workgroup of a launch costs the same, so a CU's time goes with the
 *     number of workgroups it gets, and the planner picks the count whose
 *     blocks x slices workgroups divide most evenly over the CUs (the
 *     flagship's 977 blocks: 6 slices, 22.9 -> 23 workgroups a CU, instead of
 *     2 slices, 7.63 -> 8), with at least ~2048 sources a slice and the
 *     partial workspace capped. A pure function of shape, CU count and
 *     the functor's launch bound, so the summation order stays reproducible;
 *     skelly_set_pair_slices() forces a count for sweeps and tests.
 *   - The same driver evaluates the analytic velocity gradients of the four
 *     kernels (9 outputs a target, K::OUTDIM; functors further down) and
 *     the pressures of the Stokeslet, Oseen and stresslet fields (1 output).
 *   - One functor is no sum: Nearest keeps per target the smallest squared
 *     distance to an eligible source and that source's index. The driver
 *     serves it through three functor traits that default to what the sums
 *     need: the accumulators start from K::init (the reduction's neutral
 *     element, which an empty slice of a forced split writes), a target may
 *     carry more than its coordinates (K::TRGDIM), and reduce_partials folds
 *     a K::JOINT functor's partials a target at a time with K::combine.
 *
 * Roofline: compute-bound on the fp64 VALU. The kernels are
 * deliberately not GEMM-shaped: gfx950's fp64 matrix rate equals its vector
 * rate, so MFMA buys nothing here.
 */

#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <type_traits>

#include "launch_workspace.hpp"
#include "pair_functors.hpp"
#include "pair_kernels.hpp"
#include "pair_plan.hpp"

#define BLOCK 256

/* Sources per unmasked chunk between two accumulator checks, counted from the
 * slice start. Measured on MI355X, profiles/pair_fastpath.md. */
#ifndef SKELLY_CHUNK
#define SKELLY_CHUNK 64
#endif

/* ---- driver ----------------------------------------------------------- */

/* Write the launch's sources as packed records, the padding as zeros. One
 * thread per double of the buffer (coalesced stores); g = 0.25 * f is an
 * exact power-of-two product. */
template <typename K>
__global__ __launch_bounds__(BLOCK) void pack_sources(const double *__restrict__ r_src,
                                                      const double *__restrict__ f_src,
                                                      double *__restrict__ rec,
                                                      long long n_src) {
    constexpr int R = rec_doubles<K>();
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= R * rec_count<K>(n_src))
        return;
    const long long s = i / R;
    const int j = (int)(i - s * R);
    double v = 0.0;
    if (s < n_src) {
        if (j < 3)
            v = r_src[3 * s + j];
        else if (j < 3 + K::SRCDIM)
            v = f_src[K::SRCDIM * s + (j - 3)];
        else /* AUXDIM == SRCDIM where present */
            v = 0.25 * f_src[K::SRCDIM * s + (j - 3 - K::SRCDIM)];
    }
    rec[i] = v;
}

/* One group of records into registers. `src` is block-uniform (kernel
 * arguments, blockIdx and loop counters only) and the buffer is never written
 * by this kernel, so these are scalar loads into SGPRs. */
template <int N>
__device__ __forceinline__ void load_group(double (&dst)[N], const double *__restrict__ src) {
    /* Scalar loads return out of order, so the only wait there is is for all
     * of them: take the wait for the group loaded before (the one about to
     * be used) here, ahead of these loads. Behind them it would wait for
     * these as well. s_waitcnt lgkmcnt(0) with vmcnt and expcnt left alone. */
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < N; ++i)
        dst[i] = src[i];
    /* Pin the loads here: left alone, the scheduler sinks them below the
     * arithmetic of the group before, right in front of their own wait. */
    __builtin_amdgcn_sched_barrier(0);
}

/* The first `count` sources of a loaded group (all of them with FULL) onto
 * this thread's TPT targets, in source order. */
template <typename K, int TPT, bool MASKED, bool FULL>
__device__ __forceinline__ void pair_group(const double (&g)[K::GROUP * rec_doubles<K>()],
                                           const int count, const double (&tp)[TPT][K::TRGDIM],
                                           double (&acc)[TPT][K::OUTDIM],
                                           const typename K::Params &params, unsigned &zmin) {
    constexpr int R = rec_doubles<K>();
#pragma unroll
    for (int u = 0; u < K::GROUP; ++u) {
        if (!FULL && u >= count)
            break;
#pragma unroll
        for (int k = 0; k < TPT; ++k)
            K::template pair<MASKED>(tp[k], g + R * u, g + R * u + 3, g + R * u + 3 + K::SRCDIM,
                                     acc[k], params, zmin);
    }
}

/* The n >= 1 sources whose records start at `rec` onto this thread's TPT
 * targets, in source order. Two groups of K::GROUP records are in flight:
 * the scalar loads of the next group issue before the arithmetic of the
 * current one (scalar loads return out of order, so the only usable wait is
 * for all of them, and it falls behind a whole group of arithmetic). Loads
 * reach at most K::GROUP - 1 records past source n: the buffer's padding.
 * `a` comes in with the loads of the group at `rec` issued (load_group) and,
 * when n is a multiple of 2 * K::GROUP, goes out with those of the group at
 * source n issued: a chunk hands the next one its first group, so that only
 * a slice's first group is waited for with nothing to compute meanwhile. */
template <typename K, int TPT, bool MASKED>
__device__ __forceinline__ void pair_span(const double *__restrict__ rec, const int n,
                                          double (&a)[K::GROUP * rec_doubles<K>()],
                                          const double (&tp)[TPT][K::TRGDIM],
                                          double (&acc)[TPT][K::OUTDIM],
                                          const typename K::Params &params, unsigned &zmin) {
    constexpr int G = K::GROUP;
    constexpr int R = rec_doubles<K>();
    double b[G * R];
    int s = 0;
    for (; s + 2 * G <= n; s += 2 * G) {
        load_group(b, rec + R * (s + G));
        pair_group<K, TPT, MASKED, true>(a, G, tp, acc, params, zmin);
        load_group(a, rec + R * (s + 2 * G));
        pair_group<K, TPT, MASKED, true>(b, G, tp, acc, params, zmin);
    }
    /* 0 .. 2G-1 sources left; `a` holds the group at s */
    const int left = n - s;
    if (left > G) {
        load_group(b, rec + R * (s + G));
        pair_group<K, TPT, MASKED, true>(a, G, tp, acc, params, zmin);
        pair_group<K, TPT, MASKED, false>(b, left - G, tp, acc, params, zmin);
    } else {
        pair_group<K, TPT, MASKED, false>(a, left, tp, acc, params, zmin);
    }
}

/* PARTIAL=false: each block sums ALL sources for its targets and writes the
 * finished (scaled) velocities. PARTIAL=true (source-split, used when small
 * target counts would underfill the 256 CUs): gridDim.y slices partition the
 * sources; block (x, y) sums slice y for target tile x into
 * u_trg[y * OUTDIM*n_trg ...] UNSCALED; reduce_partials then sums the slices in
 * fixed slice order (deterministic) and applies the finish scale.
 * fastpath != 0 runs each chunk unmasked first (see the file header). */
template <typename K, int TPT, bool PARTIAL = false>
__global__ __launch_bounds__(BLOCK, K::MIN_WAVES) void pair_driver(const double *__restrict__ rec,
                                                     const double *__restrict__ r_trg,
                                                     double *__restrict__ u_trg,
                                                     long long n_src, long long n_trg,
                                                     long long slice_len,
                                                     typename K::Params params, int fastpath) {
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * (BLOCK * TPT);

    constexpr int TD = K::TRGDIM;
    double tp[TPT][TD];
    constexpr int OD = K::OUTDIM;
    double acc[TPT][OD];
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        long long it = base + (long long)k * BLOCK + tid;
        const long long itc = it < n_trg ? it : (n_trg > 0 ? n_trg - 1 : 0);
        tp[k][0] = r_trg[TD * itc + 0];
        tp[k][1] = r_trg[TD * itc + 1];
        tp[k][2] = r_trg[TD * itc + 2];
        if constexpr (TD > 3)
            tp[k][3] = r_trg[TD * itc + 3];
#pragma unroll
        for (int j = 0; j < OD; ++j)
            acc[k][j] = K::init(j);
    }

    /* An empty use of the target coordinates: the wait for their loads falls
     * here, once, instead of in the pair loop as one counted wait a target. */
#pragma unroll
    for (int k = 0; k < TPT; ++k)
        asm volatile("" : "+v"(tp[k][0]), "+v"(tp[k][1]), "+v"(tp[k][2]));
    if constexpr (TD > 3) {
#pragma unroll
        for (int k = 0; k < TPT; ++k)
            asm volatile("" : "+v"(tp[k][3]));
    }

    /* slice_len = ceil(n_src / gridDim.y) comes from the host: a 64-bit
     * division here would leave the slice start, and every record address
     * derived from it, in vector registers. */
    long long src_begin = 0, src_end = n_src;
    if (PARTIAL) {
        src_begin = (long long)blockIdx.y * slice_len;
        src_end = src_begin + slice_len < n_src ? src_begin + slice_len : n_src;
    }

    /* Kernels with a wired fast path walk the slice in chunks of
     * SKELLY_CHUNK sources counted from the slice start. The others have no
     * mask to skip, or always go through it: one span over the slice (in
     * pieces that keep pair_span's counters 32-bit). */
    constexpr bool CHUNKED = K::HAS_MASK && K::FASTPATH;
    constexpr int SPAN = CHUNKED ? SKELLY_CHUNK : (1 << 30);
    constexpr int R = rec_doubles<K>();
    static_assert(SPAN % (2 * K::GROUP) == 0, "a full span must hand on the next group");
    /* the group at the start of the span, loaded by the span before */
    double first[K::GROUP * R];
    if (src_begin < src_end)
        load_group(first, rec + R * src_begin);
    for (long long c0 = src_begin; c0 < src_end; c0 += SPAN) {
        const int n = (int)((src_end - c0 < SPAN) ? (src_end - c0) : SPAN);
        const double *span = rec + R * c0;
        unsigned zmin = ~0u;
        if (!CHUNKED) {
            pair_span<K, TPT, K::HAS_MASK>(span, n, first, tp, acc, params, zmin);
            continue;
        }
        bool masked = !fastpath;
        if (fastpath) {
            double saved[TPT][OD];
#pragma unroll
            for (int k = 0; k < TPT; ++k)
#pragma unroll
                for (int j = 0; j < OD; ++j)
                    saved[k][j] = acc[k][j];
            pair_span<K, TPT, false>(span, n, first, tp, acc, params, zmin);
            bool hit = zmin == 0u;
            if (K::NAN_PROBE) {
#pragma unroll
                for (int k = 0; k < TPT; ++k)
#pragma unroll
                    for (int j = 0; j < OD; ++j)
                        hit |= acc[k][j] != acc[k][j];
            }
            masked = __any(hit); /* wave-uniform */
            if (masked) {
#pragma unroll
                for (int k = 0; k < TPT; ++k)
#pragma unroll
                    for (int j = 0; j < OD; ++j)
                        acc[k][j] = saved[k][j];
                load_group(first, span); /* the rerun starts over */
            }
        }
        if (masked)
            pair_span<K, TPT, true>(span, n, first, tp, acc, params, zmin);
    }

    /* Recompute the target index from an opaque copy of tid: otherwise the
     * prologue's 64-bit index is kept live (or spilled) across the pair loop. */
    int tid_out = tid;
    asm volatile("" : "+v"(tid_out));
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        const long long it = base + (long long)k * BLOCK + tid_out;
        if (it < n_trg) {
            if (PARTIAL) {
                double *p = u_trg + (long long)blockIdx.y * OD * n_trg;
#pragma unroll
                for (int j = 0; j < OD; ++j)
                    p[OD * it + j] = acc[k][j];
            } else {
#pragma unroll
                for (int j = 0; j < OD; ++j)
                    u_trg[OD * it + j] = K::finish(acc[k][j], params);
            }
        }
    }
}

/* Sum source-slice partials in fixed slice order and apply the finish scale.
 * partial layout: [n_slices][n_trg][OUTDIM]; one thread per (target, component).
 * A K::JOINT functor's partials are one value a target: one thread per target
 * folds them with K::combine from K::init, in slice order. */
template <typename K>
__global__ __launch_bounds__(BLOCK) void reduce_partials(const double *__restrict__ partial,
                                                         double *__restrict__ u_trg,
                                                         long long n_trg, int n_slices,
                                                         typename K::Params params) {
    const long long n_out = K::OUTDIM * n_trg;
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if constexpr (K::JOINT) {
        constexpr int OD = K::OUTDIM;
        if (i >= n_trg)
            return;
        double a[OD], b[OD];
#pragma unroll
        for (int j = 0; j < OD; ++j)
            a[j] = K::init(j);
        for (int y = 0; y < n_slices; ++y) {
#pragma unroll
            for (int j = 0; j < OD; ++j)
                b[j] = partial[(long long)y * n_out + OD * i + j];
            K::combine(a, b);
        }
#pragma unroll
        for (int j = 0; j < OD; ++j)
            u_trg[OD * i + j] = K::finish(a[j], params);
    } else {
        if (i >= n_out)
            return;
        double s = 0.0;
        for (int y = 0; y < n_slices; ++y)
            s += partial[(long long)y * n_out + i];
        u_trg[i] = K::finish(s, params);
    }
}

/* skelly_nearest_*'s arguments as the Nearest functor reads them: one thread
 * per index writes source i's strength {i, group} and target i's four doubles
 * {r[3], group}. Without groups (both pointers null) every source is in group
 * 0 and every target in group -1. */
__global__ __launch_bounds__(BLOCK) void stage_nearest(const long long *__restrict__ src_group,
                                                       long long n_src,
                                                       const double *__restrict__ r_trg,
                                                       const long long *__restrict__ trg_group,
                                                       long long n_trg, double *__restrict__ f_src,
                                                       double *__restrict__ trg4) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n_src) {
        f_src[2 * i + 0] = (double)i;
        f_src[2 * i + 1] = src_group ? (double)src_group[i] : 0.0;
    }
    if (i < n_trg) {
        trg4[4 * i + 0] = r_trg[3 * i + 0];
        trg4[4 * i + 1] = r_trg[3 * i + 1];
        trg4[4 * i + 2] = r_trg[3 * i + 2];
        trg4[4 * i + 3] = trg_group ? (double)trg_group[i] : -1.0;
    }
}

/* The functor's {d^2, index} pairs into the caller's two arrays. */
__global__ __launch_bounds__(BLOCK) void unpack_nearest(const double *__restrict__ out2,
                                                        long long n_trg, double *__restrict__ d2,
                                                        long long *__restrict__ index) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_trg)
        return;
    d2[i] = out2[2 * i + 0];
    index[i] = (long long)out2[2 * i + 1];
}

/* ---- launch helpers (host) -------------------------------------------- */

namespace skelly {

/* Unmasked fast path of the pair kernels (see the file header). Mode, from
 * skelly_set_pair_fastpath() or else SKELLY_PAIR_FASTPATH:
 *   0  off: the masked path everywhere (A/B measurement, identity tests);
 *   1  auto (default): on for launches whose blocks each walk at least
 *      PAIR_FASTPATH_MIN_SRC sources;
 *   2  always on.
 * Why auto: when sources and targets coincide, a wave reruns up to 2*TPT = 8
 * chunks (its 4 x 64 consecutive targets straddle two chunks each). A full
 * grid hides that, but small launches are latency-bound on the one source
 * slice that holds the wave's own targets: measured on MI355X at
 * n_src = n_trg = 5e3 / 2e4 (1667 / 2000 sources a slice) always-on was
 * 24% / 17% SLOWER than the masked path, at 1e5 (9091 a slice) 7% faster
 * (profiles/pair_fastpath.md). 128 chunks bound the worst-case rerun at
 * 8/128 = 6% of the slice, under the ~8% the fast path gains. */
static constexpr long long PAIR_FASTPATH_MIN_SRC = 128LL * SKELLY_CHUNK;
static Knob g_pair_fastpath{"SKELLY_PAIR_FASTPATH", 1,
                            [](int v) { return v < 0 ? 0 : (v > 2 ? 2 : v); }};

/* Source-slice count of the split launches. 0 (default): the planner of
 * pair_plan.hpp decides. n >= 1, from skelly_set_pair_slices() or else
 * SKELLY_PAIR_SLICES: exactly n slices (clamped to n_src and to the
 * gridDim.y limit), for sweeps and tests; slices may then be shorter than a
 * chunk, start anywhere, and the last ones may be empty (they write zeros). */
static Knob g_pair_slices{"SKELLY_PAIR_SLICES", 0, [](int v) { return v < 0 ? 0 : v; }};

/* The device's CU count for the planner, asked once per device (256 on
 * MI355X, the default if the query fails). */
static int pair_device_cus() {
    static std::mutex mu;
    static std::map<int, int> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(dev);
    if (it != cache.end())
        return it->second;
    int n_cu = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        n_cu = prop.multiProcessorCount;
    (void)hipGetLastError();
    cache[dev] = n_cu;
    return n_cu;
}

/* f(std::integral_constant<int, TPT>) for the runtime tpt, instantiating only
 * what the functor's registers allow (K::MAX_TPT). */
template <typename K, typename F>
static auto dispatch_tpt(int tpt, F &&f) {
    if constexpr (K::MAX_TPT >= 4)
        if (tpt == 4)
            return f(std::integral_constant<int, 4>{});
    if constexpr (K::MAX_TPT >= 2)
        if (tpt == 2)
            return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 1>{});
}

template <typename K>
static inline int pick_tpt(long long n_trg) {
    /* Prefer 4 targets/thread (amortizes the per-source scalar loads 4x),
     * up to what the functor's registers hold; occupancy for small
     * target counts is recovered by source splitting, not by shrinking TPT. */
    if (K::MAX_TPT >= 4 && n_trg >= BLOCK * 4)
        return 4;
    if (K::MAX_TPT >= 2 && n_trg >= BLOCK * 2)
        return 2;
    return 1;
}

/* pack_sources<K> over the whole record buffer, padding included. */
template <typename K>
static void launch_pack(const double *r_src, const double *f_src, long long n_src, double *rec,
                        hipStream_t stream) {
    const long long total = (long long)rec_doubles<K>() * rec_count<K>(n_src);
    hipLaunchKernelGGL((pack_sources<K>), dim3((unsigned)((total + BLOCK - 1) / BLOCK)),
                       dim3(BLOCK), 0, stream, r_src, f_src, rec, n_src);
}

/* What a launch of n_trg >= 1 targets is made of: targets a thread, target
 * blocks, source slices, the fast-path switch, and the doubles of workspace
 * it takes (the packed source records, then, for split launches, the
 * partials of every slice). */
struct PairLaunch {
    int tpt;
    long long blocks;
    int n_slices;
    int fast;
    size_t rec_doubles_total;
    size_t partial_doubles;
    size_t doubles() const { return rec_doubles_total + partial_doubles; }
};

template <typename K>
static PairLaunch plan_launch(long long n_src, long long n_trg) {
    PairLaunch l;
    l.tpt = pick_tpt<K>(n_trg);
    l.blocks = (n_trg + (long long)BLOCK * l.tpt - 1) / ((long long)BLOCK * l.tpt);

    /* Source slices from the CU load-balance model (pair_plan.hpp): the
     * slice count that leaves the CUs the least uneven numbers of
     * workgroups, within the slice-length floor and the workspace cap. */
    /* wg_per_cu: the functor's launch bound, as the planner's constants were
     * fitted with. Without LDS the occupancy query answers more, and the
     * plans (with them the summation order) are not to move with it. */
    const PairPlan plan =
        pair_plan(n_src, n_trg, K::MAX_TPT, K::OUTDIM, g_pair_fastpath.get(),
                  PAIR_FASTPATH_MIN_SRC, pair_device_cus(), K::MIN_WAVES, g_pair_slices.get());
    l.n_slices = plan.n_slices;
    l.fast = plan.fast;
    l.rec_doubles_total = (size_t)rec_doubles<K>() * rec_count<K>(n_src);
    l.partial_doubles = l.n_slices > 1 ? (size_t)l.n_slices * K::OUTDIM * n_trg : 0;
    return l;
}

/* The kernels of launch `l` onto `stream`, working in the l.doubles() doubles
 * at `ws`. r_trg is (n_trg, K::TRGDIM); `params` as launch_params<K> made
 * them. */
template <typename K>
static void enqueue_pair(const PairLaunch &l, double *ws, const double *r_src,
                         const double *f_src, const double *r_trg, double *u_trg,
                         long long n_src, long long n_trg, typename K::Params params,
                         hipStream_t stream) {
    const int tpt = l.tpt, n_slices = l.n_slices, fast = l.fast;
    const long long blocks = l.blocks;
    double *rec = ws;
    double *partials = rec + l.rec_doubles_total;

    const long long slice_len = (n_src + n_slices - 1) / n_slices;
    dim3 block(BLOCK);
    launch_pack<K>(r_src, f_src, n_src, rec, stream);
    /* pair_driver<K, tpt, PARTIAL> over `grid` into `dst` */
    auto launch_driver = [&](auto partial, dim3 grid, double *dst) {
        dispatch_tpt<K>(tpt, [&](auto t) {
            hipLaunchKernelGGL((pair_driver<K, decltype(t)::value, decltype(partial)::value>),
                               grid, block, 0, stream, rec, r_trg, dst, n_src, n_trg, slice_len,
                               params, fast);
        });
    };
    if (n_slices == 1) {
        launch_driver(std::false_type{}, dim3((unsigned)blocks), u_trg);
    } else {
        /* split path: same TPT, gridDim.y source slices into the partials */
        launch_driver(std::true_type{}, dim3((unsigned)blocks, (unsigned)n_slices), partials);
        const long long rthreads = K::JOINT ? n_trg : K::OUTDIM * n_trg;
        const long long rblocks = (rthreads + BLOCK - 1) / BLOCK;
        hipLaunchKernelGGL((reduce_partials<K>), dim3((unsigned)rblocks), block, 0, stream,
                           partials, u_trg, n_trg, n_slices, params);
    }
}

template <typename K>
static hipError_t launch_pair(const double *r_src, const double *f_src, const double *r_trg,
                              double *u_trg, long long n_src, long long n_trg,
                              typename K::Params params, hipStream_t stream) {
    if (n_trg <= 0)
        return hipSuccess;
    const PairLaunch l = plan_launch<K>(n_src, n_trg);
    LaunchWorkspace workspace;
    const hipError_t err = workspace.acquire(stream, l.doubles() * sizeof(double));
    if (err != hipSuccess)
        return err;
    enqueue_pair<K>(l, workspace.get(), r_src, f_src, r_trg, u_trg, n_src, n_trg, params, stream);
    return workspace.finish(hipGetLastError());
}

/* f(K{}) for the functor the enum names. */
template <typename F>
static auto with_kernel(PairKernel kernel, F &&f) {
    switch (kernel) {
    case PairKernel::Stokeslet:
        return f(Stokeslet{});
    case PairKernel::Stresslet:
        return f(Stresslet{});
    case PairKernel::OseenContract:
        return f(OseenContract{});
    case PairKernel::Rotlet:
        return f(Rotlet{});
    case PairKernel::StressletNormalDensity:
        return f(StressletNormalDensity{});
    case PairKernel::StokesletGrad:
        return f(StokesletGrad{});
    case PairKernel::StressletGrad:
        return f(StressletGrad{});
    case PairKernel::RotletGrad:
        return f(RotletGrad{});
    case PairKernel::StokesletPressure:
        return f(StokesletPressure{});
    case PairKernel::StressletPressure:
        return f(StressletPressure{});
    case PairKernel::Nearest:
        return f(Nearest{});
    }
    __builtin_unreachable();
}

PairDims pair_kernel_dims(PairKernel kernel) {
    return with_kernel(kernel, [](auto k) {
        using K = decltype(k);
        return PairDims{K::SRCDIM, K::OUTDIM};
    });
}

hipError_t launch_pair_kernel(PairKernel kernel, const double *r_src, const double *f_src,
                              const double *r_trg, double *out, long long n_src, long long n_trg,
                              double scale, double reg, double eps, hipStream_t stream) {
    return with_kernel(kernel, [&](auto k) {
        using K = decltype(k);
        return launch_pair<K>(r_src, f_src, r_trg, out, n_src, n_trg,
                              launch_params<K>(scale, reg, eps), stream);
    });
}

/* The Nearest functor on the entry points' own types. One workspace block
 * holds the launch's records and partials, then the staged strengths
 * (n_src, 2), the 4-wide targets and the functor's (n_trg, 2) result, which
 * unpack_nearest splits into d2 and index. */
hipError_t launch_nearest(const double *r_src, const long long *src_group, long long n_src,
                          const double *r_trg, const long long *trg_group, long long n_trg,
                          double *d2, long long *index, hipStream_t stream) {
    if (n_trg <= 0)
        return hipSuccess;
    using K = Nearest;
    const PairLaunch l = plan_launch<K>(n_src, n_trg);
    const size_t f_doubles = (size_t)K::SRCDIM * n_src, trg_doubles = (size_t)K::TRGDIM * n_trg;
    const size_t out_doubles = (size_t)K::OUTDIM * n_trg;
    LaunchWorkspace workspace;
    const hipError_t err = workspace.acquire(
        stream, (l.doubles() + f_doubles + trg_doubles + out_doubles) * sizeof(double));
    if (err != hipSuccess)
        return err;
    double *f_src = workspace.get() + l.doubles();
    double *trg4 = f_src + f_doubles;
    double *out2 = trg4 + trg_doubles;
    const long long n_max = n_src > n_trg ? n_src : n_trg;
    const dim3 grid((unsigned)((n_max + BLOCK - 1) / BLOCK)), block(BLOCK);
    hipLaunchKernelGGL(stage_nearest, grid, block, 0, stream, src_group, n_src, r_trg, trg_group,
                       n_trg, f_src, trg4);
    enqueue_pair<K>(l, workspace.get(), r_src, f_src, trg4, out2, n_src, n_trg,
                    launch_params<K>(1.0, 0.0, 0.0), stream);
    hipLaunchKernelGGL(unpack_nearest, dim3((unsigned)((n_trg + BLOCK - 1) / BLOCK)), block, 0,
                       stream, out2, n_trg, d2, index);
    return workspace.finish(hipGetLastError());
}

void launch_pack_sources(PairKernel kernel, const double *r_src, const double *f_src,
                         long long n_src, double *rec, hipStream_t stream) {
    with_kernel(kernel, [&](auto k) { launch_pack<decltype(k)>(r_src, f_src, n_src, rec, stream); });
}

/* ---- batched oseen_tensor_direct dense builder (kernels.cpp:146-195) ---
 * points: (nf, n, 3); G: (nf, 3n, 3n) row-major (G is symmetric, so this is
 * bit-identical to the reference's col-major). One thread per (fiber, trg,
 * src) pair writes its 3x3 block. Setup-time op (per-fiber self-stokeslet,
 * fiber_finite_difference.cpp:56), not GMRES-hot. */
__global__ __launch_bounds__(BLOCK) void oseen_tensor_kernel(const double *__restrict__ pts,
                                                             double *__restrict__ G,
                                                             long long nf, long long n,
                                                             double factor, double reg2,
                                                             double eps2) {
    const long long idx = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long total = nf * n * n;
    if (idx >= total)
        return;
    const long long f = idx / (n * n);
    const long long r = idx % (n * n);
    const long long t = r / n, s = r % n;
    const double *p = pts + f * n * 3;
    const double dx = p[3 * s + 0] - p[3 * t + 0];
    const double dy = p[3 * s + 1] - p[3 * t + 1];
    const double dz = p[3 * s + 2] - p[3 * t + 2];
    double dr2 = dx * dx;
    dr2 = __builtin_fma(dy, dy, dr2);
    dr2 = __builtin_fma(dz, dz, dr2);
    const double denom2 = (dr2 > eps2) ? dr2 : dr2 + reg2;
    double y = rsq_refined(denom2);
    y = (dr2 == 0.0) ? 0.0 : y; /* dr2==0 -> whole block zero (cpp:166-167) */
    const double fr = factor * y;
    const double gr = fr * (y * y);
    const long long ld = 3 * n;
    double *blk = G + f * ld * ld + (3 * t) * ld + 3 * s;
    const double d[3] = {dx, dy, dz};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
            blk[a * ld + b] = (a == b ? fr : 0.0) + gr * d[a] * d[b];
}

/* stresslet_times_normal dense builder (kernels.cpp:264-287):
 * Snormal block (i, j) = -3/(4*pi) * (d.n_j)/r^5 * d d^T, d = r_i - r_j;
 * i == j blocks zero (kernels.cpp:273-274); r < eps regularized
 * (kernels.cpp:278-279). Output is (3n, 3n) C row-major with
 * out[3i+a][3j+b] = Snormal(3i+a, 3j+b) — same logical indexing as the
 * reference (its Eigen buffer is col-major; the MATRIX is identical). */
__global__ __launch_bounds__(BLOCK) void stresslet_normal_kernel(
    const double *__restrict__ pts, const double *__restrict__ normals, double *__restrict__ G,
    long long n, double factor, double reg2, double eps2) {
    const long long idx = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= n * n)
        return;
    const long long i = idx / n, j = idx % n;
    const long long ld = 3 * n;
    double *blk = G + (3 * i) * ld + 3 * j;
    if (i == j) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b)
                blk[a * ld + b] = 0.0;
        return;
    }
    const double dx = pts[3 * i + 0] - pts[3 * j + 0];
    const double dy = pts[3 * i + 1] - pts[3 * j + 1];
    const double dz = pts[3 * i + 2] - pts[3 * j + 2];
    double dr2 = dx * dx;
    dr2 = __builtin_fma(dy, dy, dr2);
    dr2 = __builtin_fma(dz, dz, dr2);
    const double denom2 = (dr2 < eps2) ? dr2 + reg2 : dr2;
    const double y = rsq_refined(denom2);
    const double y2 = y * y;
    const double rinv5 = y * y2 * y2;
    double ddn = dx * normals[3 * j + 0];
    ddn = __builtin_fma(dy, normals[3 * j + 1], ddn);
    ddn = __builtin_fma(dz, normals[3 * j + 2], ddn);
    const double c = factor * ddn * rinv5;
    const double d[3] = {dx, dy, dz};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
            blk[a * ld + b] = c * d[a] * d[b];
}

hipError_t launch_stresslet_times_normal(const double *pts, const double *normals, double *G,
                                         long long n, double reg, double eps,
                                         hipStream_t stream) {
    if (n <= 0)
        return hipSuccess;
    const long long blocks = (n * n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(stresslet_normal_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, stream,
                       pts, normals, G, n, -3.0 / (4.0 * M_PI), reg * reg, eps * eps);
    return hipGetLastError();
}

hipError_t launch_oseen_tensor_batched(const double *pts, double *G, long long nf, long long n,
                                       double eta, double reg, double eps, hipStream_t stream) {
    if (nf <= 0 || n <= 0)
        return hipSuccess;
    const double factor = 1.0 / (8.0 * M_PI * eta);
    const long long total = nf * n * n;
    const long long blocks = (total + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(oseen_tensor_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, stream, pts,
                       G, nf, n, factor, reg * reg, eps * eps);
    return hipGetLastError();
}

} // namespace skelly

/* Runtime override of the unmasked pair fast path: 0 off, 1 auto, 2 always
 * (see g_pair_fastpath above). Results do not depend on it. */
extern "C" void skelly_set_pair_fastpath(int mode) {
    skelly::g_pair_fastpath.forced = skelly::g_pair_fastpath.clamp(mode);
}

/* Runtime override of the source-slice count: 0 = the planner, n >= 1 =
 * exactly n slices (see g_pair_slices above). Results depend on it only
 * through the summation order. */
extern "C" void skelly_set_pair_slices(int n) {
    skelly::g_pair_slices.forced = skelly::g_pair_slices.clamp(n);
}
