/* probe_kernels.hip — the microbenchmarks and probes behind the numbers that
 * DESIGN.md and profiles/ quote: the fp64 FMA peak, the issue-cost probe and
 * the rsqrt accuracy probe. Nothing here is on a hot path; it is a unit of its
 * own so that the pair kernels' unit holds the pair kernels only. */

#include <hip/hip_runtime.h>

#include "pair_functors.hpp"
#include "pair_kernels.hpp"

#define BLOCK 256

namespace skelly {

/* ---- fp64 FMA peak microbenchmark (roofline denominator) -------------- */

__global__ __launch_bounds__(256) void fp64_fma_peak_kernel(double *out, int iters) {
    /* 16 independent accumulators: with 8, the chain is fp64-FMA
     * dependent-latency-bound (~20% below issue rate) and under-reports the
     * sustained peak. */
    double a[16];
#pragma unroll
    for (int k = 0; k < 16; ++k)
        a[k] = 1.0 + 1e-9 * threadIdx.x + 0.1 * k;
    const double b = 1.0 + 1e-12, c = 1e-12;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            a[k] = __builtin_fma(a[k], b, c);
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        s += a[k];
    if (s == -1.0) /* never true; defeats DCE without a store per thread */
        out[blockIdx.x] = s;
}

hipError_t run_fp64_peak(double *out_tflops) {
    const int iters = 100000, blocks = 2048, threads = 256;
    double *d;
    hipError_t err = hipMalloc(&d, blocks * sizeof(double));
    if (err != hipSuccess)
        return err;
    hipEvent_t t0, t1;
    (void)hipEventCreate(&t0);
    (void)hipEventCreate(&t1);
    /* warmup */
    hipLaunchKernelGGL(fp64_fma_peak_kernel, dim3(blocks), dim3(threads), 0, 0, d, iters / 10);
    (void)hipEventRecord(t0);
    hipLaunchKernelGGL(fp64_fma_peak_kernel, dim3(blocks), dim3(threads), 0, 0, d, iters);
    (void)hipEventRecord(t1);
    err = hipEventSynchronize(t1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, t0, t1);
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    (void)hipFree(d);
    if (err != hipSuccess)
        return err;
    const double flops = 2.0 * 16.0 * (double)iters * (double)blocks * threads;
    *out_tflops = flops / (ms * 1e-3) / 1e12;
    return hipSuccess;
}

/* ---- issue-cost probe (what a non-FMA instruction costs the FMA pipe) -----
 * The body of fp64_fma_peak_kernel four times over (64 independent
 * v_fma_f64 on 16 accumulators) with 4 instructions of one kind put in front.
 * It was written when the pair loop still read its sources from LDS (16
 * v_rsq_f64 and 18 ds_read_b128 to 320 fp64 ops, the mix it imitates) and
 * priced those two instructions on MI355X at 3.8 and 1.0 FMA slots.
 * profiles/pair_scalar.md weighs the figures against the loop that then took
 * the LDS reads out for scalar record loads; today's loop has none, and the
 * rsq figure is the one still in use. Kept because that record cites it:
 *   PROBE_NONE  nothing (the base time);
 *   PROBE_RSQ   4 independent v_rsq_f64;
 *   PROBE_LDS   4 ds_read_b128 of one address for all lanes (a broadcast),
 *               waited for behind the 64 FMAs.
 * What an inserted instruction costs is the FMA rate it takes away. */
enum { PROBE_NONE = 0, PROBE_RSQ = 1, PROBE_LDS = 2 };
constexpr int PROBE_FMA = 64, PROBE_INSERTED = 4, PROBE_ITERS = 25000;

template <int MODE>
__global__ __launch_bounds__(256) void issue_probe_kernel(double *out, int iters) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    __shared__ __attribute__((aligned(16))) double lds[2 * PROBE_INSERTED];
    if (threadIdx.x < 2 * PROBE_INSERTED)
        lds[threadIdx.x] = 1.0 + threadIdx.x;
    __syncthreads();
    /* the low 32 bits of a flat LDS address are the LDS offset */
    const unsigned lds_addr = (unsigned)(size_t)lds;
    double a[16], x[PROBE_INSERTED];
#pragma unroll
    for (int k = 0; k < 16; ++k)
        a[k] = 1.0 + 1e-9 * threadIdx.x + 0.1 * k;
#pragma unroll
    for (int j = 0; j < PROBE_INSERTED; ++j)
        x[j] = 2.0 + j + 1e-3 * threadIdx.x;
    const double b = 1.0 + 1e-12, c = 1e-12;
    for (int i = 0; i < iters; ++i) {
        double y[PROBE_INSERTED];
        d2 v[PROBE_INSERTED];
        if (MODE == PROBE_RSQ) {
#pragma unroll
            for (int j = 0; j < PROBE_INSERTED; ++j)
                asm volatile("v_rsq_f64 %0, %1" : "=v"(y[j]) : "v"(x[j]));
        }
        if (MODE == PROBE_LDS) {
#pragma unroll
            for (int j = 0; j < PROBE_INSERTED; ++j)
                asm volatile("ds_read_b128 %0, %1 offset:%2"
                             : "=v"(v[j])
                             : "v"(lds_addr), "i"(16 * j));
        }
#pragma unroll
        for (int r = 0; r < PROBE_FMA / 16; ++r)
#pragma unroll
            for (int k = 0; k < 16; ++k)
                a[k] = __builtin_fma(a[k], b, c);
        /* the destinations stay allocated until the reads have landed */
        if (MODE == PROBE_LDS) {
            asm volatile("s_waitcnt lgkmcnt(0)");
#pragma unroll
            for (int j = 0; j < PROBE_INSERTED; ++j)
                asm volatile("" ::"v"(v[j]));
        }
        if (MODE == PROBE_RSQ) {
#pragma unroll
            for (int j = 0; j < PROBE_INSERTED; ++j)
                asm volatile("" ::"v"(y[j]));
        }
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        s += a[k];
    if (s == -1.0) /* never true; defeats DCE without a store per thread */
        out[blockIdx.x] = s;
}

template <int MODE>
static hipError_t time_issue_probe(double *d, hipEvent_t t0, hipEvent_t t1, float *ms) {
    const int iters = PROBE_ITERS, blocks = 2048, threads = 256;
    hipLaunchKernelGGL(issue_probe_kernel<MODE>, dim3(blocks), dim3(threads), 0, 0, d, iters / 10);
    (void)hipEventRecord(t0);
    hipLaunchKernelGGL(issue_probe_kernel<MODE>, dim3(blocks), dim3(threads), 0, 0, d, iters);
    (void)hipEventRecord(t1);
    const hipError_t err = hipEventSynchronize(t1);
    (void)hipEventElapsedTime(ms, t0, t1);
    return err;
}

/* out[0], out[1]: what one v_rsq_f64 and one broadcast ds_read_b128 cost, in
 * issue slots of a v_fma_f64 (4 cycles of the SIMD each):
 * (t_with - t_base) / t_base * PROBE_FMA / PROBE_INSERTED. out[2]: the base
 * run's TFLOP/s, to check it against run_fp64_peak. The three runs are taken
 * twice, alternating; the second round is reported. */
hipError_t run_issue_cost_probe(double *out) {
    const int blocks = 2048;
    double *d;
    hipError_t err = hipMalloc(&d, blocks * sizeof(double));
    if (err != hipSuccess)
        return err;
    hipEvent_t t0, t1;
    (void)hipEventCreate(&t0);
    (void)hipEventCreate(&t1);
    float base = 0, rsq = 0, lds = 0;
    for (int round = 0; round < 2 && err == hipSuccess; ++round) {
        err = time_issue_probe<PROBE_NONE>(d, t0, t1, &base);
        if (err == hipSuccess)
            err = time_issue_probe<PROBE_RSQ>(d, t0, t1, &rsq);
        if (err == hipSuccess)
            err = time_issue_probe<PROBE_LDS>(d, t0, t1, &lds);
    }
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    (void)hipFree(d);
    if (err != hipSuccess)
        return err;
    const double per = (double)PROBE_FMA / PROBE_INSERTED;
    out[0] = (rsq - base) / base * per;
    out[1] = (lds - base) / base * per;
    out[2] = 2.0 * PROBE_FMA * (double)PROBE_ITERS * blocks * 256 / (base * 1e-3) / 1e12;
    return hipSuccess;
}

/* ---- rsqrt accuracy probe (what the functors' one primitive returns) ----
 * seed[i] = the raw v_rsq_f64 of x[i], refined[i] = rsq_x2(x[i]), the very
 * function the functors and builders call. One thread an argument; measured
 * against a long double 1/sqrt(x) in tests/test_gpu_rsq.py
 * (profiles/pair_accuracy.md). */
__global__ __launch_bounds__(BLOCK) void rsq_probe_kernel(const double *__restrict__ x,
                                                          double *__restrict__ seed,
                                                          double *__restrict__ refined,
                                                          long long n) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n)
        return;
    const double xi = x[i];
    double y;
    asm("v_rsq_f64 %0, %1" : "=v"(y) : "v"(xi));
    seed[i] = y;
    refined[i] = rsq_x2(xi);
}

hipError_t launch_rsq_probe(const double *x, double *seed, double *refined, long long n,
                            hipStream_t stream) {
    if (n <= 0)
        return hipSuccess;
    const long long blocks = (n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(rsq_probe_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, stream, x, seed,
                       refined, n);
    return hipGetLastError();
}

} // namespace skelly
