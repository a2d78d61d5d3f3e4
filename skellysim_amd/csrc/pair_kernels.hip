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
 *     the host divides Params::scale by K::ACC_FOLD; stokeslet and oseen,
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
 *
 * Roofline: compute-bound on the fp64 VALU. The kernels are
 * deliberately not GEMM-shaped: gfx950's fp64 matrix rate equals its vector
 * rate, so MFMA buys nothing here.
 */

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "pair_kernels.hpp"
#include "pair_plan.hpp"

#define BLOCK 256

/* Sources per unmasked chunk between two accumulator checks, counted from the
 * slice start. Measured on MI355X, profiles/pair_fastpath.md. */
#ifndef SKELLY_CHUNK
#define SKELLY_CHUNK 64
#endif

/* Sources per group of scalar loads of the 9-double records (stokeslet,
 * oseen, rotlet, normal-density stresslet: 18 SGPRs a source). Two groups are
 * in flight, so a group costs 2 x 18 x GROUP of the ~100 SGPRs a wave has:
 * 2 fits, 4 does not (profiles/pair_scalar.md). */
#ifndef SKELLY_GROUP
#define SKELLY_GROUP 2
#endif

/* R = 2/sqrt(x): v_rsq_f64 + one refinement step with the constant factor
 * left out. Inputs here are finite and >= 0; x == 0 gives NaN (inf seed,
 * 0*inf), which the caller masks or detects. */
__device__ inline double rsq_x2(double x) {
    double y;
    asm("v_rsq_f64 %0, %1" : "=v"(y) : "v"(x));
#ifdef SKELLY_RSQ_PRECISE
    /* 5-op Householder (2nd order) step — the same polish ROCm libm applies:
     * cubic convergence, <= 2 ulp of fp64 — plus the doubling, so that the
     * folded scales below hold for this variant too. */
    const double e = __builtin_fma(-x * y, y, 1.0);
    const double c = __builtin_fma(e, 0.375, 0.5);
    return 2.0 * __builtin_fma(y * e, c, y);
#else
    /* Default: quadratic Newton step y' = (0.5*y) * (3 - (x*y)*y), issued as
     * the 3 ops t = x*y, q = fma(-t, y, 3), R = y*q = 2y' (exactly: the
     * missing 0.5 is a power of two). Measured on MI355X
     * (profiles/rocprof_r01.md): identical norm-relative parity vs the CPU
     * oracle (~5e-16 at 2e4x4096 incl. near-coincident pairs) and
     * +4.6%/+2.9%/+2.2% on stokeslet/stresslet/oseen over the Householder
     * form. That parity is a property of sums over thousands of sources, not
     * of a single pair: v_rsq_f64's seed is good to 5.2e-8 relative (2^-24.2,
     * measured by skelly_rsq_accuracy_probe over 2^17 arguments,
     * profiles/pair_accuracy.md), so R carries 1.5 e^2 = up to 36 u
     * (4.0e-15, u = 2^-53) on top of the step's 2.5 u of rounding, and a
     * term in R^p p times that. tests/pair_reference.py bounds it by
     * E_RSQ = 1.5 (2 e)^2 + 2.5 u = 1.62e-14. */
    const double t = x * y;
    const double q = __builtin_fma(-t, y, 3.0);
    return y * q;
#endif
}

/* 1/sqrt(x) for the dense builders below (setup-time, not hot). */
__device__ inline double rsq_refined(double x) { return 0.5 * rsq_x2(x); }

/* ---- kernel functors -------------------------------------------------
 * pair<MASKED>() adds one source's contribution to one target's
 * accumulators. With R = 2/r the accumulators hold ACC_FOLD times the plain
 * sum; the launch helpers divide Params::scale by ACC_FOLD. make_params()
 * (host) builds Params from the C entry point's (scale, reg, eps).
 *   HAS_MASK   the kernel zeroes coincident pairs; MASKED=false leaves the
 *              select out and must make a coincident pair detectable.
 *   NAN_PROBE  an unmasked coincident pair turns the accumulators NaN
 *              (else pair<false> lowers `zmin` to 0 on one).
 *   AUXDIM     doubles per source of the record's second copy g = f/4 (0: none).
 *   OUTDIM     accumulators and outputs per target (3 velocity components,
 *              9 for the gradient functors further down).
 *   MAX_TPT    most targets a thread holds (register budget).
 *   GROUP      sources per group of scalar record loads (SGPR budget: two
 *              groups of GROUP x 2 x (3 + SRCDIM + AUXDIM) SGPRs are live).
 *   FASTPATH   the unmasked chunk-rerun path is wired (needs HAS_MASK). */

struct VelocityTraits {
    static constexpr int OUTDIM = 3;
    static constexpr int MAX_TPT = 4;
    static constexpr int GROUP = SKELLY_GROUP;
    static constexpr bool FASTPATH = true;
};

struct Stokeslet : VelocityTraits {
    static constexpr int MIN_WAVES = 3;
    static constexpr int SRCDIM = 3;
    static constexpr int AUXDIM = 3;
    static constexpr bool HAS_MASK = true;
    static constexpr bool NAN_PROBE = true;
    static constexpr double ACC_FOLD = 2.0;
    struct Params {
        double scale; /* 1/(8*pi) [ / eta when folded] / ACC_FOLD */
    };
    static Params make_params(double scale, double, double) { return {scale}; }
    /* u += (1/r)(f + rhat (f.rhat)); r = t - s; r==0 -> 0 (kernels.cu:62-76).
     * With R = 2/r and g = f/4: (g.d) R^2 = (f.d)/r^2, so each term is
     * R (f + d (f.d)/r^2) = 2x the plain one. */
    template <bool MASKED>
    __device__ static inline void pair(const double t[3], const double sp[3], const double f[3],
                                       const double g[3], double acc[3], const Params &,
                                       unsigned &) {
        const double dx = t[0] - sp[0];
        const double dy = t[1] - sp[1];
        const double dz = t[2] - sp[2];
        double r2 = dx * dx;
        r2 = __builtin_fma(dy, dy, r2);
        r2 = __builtin_fma(dz, dz, r2);
        double rinv = rsq_x2(r2);
        if (MASKED)
            rinv = (r2 == 0.0) ? 0.0 : rinv; /* kernels.cu:70 */
        const double rinv2 = rinv * rinv;
        double fdotr = g[0] * dx;
        fdotr = __builtin_fma(g[1], dy, fdotr);
        fdotr = __builtin_fma(g[2], dz, fdotr);
        const double inner = fdotr * rinv2;
        acc[0] = __builtin_fma(rinv, __builtin_fma(dx, inner, f[0]), acc[0]);
        acc[1] = __builtin_fma(rinv, __builtin_fma(dy, inner, f[1]), acc[1]);
        acc[2] = __builtin_fma(rinv, __builtin_fma(dz, inner, f[2]), acc[2]);
    }
    __device__ static inline double finish(double a, const Params &p) { return a * p.scale; }
};

struct Stresslet : VelocityTraits {
    static constexpr int MIN_WAVES = 2;
    static constexpr int GROUP = 1; /* 24 SGPRs a source */
    static constexpr int SRCDIM = 9;
    static constexpr int AUXDIM = 0;
    static constexpr bool HAS_MASK = true;
    static constexpr bool NAN_PROBE = true;
    static constexpr double ACC_FOLD = 32.0; /* R^5 = 32/r^5 */
    struct Params {
        double scale; /* 1/(8*pi) [ / eta when folded] / ACC_FOLD */
    };
    static Params make_params(double scale, double, double) { return {scale}; }
    /* u += -3 (d^T S d)/r^5 d; d = t - s; r==0 -> 0 (kernels.cu:29-54) */
    template <bool MASKED>
    __device__ static inline void pair(const double t[3], const double sp[3], const double f[9],
                                       const double *, double acc[3], const Params &,
                                       unsigned &) {
        const double dx = t[0] - sp[0];
        const double dy = t[1] - sp[1];
        const double dz = t[2] - sp[2];
        const double dxx = dx * dx, dyy = dy * dy, dzz = dz * dz;
        double dr2 = dxx + dyy;
        dr2 += dzz;
        const double rinv = rsq_x2(dr2);
        const double rinv2 = rinv * rinv;
        double rinv5 = rinv * rinv2 * rinv2;
        if (MASKED)
            rinv5 = (dr2 == 0.0) ? 0.0 : rinv5; /* kernels.cu:39 */
        /* coeff = sxx dx^2 + syy dy^2 + szz dz^2 + (sxy+syx) dx dy
         *       + (sxz+szx) dx dz + (syz+szy) dy dz   (kernels.cu:45-48) */
        double coeff = f[0] * dxx;
        coeff = __builtin_fma(f[4], dyy, coeff);
        coeff = __builtin_fma(f[8], dzz, coeff);
        coeff = __builtin_fma(f[1] + f[3], dx * dy, coeff);
        coeff = __builtin_fma(f[2] + f[6], dx * dz, coeff);
        coeff = __builtin_fma(f[5] + f[7], dy * dz, coeff);
        coeff *= -3.0 * rinv5;
        acc[0] = __builtin_fma(dx, coeff, acc[0]);
        acc[1] = __builtin_fma(dy, coeff, acc[1]);
        acc[2] = __builtin_fma(dz, coeff, acc[2]);
    }
    __device__ static inline double finish(double a, const Params &p) { return a * p.scale; }
};

struct OseenContract : VelocityTraits {
    static constexpr int MIN_WAVES = 3;
    static constexpr int SRCDIM = 3;
    static constexpr int AUXDIM = 3;
    static constexpr bool HAS_MASK = true;
    static constexpr bool NAN_PROBE = false; /* r = 0 regularizes to a finite 1/reg */
    static constexpr double ACC_FOLD = 2.0;
    struct Params {
        double scale; /* factor = 1/(8*pi*eta) / ACC_FOLD, hoisted out of the pair loop */
        double reg2;
        double eps2;
    };
    static Params make_params(double scale, double reg, double eps) {
        return {scale, reg * reg, eps * eps};
    }
    /* kernels.cpp:96-127: dr==0 skipped; dr > eps -> fr=1/dr, gr=1/dr^3;
     * else fr=1/sqrt(dr^2+reg^2), gr that cubed. The dr > eps comparison is
     * evaluated as dr2 > eps^2 (monotone equivalent for exact values; can
     * differ only when sqrt rounding straddles eps itself). `factor` is
     * applied once at the end (linear in the sum). With y = 2*fr and
     * g = rho/4: y^3 (d.g) = 2 gr (d.rho), so both terms are 2x.
     * Unmasked, a coincident pair would add the finite fr*rho, so the high
     * dword of dr2 is min-tracked instead: 0 there means dr2 < 2^-1042
     * (the exponent field and the top 20 mantissa bits are zero: zero or a
     * small subnormal) and sends the chunk to the masked rerun. */
    template <bool MASKED>
    __device__ static inline void pair(const double t[3], const double sp[3], const double rho[3],
                                       const double g[3], double acc[3], const Params &p,
                                       unsigned &zmin) {
        const double dx = sp[0] - t[0]; /* src - trg, kernels.cpp:99-101 */
        const double dy = sp[1] - t[1];
        const double dz = sp[2] - t[2];
        double dr2 = dx * dx;
        dr2 = __builtin_fma(dy, dy, dr2);
        dr2 = __builtin_fma(dz, dz, dr2);
        const double denom2 = (dr2 > p.eps2) ? dr2 : dr2 + p.reg2;
        double y = rsq_x2(denom2);
        if (MASKED) {
            y = (dr2 == 0.0) ? 0.0 : y; /* kernels.cpp:105-106 skip */
        } else {
            const unsigned hi = (unsigned)__double2hiint(dr2);
            zmin = hi < zmin ? hi : zmin;
        }
        const double y3 = y * (y * y);
        double ddotrho = dx * g[0];
        ddotrho = __builtin_fma(dy, g[1], ddotrho);
        ddotrho = __builtin_fma(dz, g[2], ddotrho);
        const double c = y3 * ddotrho;
        acc[0] = __builtin_fma(y, rho[0], acc[0]);
        acc[1] = __builtin_fma(y, rho[1], acc[1]);
        acc[2] = __builtin_fma(y, rho[2], acc[2]);
        acc[0] = __builtin_fma(dx, c, acc[0]);
        acc[1] = __builtin_fma(dy, c, acc[1]);
        acc[2] = __builtin_fma(dz, c, acc[2]);
    }
    __device__ static inline double finish(double a, const Params &p) { return a * p.scale; }
};

struct Rotlet : VelocityTraits {
    static constexpr int MIN_WAVES = 3;
    static constexpr int SRCDIM = 3;
    static constexpr int AUXDIM = 0;
    static constexpr bool HAS_MASK = false;
    static constexpr bool NAN_PROBE = false;
    static constexpr double ACC_FOLD = 8.0; /* y^3 = 8*fr */
    struct Params {
        double scale; /* factor = 1/(8*pi*eta) / ACC_FOLD, applied at the end
                         as the reference does (kernels.cpp:239) */
        double reg2;
        double eps2;
    };
    static Params make_params(double scale, double reg, double eps) {
        return {scale, reg * reg, eps * eps};
    }
    /* kernels.cpp:218-236: dr = dr2 < eps^2 ? sqrt(reg2+dr2) : sqrt(dr2)
     * (no dr==0 skip); fr = 1/dr^3; u += fr * (d x' rho) with the reference's
     * sign convention u_x += fr*(dz*rho_y - dy*rho_z), d = trg - src. */
    template <bool MASKED>
    __device__ static inline void pair(const double t[3], const double sp[3], const double rho[3],
                                       const double *, double acc[3], const Params &p,
                                       unsigned &) {
        const double dx = t[0] - sp[0];
        const double dy = t[1] - sp[1];
        const double dz = t[2] - sp[2];
        double dr2 = dx * dx;
        dr2 = __builtin_fma(dy, dy, dr2);
        dr2 = __builtin_fma(dz, dz, dr2);
        const double denom2 = (dr2 < p.eps2) ? dr2 + p.reg2 : dr2;
        const double y = rsq_x2(denom2);
        const double fr = y * (y * y);
        const double cx = __builtin_fma(dz, rho[1], -(dy * rho[2]));
        const double cy = __builtin_fma(dx, rho[2], -(dz * rho[0]));
        const double cz = __builtin_fma(dy, rho[0], -(dx * rho[1]));
        acc[0] = __builtin_fma(fr, cx, acc[0]);
        acc[1] = __builtin_fma(fr, cy, acc[1]);
        acc[2] = __builtin_fma(fr, cz, acc[2]);
    }
    __device__ static inline double finish(double a, const Params &p) { return a * p.scale; }
};

struct StressletNormalDensity : VelocityTraits {
    static constexpr int MIN_WAVES = 3;
    static constexpr int SRCDIM = 6; /* normal[3] + density[3] per source */
    static constexpr int AUXDIM = 0;
    static constexpr bool HAS_MASK = true;
    /* Unmasked, d == 0 gives f0 = (+-0)*(+-0)*rinv5: the same signed zero as
     * the masked rinv5 = +0 while the regularized rinv5 is finite, and NaN
     * (0*inf, or the rsq(0) seed when reg == 0) otherwise. */
    static constexpr bool NAN_PROBE = true;
    static constexpr double ACC_FOLD = 32.0; /* y^5 = 32/r^5 */
    struct Params {
        double scale; /* -3/(4*pi) / ACC_FOLD, kernels.cpp:311 (no eta dependence) */
        double reg2;
        double eps2;
    };
    /* the prefactor is the kernel's own: the caller's scale is not read */
    static Params make_params(double, double reg, double eps) {
        return {-3.0 / (4.0 * M_PI), reg * reg, eps * eps};
    }
    /* kernels::stresslet_times_normal_times_density (kernels.cpp:307-334):
     * Sdn_i += (d.rho_j)(d.n_j)/r^5 d, d = trg - src; r_norm < eps ->
     * sqrt(r^2+reg^2) (kernels.cpp:320-323). The reference's i==j skip is a
     * d==0 mask here (identical: the numerator is ~d^3). */
    template <bool MASKED>
    __device__ static inline void pair(const double t[3], const double sp[3], const double f[6],
                                       const double *, double acc[3], const Params &p,
                                       unsigned &) {
        const double dx = t[0] - sp[0];
        const double dy = t[1] - sp[1];
        const double dz = t[2] - sp[2];
        double dr2 = dx * dx;
        dr2 = __builtin_fma(dy, dy, dr2);
        dr2 = __builtin_fma(dz, dz, dr2);
        const double denom2 = (dr2 < p.eps2) ? dr2 + p.reg2 : dr2;
        double y = rsq_x2(denom2);
        if (MASKED)
            y = (dr2 == 0.0) ? 0.0 : y;
        const double y2 = y * y;
        const double rinv5 = y * y2 * y2;
        double ddn = dx * f[0];
        ddn = __builtin_fma(dy, f[1], ddn);
        ddn = __builtin_fma(dz, f[2], ddn);
        double ddrho = dx * f[3];
        ddrho = __builtin_fma(dy, f[4], ddrho);
        ddrho = __builtin_fma(dz, f[5], ddrho);
        const double f0 = ddrho * ddn * rinv5;
        acc[0] = __builtin_fma(f0, dx, acc[0]);
        acc[1] = __builtin_fma(f0, dy, acc[1]);
        acc[2] = __builtin_fma(f0, dz, acc[2]);
    }
    __device__ static inline double finish(double a, const Params &p) { return a * p.scale; }
};

/* ---- velocity-gradient functors ----------------------------------------
 * G[i][j] = d u_i / d x_j at the target, 9 accumulators per target stored
 * row-major (acc[3*i + j]); d = t - s, y = 1/sqrt(den), R = 2y from rsq_x2.
 * Each formula is the exact derivative of the matching velocity kernel inside
 * each of its branches (the regularized branches differentiate the
 * regularized expression). Nine accumulators a target leave room for fewer
 * targets per thread than the velocity kernels (MAX_TPT; numbers in
 * DESIGN.md), and every pair goes through the
 * r == 0 mask (FASTPATH off), so the result cannot depend on
 * skelly_set_pair_fastpath. */

#ifndef SKELLY_GRAD_TPT
#define SKELLY_GRAD_TPT 2
#endif
#ifndef SKELLY_DLGRAD_TPT
#define SKELLY_DLGRAD_TPT 2
#endif

struct GradTraits {
    static constexpr int OUTDIM = 9;
    static constexpr int GROUP = SKELLY_GROUP;
    static constexpr int AUXDIM = 0;
    static constexpr bool FASTPATH = false;
    static constexpr bool NAN_PROBE = false;
};

/* Stokeslet and regularized Oseen in one functor: Params{., 0, 0} is the
 * plain Stokeslet (den = r^2), else den follows OseenContract::pair.
 *   u_i  = y f_i + y^3 (f.d) d_i
 *   G_ij = y^3 (d_i f_j - f_i d_j + (f.d) delta_ij) - 3 y^5 (f.d) d_i d_j
 * With R^3 = 8 y^3 and -3 y^2 = -0.75 R^2 every term is 8x the plain one. */
struct StokesletGrad : GradTraits {
    static constexpr int MIN_WAVES = 3;
    static constexpr int MAX_TPT = SKELLY_GRAD_TPT;
    static constexpr int SRCDIM = 3;
    static constexpr bool HAS_MASK = true;
    static constexpr double ACC_FOLD = 8.0;
    struct Params {
        double scale; /* 1/(8*pi*eta) / ACC_FOLD */
        double reg2;
        double eps2;
    };
    static Params make_params(double scale, double reg, double eps) {
        return {scale, reg * reg, eps * eps};
    }
    template <bool MASKED>
    __device__ static inline void pair(const double t[3], const double sp[3], const double f[3],
                                       const double *, double acc[9], const Params &p,
                                       unsigned &) {
        const double dx = t[0] - sp[0];
        const double dy = t[1] - sp[1];
        const double dz = t[2] - sp[2];
        double r2 = dx * dx;
        r2 = __builtin_fma(dy, dy, r2);
        r2 = __builtin_fma(dz, dz, r2);
        const double den = (r2 > p.eps2) ? r2 : r2 + p.reg2;
        double R = rsq_x2(den);
        if (MASKED)
            R = (r2 == 0.0) ? 0.0 : R;
        const double R2 = R * R;
        const double R3 = R2 * R;
        double fd = f[0] * dx;
        fd = __builtin_fma(f[1], dy, fd);
        fd = __builtin_fma(f[2], dz, fd);
        const double A = fd * R3;            /* 8 y^3 (f.d) */
        const double B = A * (-0.75 * R2);   /* -8 * 3 y^5 (f.d) */
        const double Bdx = B * dx, Bdy = B * dy, Bdz = B * dz;
        const double Rfx = R3 * f[0], Rfy = R3 * f[1], Rfz = R3 * f[2];
        const double vx = Bdx + Rfx, vy = Bdy + Rfy, vz = Bdz + Rfz;
        /* diagonal: the antisymmetric part cancels exactly */
        acc[0] = __builtin_fma(Bdx, dx, acc[0]) + A;
        acc[4] = __builtin_fma(Bdy, dy, acc[4]) + A;
        acc[8] = __builtin_fma(Bdz, dz, acc[8]) + A;
        /* off-diagonal: d_i (B d_j + R3 f_j) - (R3 f_i) d_j */
        acc[1] = __builtin_fma(-Rfx, dy, __builtin_fma(dx, vy, acc[1]));
        acc[2] = __builtin_fma(-Rfx, dz, __builtin_fma(dx, vz, acc[2]));
        acc[3] = __builtin_fma(-Rfy, dx, __builtin_fma(dy, vx, acc[3]));
        acc[5] = __builtin_fma(-Rfy, dz, __builtin_fma(dy, vz, acc[5]));
        acc[6] = __builtin_fma(-Rfz, dx, __builtin_fma(dz, vx, acc[6]));
        acc[7] = __builtin_fma(-Rfz, dy, __builtin_fma(dz, vy, acc[7]));
    }
    __device__ static inline double finish(double a, const Params &p) { return a * p.scale; }
};

/* Stresslet: S_kl = f[3k+l], C = d_k S_kl d_l, b_j = (S_jl + S_lj) d_l.
 *   G_ij = -3 [ y^5 (d_i b_j + C delta_ij) - 5 y^7 C d_i d_j ]
 * The accumulators hold 32x the bracket (R^5 = 32 y^5, -5 y^2 = -1.25 R^2);
 * the -3 rides in Params::scale. b.d = 2C. */
struct StressletGrad : GradTraits {
    static constexpr int MIN_WAVES = 3;
    static constexpr int GROUP = 1; /* 24 SGPRs a source */
    static constexpr int MAX_TPT = SKELLY_DLGRAD_TPT;
    static constexpr int SRCDIM = 9;
    static constexpr bool HAS_MASK = true;
    static constexpr double ACC_FOLD = 32.0;
    struct Params {
        double scale; /* -3/(8*pi*eta) / ACC_FOLD */
    };
    static Params make_params(double scale, double, double) { return {-3.0 * scale}; }
    template <bool MASKED>
    __device__ static inline void pair(const double t[3], const double sp[3], const double f[9],
                                       const double *, double acc[9], const Params &,
                                       unsigned &) {
        const double dx = t[0] - sp[0];
        const double dy = t[1] - sp[1];
        const double dz = t[2] - sp[2];
        double r2 = dx * dx;
        r2 = __builtin_fma(dy, dy, r2);
        r2 = __builtin_fma(dz, dz, r2);
        double R = rsq_x2(r2);
        if (MASKED)
            R = (r2 == 0.0) ? 0.0 : R;
        const double R2 = R * R;
        const double R5 = R * R2 * R2;
        const double txy = f[1] + f[3], txz = f[2] + f[6], tyz = f[5] + f[7];
        const double px = f[0] * dx, py = f[4] * dy, pz = f[8] * dz;
        const double bx = __builtin_fma(txy, dy, __builtin_fma(txz, dz, px + px));
        const double by = __builtin_fma(txy, dx, __builtin_fma(tyz, dz, py + py));
        const double bz = __builtin_fma(txz, dx, __builtin_fma(tyz, dy, pz + pz));
        double c2 = bx * dx;
        c2 = __builtin_fma(by, dy, c2);
        c2 = __builtin_fma(bz, dz, c2);
        const double A = c2 * (0.5 * R5);    /* 32 y^5 C */
        const double Bq = A * (-1.25 * R2);  /* -32 * 5 y^7 C */
        const double vx = __builtin_fma(Bq, dx, R5 * bx);
        const double vy = __builtin_fma(Bq, dy, R5 * by);
        const double vz = __builtin_fma(Bq, dz, R5 * bz);
        acc[0] = __builtin_fma(dx, vx, acc[0]) + A;
        acc[1] = __builtin_fma(dx, vy, acc[1]);
        acc[2] = __builtin_fma(dx, vz, acc[2]);
        acc[3] = __builtin_fma(dy, vx, acc[3]);
        acc[4] = __builtin_fma(dy, vy, acc[4]) + A;
        acc[5] = __builtin_fma(dy, vz, acc[5]);
        acc[6] = __builtin_fma(dz, vx, acc[6]);
        acc[7] = __builtin_fma(dz, vy, acc[7]);
        acc[8] = __builtin_fma(dz, vz, acc[8]) + A;
    }
    __device__ static inline double finish(double a, const Params &p) { return a * p.scale; }
};

/* Rotlet: c = rho x d in Rotlet::pair's sign convention, den as there (no
 * zero mask).
 *   u_i  = y^3 c_i
 *   G_ij = y^3 eps_ikj rho_k - 3 y^5 c_i d_j          (accumulated 8x) */
struct RotletGrad : GradTraits {
    static constexpr int MIN_WAVES = 3;
    static constexpr int MAX_TPT = SKELLY_GRAD_TPT;
    static constexpr int SRCDIM = 3;
    static constexpr bool HAS_MASK = false;
    static constexpr double ACC_FOLD = 8.0;
    struct Params {
        double scale; /* 1/(8*pi*eta) / ACC_FOLD */
        double reg2;
        double eps2;
    };
    static Params make_params(double scale, double reg, double eps) {
        return {scale, reg * reg, eps * eps};
    }
    template <bool MASKED>
    __device__ static inline void pair(const double t[3], const double sp[3], const double rho[3],
                                       const double *, double acc[9], const Params &p,
                                       unsigned &) {
        const double dx = t[0] - sp[0];
        const double dy = t[1] - sp[1];
        const double dz = t[2] - sp[2];
        double r2 = dx * dx;
        r2 = __builtin_fma(dy, dy, r2);
        r2 = __builtin_fma(dz, dz, r2);
        const double den = (r2 < p.eps2) ? r2 + p.reg2 : r2;
        const double R = rsq_x2(den);
        const double R2 = R * R;
        const double R3 = R2 * R;
        const double q = (-0.75 * R2) * R3; /* -8 * 3 y^5 */
        const double cx = __builtin_fma(dz, rho[1], -(dy * rho[2]));
        const double cy = __builtin_fma(dx, rho[2], -(dz * rho[0]));
        const double cz = __builtin_fma(dy, rho[0], -(dx * rho[1]));
        const double qx = q * cx, qy = q * cy, qz = q * cz;
        const double wx = R3 * rho[0], wy = R3 * rho[1], wz = R3 * rho[2];
        acc[0] = __builtin_fma(qx, dx, acc[0]);
        acc[1] = __builtin_fma(qx, dy, acc[1]) - wz;
        acc[2] = __builtin_fma(qx, dz, acc[2]) + wy;
        acc[3] = __builtin_fma(qy, dx, acc[3]) + wz;
        acc[4] = __builtin_fma(qy, dy, acc[4]);
        acc[5] = __builtin_fma(qy, dz, acc[5]) - wx;
        acc[6] = __builtin_fma(qz, dx, acc[6]) - wy;
        acc[7] = __builtin_fma(qz, dy, acc[7]) + wx;
        acc[8] = __builtin_fma(qz, dz, acc[8]);
    }
    __device__ static inline double finish(double a, const Params &p) { return a * p.scale; }
};

/* ---- pressure functors --------------------------------------------------
 * The Stokes pressure p that goes with the velocity kernels above, one
 * accumulator per target (OUTDIM 1); d = t - s, y = 1/sqrt(den), R = 2y.
 * With sigma = -p I + eta (G + G^T) and the velocity's 1/(8 pi eta):
 *   Stokeslet / Oseen   p = 1/(4 pi) sum (f.d) y^3
 *   Stresslet           p = 1/(4 pi) sum [ tr(S) y^3 - 3 C y^5 ],  C = d^T S d
 *   Rotlet              p = 0 identically: there is no functor.
 * Neither depends on eta (a double layer's f_dl = 2 eta n (x) rho brings its
 * own). Every pair goes through the r == 0 mask (FASTPATH off, as for the
 * gradients), so the result cannot depend on skelly_set_pair_fastpath.
 *
 * MAX_TPT = 4, MIN_WAVES = 4. One accumulator a target needs 8 VGPRs a
 * target (6 of coordinates, 2 of sum) against the velocity functors' 12, and
 * the compiler's kernel-resource-usage reports 58 (StokesletPressure) and 66
 * (StressletPressure) VGPRs at 4 targets a thread, 28 and 38 at one, no
 * scratch: 8 targets would fit the register file. They are not taken: the
 * loop is bound by fp64 VALU issue, not by the scalar record loads that more
 * targets a thread would amortise (a source's 6 or 12 SGPR pairs already
 * serve 4 x 64 pairs), and the launch planner and dispatch_tpt are built and
 * fitted for 1, 2 and 4. The spare registers go to occupancy instead: a
 * launch bound of 4 waves a SIMD (a 128-VGPR budget, met twice over), one
 * more than the velocity functors, to cover the rsq latency of a loop with
 * this little independent arithmetic a pair. SGPRs: two groups in flight,
 * 2 x GROUP x 2 x (3 + SRCDIM) = 48 for both, 84-86 in all of the ~100. */

struct PressureTraits {
    static constexpr int OUTDIM = 1;
    static constexpr int MAX_TPT = 4;
    static constexpr int MIN_WAVES = 4;
    static constexpr int AUXDIM = 0;
    static constexpr bool HAS_MASK = true;
    static constexpr bool FASTPATH = false;
    static constexpr bool NAN_PROBE = false;
    static constexpr double ACC_FOLD = 8.0; /* R^3 = 8 y^3 */
};

/* Stokeslet and regularized Oseen in one functor, as StokesletGrad:
 * Params{., 0, 0} is the plain Stokeslet, else den follows OseenContract::pair
 * (the pressure of the regularized branch is defined by the same
 * substitution). acc += R^3 (f.d). */
struct StokesletPressure : PressureTraits {
    static constexpr int GROUP = SKELLY_GROUP;
    static constexpr int SRCDIM = 3;
    struct Params {
        double scale; /* 1/(4*pi) / ACC_FOLD */
        double reg2;
        double eps2;
    };
    static Params make_params(double scale, double reg, double eps) {
        return {scale, reg * reg, eps * eps};
    }
    template <bool MASKED>
    __device__ static inline void pair(const double t[3], const double sp[3], const double f[3],
                                       const double *, double acc[1], const Params &p,
                                       unsigned &) {
        const double dx = t[0] - sp[0];
        const double dy = t[1] - sp[1];
        const double dz = t[2] - sp[2];
        double r2 = dx * dx;
        r2 = __builtin_fma(dy, dy, r2);
        r2 = __builtin_fma(dz, dz, r2);
        const double den = (r2 > p.eps2) ? r2 : r2 + p.reg2;
        double R = rsq_x2(den);
        if (MASKED)
            R = (r2 == 0.0) ? 0.0 : R;
        const double R3 = (R * R) * R;
        double fd = f[0] * dx;
        fd = __builtin_fma(f[1], dy, fd);
        fd = __builtin_fma(f[2], dz, fd);
        acc[0] = __builtin_fma(fd, R3, acc[0]);
    }
    __device__ static inline double finish(double a, const Params &p) { return a * p.scale; }
};

/* acc += R^3 (tr(S) - 0.75 R^2 C) = 8 [ tr(S) y^3 - 3 C y^5 ]. */
struct StressletPressure : PressureTraits {
    static constexpr int GROUP = 1; /* 24 SGPRs a source */
    static constexpr int SRCDIM = 9;
    struct Params {
        double scale; /* 1/(4*pi) / ACC_FOLD */
    };
    static Params make_params(double scale, double, double) { return {scale}; }
    template <bool MASKED>
    __device__ static inline void pair(const double t[3], const double sp[3], const double f[9],
                                       const double *, double acc[1], const Params &,
                                       unsigned &) {
        const double dx = t[0] - sp[0];
        const double dy = t[1] - sp[1];
        const double dz = t[2] - sp[2];
        const double dxx = dx * dx, dyy = dy * dy, dzz = dz * dz;
        double dr2 = dxx + dyy;
        dr2 += dzz;
        double R = rsq_x2(dr2);
        if (MASKED)
            R = (dr2 == 0.0) ? 0.0 : R;
        const double R2 = R * R;
        const double R3 = R2 * R;
        /* C as Stresslet::pair's coeff */
        double C = f[0] * dxx;
        C = __builtin_fma(f[4], dyy, C);
        C = __builtin_fma(f[8], dzz, C);
        C = __builtin_fma(f[1] + f[3], dx * dy, C);
        C = __builtin_fma(f[2] + f[6], dx * dz, C);
        C = __builtin_fma(f[5] + f[7], dy * dz, C);
        const double tr = (f[0] + f[4]) + f[8];
        const double q = __builtin_fma(-0.75 * R2, C, tr);
        acc[0] = __builtin_fma(R3, q, acc[0]);
    }
    __device__ static inline double finish(double a, const Params &p) { return a * p.scale; }
};

/* ---- driver ----------------------------------------------------------- */

/* Doubles of one packed source record {r[3], f[SRCDIM], g[AUXDIM]}. */
template <typename K>
constexpr int rec_doubles() {
    return 3 + K::SRCDIM + K::AUXDIM;
}

/* Records the buffer holds for n_src sources: one group of padding, so that
 * the pair loop may load a whole group past the last source. */
template <typename K>
constexpr long long rec_count(long long n_src) {
    return n_src + K::GROUP;
}

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
                                           const int count, const double (&tp)[TPT][3],
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
                                          const double (&tp)[TPT][3],
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

    double tp[TPT][3];
    constexpr int OD = K::OUTDIM;
    double acc[TPT][OD];
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        long long it = base + (long long)k * BLOCK + tid;
        const long long itc = it < n_trg ? it : (n_trg > 0 ? n_trg - 1 : 0);
        tp[k][0] = r_trg[3 * itc + 0];
        tp[k][1] = r_trg[3 * itc + 1];
        tp[k][2] = r_trg[3 * itc + 2];
#pragma unroll
        for (int j = 0; j < OD; ++j)
            acc[k][j] = 0.0;
    }

    /* An empty use of the target coordinates: the wait for their loads falls
     * here, once, instead of in the pair loop as one counted wait a target. */
#pragma unroll
    for (int k = 0; k < TPT; ++k)
        asm volatile("" : "+v"(tp[k][0]), "+v"(tp[k][1]), "+v"(tp[k][2]));

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
 * partial layout: [n_slices][n_trg][OUTDIM]; one thread per (target, component). */
template <typename K>
__global__ __launch_bounds__(BLOCK) void reduce_partials(const double *__restrict__ partial,
                                                         double *__restrict__ u_trg,
                                                         long long n_trg, int n_slices,
                                                         typename K::Params params) {
    const long long n_out = K::OUTDIM * n_trg;
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_out)
        return;
    double s = 0.0;
    for (int y = 0; y < n_slices; ++y)
        s += partial[(long long)y * n_out + i];
    u_trg[i] = K::finish(s, params);
}

/* ---- launch helpers (host) -------------------------------------------- */

namespace skelly {

namespace {
/* A launch knob: the value a skelly_set_*() call forced (>= 0), else the
 * environment variable, read once and passed through `clamp` (`dflt` without
 * the variable). */
struct Knob {
    const char *env;
    int dflt;
    int (*clamp)(int);
    int forced = -1; /* -1 = follow env var */
    std::once_flag once;
    int from_env = 0;

    int get() {
        if (forced >= 0)
            return forced;
        std::call_once(once, [this] {
            const char *e = getenv(env);
            from_env = clamp(e ? atoi(e) : dflt);
        });
        return from_env;
    }
};
} // namespace

/* The launch workspace (the source records of every launch and the partials
 * of the split ones). SKELLY_PERSISTENT_WS / skelly_set_persistent_ws():
 *   1 (default)  a grow-only hipMalloc block cached per (device, stream).
 *      Reuse across launches is safe because launches on one stream are
 *      ordered; an outgrown block is RETIRED, not freed or reused, for as
 *      long as its stream lives (queued work and captured graphs may still
 *      reference it; geometric growth bounds what is held at ~2x the final
 *      size). Nothing is allocated by a launch that fits, so such launches
 *      can be captured into a graph.
 *   0  a hipMallocAsync/hipFreeAsync pair per launch on the stream-ordered
 *      mempool. This was the default until it was found to give wrong
 *      results; see WORKSPACE_DEFECT below. Kept as a switch for comparison
 *      only. A launch also falls back to it if hipMalloc fails.
 *
 * WORKSPACE_DEFECT (open; DESIGN.md, "Launch workspace"): with the mempool
 * workspace, a fresh process that made ten synchronised calls of different
 * kernels back to back, host forms or device forms, got a wrong result in
 * 15 of 48 runs on MI355X (every target off by about one far source's worth:
 * some of the records the pair kernel read were not the ones pack_sources
 * had just written). It takes the pool handing its memory back at
 * hipStreamSynchronize (release threshold 0) and the next launch mapping
 * memory anew: with the threshold at its maximum, or with the persistent
 * block, none in 24 and none in 48. */
static Knob g_persistent_ws{"SKELLY_PERSISTENT_WS", 1, [](int v) { return v != 0 ? 1 : 0; }};

namespace {
struct WsEntry {
    void *ptr = nullptr;
    size_t cap = 0;
    std::vector<void *> retired;
};
struct WsCache {
    std::mutex mu;
    std::map<std::pair<int, hipStream_t>, WsEntry> blocks; /* (device, stream) */
};
WsCache &ws_cache() {
    static WsCache c;
    return c;
}
int current_device() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return dev;
}
} // namespace

static double *persistent_ws(hipStream_t stream, size_t bytes) {
    WsCache &c = ws_cache();
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(c.mu);
    WsEntry &e = c.blocks[{dev, stream}];
    if (e.cap < bytes) {
        size_t want = bytes * 2;
        void *p = nullptr;
        if (hipMalloc(&p, want) != hipSuccess)
            return nullptr; /* caller falls back to the async path */
        if (e.ptr)
            e.retired.push_back(e.ptr);
        e.ptr = p;
        e.cap = want;
    }
    return static_cast<double *>(e.ptr);
}

long long persistent_ws_bytes(hipStream_t stream) {
    WsCache &c = ws_cache();
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(c.mu);
    auto it = c.blocks.find({dev, stream});
    return it == c.blocks.end() ? 0 : (long long)it->second.cap;
}

void release_persistent_ws(hipStream_t stream) {
    WsCache &c = ws_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    for (auto it = c.blocks.begin(); it != c.blocks.end();) {
        if (it->first.second != stream) {
            ++it;
            continue;
        }
        (void)hipFree(it->second.ptr);
        for (void *p : it->second.retired)
            (void)hipFree(p);
        it = c.blocks.erase(it);
    }
}

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

template <typename K>
static hipError_t launch_pair(const double *r_src, const double *f_src, const double *r_trg,
                              double *u_trg, long long n_src, long long n_trg,
                              typename K::Params params, hipStream_t stream) {
    if (n_trg <= 0)
        return hipSuccess;
    /* the kernels accumulate ACC_FOLD x the sum (power of two: exact) */
    params.scale /= K::ACC_FOLD;
    const int tpt = pick_tpt<K>(n_trg);
    const long long blocks = (n_trg + (long long)BLOCK * tpt - 1) / ((long long)BLOCK * tpt);

    /* Source slices from the CU load-balance model (pair_plan.hpp): the
     * slice count that leaves the CUs the least uneven numbers of
     * workgroups, within the slice-length floor and the workspace cap. */
    /* wg_per_cu: the functor's launch bound, as the planner's constants were
     * fitted with. Without LDS the occupancy query answers more, and the
     * plans (with them the summation order) are not to move with it. */
    const PairPlan plan =
        pair_plan(n_src, n_trg, K::MAX_TPT, K::OUTDIM, g_pair_fastpath.get(),
                  PAIR_FASTPATH_MIN_SRC, pair_device_cus(), K::MIN_WAVES, g_pair_slices.get());
    const int n_slices = plan.n_slices;
    const int fast = plan.fast;

    /* Workspace: the packed source records, then (split launches) the
     * partials of every slice. */
    const size_t rec_doubles_total = (size_t)rec_doubles<K>() * rec_count<K>(n_src);
    const size_t partial_doubles = n_slices > 1 ? (size_t)n_slices * K::OUTDIM * n_trg : 0;
    const size_t ws_bytes = (rec_doubles_total + partial_doubles) * sizeof(double);
    double *workspace = nullptr;
    bool pooled = false;
    if (g_persistent_ws.get() != 0) {
        workspace = persistent_ws(stream, ws_bytes);
        pooled = workspace != nullptr;
    }
    if (!pooled) {
        hipError_t err = hipMallocAsync((void **)&workspace, ws_bytes, stream);
        if (err != hipSuccess)
            return err;
    }
    double *rec = workspace;
    double *partials = workspace + rec_doubles_total;

    const long long slice_len = (n_src + n_slices - 1) / n_slices;
    dim3 block(BLOCK);
    const long long pblocks = ((long long)rec_doubles_total + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL((pack_sources<K>), dim3((unsigned)pblocks), block, 0, stream, r_src, f_src,
                       rec, n_src);
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
        const long long rblocks = (K::OUTDIM * n_trg + BLOCK - 1) / BLOCK;
        hipLaunchKernelGGL((reduce_partials<K>), dim3((unsigned)rblocks), block, 0, stream,
                           partials, u_trg, n_trg, n_slices, params);
    }
    hipError_t err = hipGetLastError();
    if (pooled)
        return err;
    hipError_t err2 = hipFreeAsync(workspace, stream);
    return err != hipSuccess ? err : err2;
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
                              K::make_params(scale, reg, eps), stream);
    });
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

/* ---- issue-cost probe (what the pair loop's non-FMA instructions cost) ---
 * The body of fp64_fma_peak_kernel four times over (64 independent
 * v_fma_f64 on 16 accumulators) with 4 instructions of one kind put in front,
 * about the pair loop's mix (16 v_rsq_f64 and 18 ds_read_b128 to 320 fp64
 * ops):
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

/* The streamline tracer: a kernel of its own over the functors, pack_sources
 * and the workspace above. */
#include "streamline_kernel.hpp"

/* Runtime override of the persistent split-K workspace (see
 * g_persistent_ws above): hipGraph capture of the GMRES iteration
 * (gmres.py use_graph) requires it — hipMallocAsync nodes cannot be
 * recorded reliably, and the grow-only hipMalloc happens during the
 * UNCAPTURED warmup pass, so capture itself allocates nothing. */
extern "C" void skelly_set_persistent_ws(int on) {
    skelly::g_persistent_ws.forced = on;
}

extern "C" int skelly_persistent_ws_bytes(void *stream, long long *out_bytes) {
    *out_bytes = skelly::persistent_ws_bytes((hipStream_t)stream);
    return 0;
}

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
