/* pair_functors.hpp — the per-pair arithmetic of every kernel unit: the fp64
 * rsqrt, the eleven pair functors (ten sums and one arg-min) and the layout of a packed source record.
 * Device code, but for launch_params() at the end. pair_kernels.hip
 * (pair_driver, the dense builders), trace_kernels.hip (the field-line tracer)
 * and probe_kernels.hip (the rsq probe) include it, so that all three run the
 * same pair<MASKED>() and the same rsq_x2(). The design of the pair loop that
 * these functors were written for is recorded at the head of pair_kernels.hip. */

#ifndef SKELLY_PAIR_FUNCTORS_HPP
#define SKELLY_PAIR_FUNCTORS_HPP

#include <hip/hip_runtime.h>

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

/* 1/sqrt(x) for the dense builders of pair_kernels.hip (setup-time, not hot). */
__device__ inline double rsq_refined(double x) { return 0.5 * rsq_x2(x); }

/* ---- kernel functors -------------------------------------------------
 * pair<MASKED>() adds one source's contribution to one target's
 * accumulators. With R = 2/r the accumulators hold ACC_FOLD times the plain
 * sum; launch_params() divides Params::scale by ACC_FOLD. make_params()
 * (host) builds Params from the C entry point's (scale, reg, eps); finish()
 * turns an accumulator into the output.
 *   HAS_MASK  the kernel zeroes coincident pairs; MASKED=false leaves the
 *              select out and must make a coincident pair detectable.
 *   NAN_PROBE  an unmasked coincident pair turns the accumulators NaN
 *              (else pair<false> lowers `zmin` to 0 on one).
 *   AUXDIM     doubles per source of the record's second copy g = f/4 (0: none).
 *   OUTDIM     accumulators and outputs per target (3 velocity components,
 *              9 for the gradient functors further down).
 *   MAX_TPT    most targets a thread holds (register budget).
 *   GROUP      sources per group of scalar record loads (SGPR budget: two
 *              groups of GROUP x 2 x (3 + SRCDIM + AUXDIM) SGPRs are live).
 *   FASTPATH   the unmasked chunk-rerun path is wired (needs HAS_MASK).
 *   TRGDIM     doubles per target: the coordinates, then what the functor
 *              reads beside them (Nearest: the target's group id).
 *   init(j)    what accumulator j starts from: the neutral element of the
 *              functor's reduction, which an empty slice writes.
 *   JOINT      a target's OUTDIM partials of two slices combine as one value
 *              (combine(), in slice order) instead of component by component. */

/* What every functor has unless it says otherwise: a sum from zero over
 * three target coordinates, finished with the prefactor, applied once (linear
 * in the sum). P is the functor's Params. */
struct PairFunctor {
    static constexpr int TRGDIM = 3;
    static constexpr bool JOINT = false;
    __device__ static inline double init(int) { return 0.0; }
    template <typename P>
    __device__ static inline double finish(double a, const P &p) {
        return a * p.scale;
    }
};

/* The two shapes of Params. scale is the kernel's prefactor / ACC_FOLD, with
 * or without eta as the entry point computed it; reg2 and eps2 are read by the
 * regularized functors only. */
struct ScaleParams {
    struct Params {
        double scale;
    };
    static Params make_params(double scale, double, double) { return {scale}; }
};

struct RegParams {
    struct Params {
        double scale;
        double reg2;
        double eps2;
    };
    static Params make_params(double scale, double reg, double eps) {
        return {scale, reg * reg, eps * eps};
    }
};

struct VelocityTraits : PairFunctor {
    static constexpr int OUTDIM = 3;
    static constexpr int MAX_TPT = 4;
    static constexpr int GROUP = SKELLY_GROUP;
    static constexpr bool FASTPATH = true;
};

/* scale: 1/(8*pi) [ / eta when folded] */
struct Stokeslet : VelocityTraits, ScaleParams {
    static constexpr int MIN_WAVES = 3;
    static constexpr int SRCDIM = 3;
    static constexpr int AUXDIM = 3;
    static constexpr bool HAS_MASK = true;
    static constexpr bool NAN_PROBE = true;
    static constexpr double ACC_FOLD = 2.0;
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
};

/* scale: 1/(8*pi) [ / eta when folded] */
struct Stresslet : VelocityTraits, ScaleParams {
    static constexpr int MIN_WAVES = 2;
    static constexpr int GROUP = 1; /* 24 SGPRs a source */
    static constexpr int SRCDIM = 9;
    static constexpr int AUXDIM = 0;
    static constexpr bool HAS_MASK = true;
    static constexpr bool NAN_PROBE = true;
    static constexpr double ACC_FOLD = 32.0; /* R^5 = 32/r^5 */
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
};

/* scale: factor = 1/(8*pi*eta), hoisted out of the pair loop */
struct OseenContract : VelocityTraits, RegParams {
    static constexpr int MIN_WAVES = 3;
    static constexpr int SRCDIM = 3;
    static constexpr int AUXDIM = 3;
    static constexpr bool HAS_MASK = true;
    static constexpr bool NAN_PROBE = false; /* r = 0 regularizes to a finite 1/reg */
    static constexpr double ACC_FOLD = 2.0;
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
};

/* scale: factor = 1/(8*pi*eta), applied at the end as the reference does
 * (kernels.cpp:239) */
struct Rotlet : VelocityTraits, RegParams {
    static constexpr int MIN_WAVES = 3;
    static constexpr int SRCDIM = 3;
    static constexpr int AUXDIM = 0;
    static constexpr bool HAS_MASK = false;
    static constexpr bool NAN_PROBE = false;
    static constexpr double ACC_FOLD = 8.0; /* y^3 = 8*fr */
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
};

struct StressletNormalDensity : VelocityTraits, RegParams {
    static constexpr int MIN_WAVES = 3;
    static constexpr int SRCDIM = 6; /* normal[3] + density[3] per source */
    static constexpr int AUXDIM = 0;
    static constexpr bool HAS_MASK = true;
    /* Unmasked, d == 0 gives f0 = (+-0)*(+-0)*rinv5: the same signed zero as
     * the masked rinv5 = +0 while the regularized rinv5 is finite, and NaN
     * (0*inf, or the rsq(0) seed when reg == 0) otherwise. */
    static constexpr bool NAN_PROBE = true;
    static constexpr double ACC_FOLD = 32.0; /* y^5 = 32/r^5 */
    /* the prefactor is the kernel's own, -3/(4*pi), kernels.cpp:311 (no eta
     * dependence): the caller's scale is not read */
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

struct GradTraits : PairFunctor {
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
struct StokesletGrad : GradTraits, RegParams { /* scale: 1/(8*pi*eta) */
    static constexpr int MIN_WAVES = 3;
    static constexpr int MAX_TPT = SKELLY_GRAD_TPT;
    static constexpr int SRCDIM = 3;
    static constexpr bool HAS_MASK = true;
    static constexpr double ACC_FOLD = 8.0;
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
};

/* Stresslet: S_kl = f[3k+l], C = d_k S_kl d_l, b_j = (S_jl + S_lj) d_l.
 *   G_ij = -3 [ y^5 (d_i b_j + C delta_ij) - 5 y^7 C d_i d_j ]
 * The accumulators hold 32x the bracket (R^5 = 32 y^5, -5 y^2 = -1.25 R^2);
 * the -3 rides in Params::scale. b.d = 2C. */
struct StressletGrad : GradTraits, ScaleParams {
    static constexpr int MIN_WAVES = 3;
    static constexpr int GROUP = 1; /* 24 SGPRs a source */
    static constexpr int MAX_TPT = SKELLY_DLGRAD_TPT;
    static constexpr int SRCDIM = 9;
    static constexpr bool HAS_MASK = true;
    static constexpr double ACC_FOLD = 32.0;
    /* scale: -3/(8*pi*eta) */
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
};

/* Rotlet: c = rho x d in Rotlet::pair's sign convention, den as there (no
 * zero mask).
 *   u_i  = y^3 c_i
 *   G_ij = y^3 eps_ikj rho_k - 3 y^5 c_i d_j          (accumulated 8x) */
struct RotletGrad : GradTraits, RegParams { /* scale: 1/(8*pi*eta) */
    static constexpr int MIN_WAVES = 3;
    static constexpr int MAX_TPT = SKELLY_GRAD_TPT;
    static constexpr int SRCDIM = 3;
    static constexpr bool HAS_MASK = false;
    static constexpr double ACC_FOLD = 8.0;
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

struct PressureTraits : PairFunctor {
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
struct StokesletPressure : PressureTraits, RegParams { /* scale: 1/(4*pi) */
    static constexpr int GROUP = SKELLY_GROUP;
    static constexpr int SRCDIM = 3;
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
};

/* acc += R^3 (tr(S) - 0.75 R^2 C) = 8 [ tr(S) y^3 - 3 C y^5 ]. */
struct StressletPressure : PressureTraits, ScaleParams { /* scale: 1/(4*pi) */
    static constexpr int GROUP = 1; /* 24 SGPRs a source */
    static constexpr int SRCDIM = 9;
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
};

/* ---- nearest source ------------------------------------------------------
 * Not a sum but an arg-min: per target the smallest d^2 = |t - s|^2 over the
 * eligible sources and the index of the source that attains it, in
 * acc = {d^2, index}. The record is {r[3], index, group} and the target
 * carries its group id as a fourth double (ids and indices as exact doubles);
 * a source is eligible when its group differs from the target's. Ungrouped
 * calls give every source group 0 and every target group -1.
 *   - The update is one compare on d^2, one on the group, and selects: no
 *     rsqrt, no branch. A strict `<` in source order keeps the lowest index
 *     among equal d^2; combine() does the same across slices in slice order,
 *     so the result is the same for every slice count and target-per-thread
 *     count, bit for bit.
 *   - acc starts from {+inf, -1}: that is the answer for no eligible source,
 *     and for a NaN target or source, whose compare is false.
 *   - Every pair takes the same path (HAS_MASK and FASTPATH off): a
 *     coincident eligible pair is a hit with d^2 = 0.
 * GROUP: a record is 5 doubles = 10 SGPRs, two groups in flight. 4 sources a
 * group (80 SGPRs of records) leaves too few for addresses and counters;
 * 2 (40) compiles without spills. MAX_TPT 4, MIN_WAVES 4 as the pressures:
 * 12 VGPRs a target. */
#ifndef SKELLY_NEAREST_GROUP
#define SKELLY_NEAREST_GROUP 2
#endif

struct Nearest : PairFunctor, ScaleParams {
    static constexpr int OUTDIM = 2;
    static constexpr int MAX_TPT = 4;
    static constexpr int MIN_WAVES = 4;
    static constexpr int GROUP = SKELLY_NEAREST_GROUP;
    static constexpr int SRCDIM = 2; /* index, group */
    static constexpr int AUXDIM = 0;
    static constexpr int TRGDIM = 4; /* r[3], group */
    static constexpr bool HAS_MASK = false;
    static constexpr bool FASTPATH = false;
    static constexpr bool NAN_PROBE = false;
    static constexpr bool JOINT = true;
    static constexpr double ACC_FOLD = 1.0;
    __device__ static inline double init(int j) { return j == 0 ? __builtin_inf() : -1.0; }
    __device__ static inline double finish(double a, const Params &) { return a; }
    template <bool MASKED>
    __device__ static inline void pair(const double t[4], const double sp[3], const double f[2],
                                       const double *, double acc[2], const Params &,
                                       unsigned &) {
        const double dx = t[0] - sp[0];
        const double dy = t[1] - sp[1];
        const double dz = t[2] - sp[2];
        double d2 = dx * dx;
        d2 = __builtin_fma(dy, dy, d2);
        d2 = __builtin_fma(dz, dz, d2);
        const bool better = (d2 < acc[0]) & (f[1] != t[3]);
        acc[0] = better ? d2 : acc[0];
        acc[1] = better ? f[0] : acc[1];
    }
    /* a <- the better of a and the later slice's b */
    __device__ static inline void combine(double a[2], const double b[2]) {
        const bool better = b[0] < a[0];
        a[0] = better ? b[0] : a[0];
        a[1] = better ? b[1] : a[1];
    }
};

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

/* The Params of a launch (host): K's own from the entry point's (scale, reg,
 * eps), the prefactor divided by the ACC_FOLD that the accumulators carry (a
 * power of two: exact). The one place where the fold is divided out. */
template <typename K>
inline typename K::Params launch_params(double scale, double reg, double eps) {
    typename K::Params p = K::make_params(scale, reg, eps);
    p.scale /= K::ACC_FOLD;
    return p;
}

#endif /* SKELLY_PAIR_FUNCTORS_HPP */
