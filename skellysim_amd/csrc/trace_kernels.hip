/* trace_kernels.hip — the field-line tracer: one persistent workgroup per
 * job integrates dx/dt = u(x) (streamlines) or dx/dt = curl u(x) (vortex
 * lines) with adaptive Cash-Karp 5(4), every field evaluation, step decision
 * and record inside the one launch.
 *
 * A translation unit of its own over pair_functors.hpp: the field is summed
 * with the functors' own K::pair<true> / K::finish, with the Params that
 * launch_params<K> gives a pair launch, over records that pack_sources<K>
 * wrote (launch_pack_sources of pair_kernels.hip, so that kernel exists once),
 * so the per-pair arithmetic is the tested one. The workspace is the pair
 * launches' (launch_workspace.hpp).
 *
 * A job is one seed in one direction (a seed traced both ways is two jobs);
 * jobs share nothing but the read-only records, so there is no grid-wide seam
 * and a job's result does not depend on which other jobs are in the launch.
 *
 * Field (what listener.velocity_field sums): up to four source sets, each
 * possibly empty,
 *   Stokeslet      fibers and body centres,
 *   Stresslet      shell and body double layers (9 components),
 *   Rotlet         body and point torques,
 *   OseenContract  point forces,
 * plus the affine background uniform_j + x[components_j] * scale_j; a point
 * inside a body (|x - c_b| < radius_b) moves rigidly, U_b + w_b x (x - c_b),
 * later bodies overwriting earlier ones.
 *
 * Vorticity (TRACE_VORTICITY, the field of a vortex line): the curl of the
 * same field. Each set goes through its gradient functor (StokesletGrad for
 * the Stokeslets and, with reg and eps, for the regularized point forces;
 * StressletGrad; RotletGrad), and each thread takes the curl
 * (G21 - G12, G02 - G20, G10 - G01) of its own finished partial gradient, so
 * that three values go through the reduction below, not nine, and the three
 * diagonal accumulators are dead. The gradient functors read {r, f}, the
 * prefix of the velocity functors' records, so the pass walks the records
 * that the velocity pass reads, at the velocity functor's stride: nothing is
 * packed twice. The background adds its constant curl (TraceField::bg_curl,
 * from the host), and a point inside a body has 2 w_b.
 *
 * Evaluation: thread i takes records i, i + B, i + 2B, ... of every set with
 * vector loads (the targets differ per workgroup and the sources per lane,
 * the reverse of pair_driver, so its scalar record loads do not apply), sums
 * the finished contributions of the four sets into 3 partials, and the
 * workgroup reduces them: an xor butterfly inside each wave (every lane ends
 * with the same bits: each level adds the same two values in both lanes of a
 * pair, and a + b == b + a), lane 0 of each wave to LDS, one barrier, and every
 * thread adds the waves' sums in wave order. All threads then hold the same
 * u(x) bit for bit: that is the broadcast. The LDS slots alternate between
 * two buffers so that one barrier an evaluation is enough: a thread can only
 * write buffer p again two evaluations on, behind a barrier that every reader
 * of p has passed.
 *
 * Every thread carries the whole integrator state (x, t, dt, the stages) and
 * takes every decision (accept, reject, stop) from the reduced values, never
 * from its partials, so the barriers sit in uniform control flow; the flags
 * go through readfirstlane so that the compiler branches on scalars too.
 * Thread 0 writes the records.
 *
 * Stepper: Cash-Karp 5(4) with the control law of Boost.Odeint's
 * controlled_runge_kutta / default_error_checker(abs, rel, 1, 1) under
 * integrate_adaptive, as DESIGN.md ("Streamlines on the device") states it.
 * A vortex line takes its stages and its recorded val from the vorticity and
 * its singularity stop from the velocity, as the reference's observer does:
 * one more evaluation, of u, at every recorded point but the last.
 * Status: 0 t_final reached, 1 |u| > 1e3 at a recorded point (the point stays
 * recorded), 2 the output buffer is full (count == max_points), 3 the step
 * control gave up (1000 rejections of one step, a step that does not move t,
 * or more than 4 * max_points + 1000 tries in all). count stays at the -1 the
 * host wrote for a job that never ran. */

#include <hip/hip_runtime.h>

#include <cmath>

#include "launch_workspace.hpp"
#include "pair_functors.hpp"
#include "pair_kernels.hpp"

#ifndef SKELLY_TRACE_BLOCK
#define SKELLY_TRACE_BLOCK 256 /* profiles/streamlines.md */
#endif

static_assert(SKELLY_TRACE_BLOCK % 64 == 0 && SKELLY_TRACE_BLOCK >= 64 &&
                  SKELLY_TRACE_BLOCK <= 1024,
              "whole waves, at most one workgroup's worth");

/* Doubles of one body row: centre[3], radius, velocity[3], angular velocity[3]. */
#define SKELLY_TRACE_BODY_DOUBLES 10

/* The integrated field of a tracer instantiation. */
enum TraceKind { TRACE_VELOCITY = 0, TRACE_VORTICITY = 1 };

struct TraceField {
    const double *rec[4]; /* packed records: Stokeslet, Stresslet, Rotlet, OseenContract */
    long long n[4];
    Stokeslet::Params sl;
    Stresslet::Params dl;
    Rotlet::Params rot;
    OseenContract::Params os;
    /* the gradient functors of the same four sets, for the vorticity */
    StokesletGrad::Params gsl, gos;
    StressletGrad::Params gdl;
    RotletGrad::Params grot;
    double uniform[3], bg_scale[3];
    int components[3];
    double bg_curl[3]; /* curl of the background, constant in x */
    const double *bodies; /* (n_bodies, SKELLY_TRACE_BODY_DOUBLES) */
    int n_bodies;
};

struct TraceJobs {
    const double *seeds; /* (n_seeds, 3) */
    long long n_seeds;   /* job j < n_seeds runs seed j forward, job n_seeds + j backward */
    double dt_init, t_final, abs_err, rel_err;
    int max_points;
    double *x, *t, *val; /* (n_jobs, max_points, 3), (n_jobs, max_points), as x */
    int *count, *status; /* (n_jobs) */
};

/* A set's finished (scaled) partial velocity, added to u. */
template <typename K>
__device__ __forceinline__ void trace_finish(const double (&acc)[3],
                                             const typename K::Params &params, double (&u)[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
        u[j] += K::finish(acc[j], params);
}

/* The curl of a set's finished partial gradient, added to w. */
template <typename K>
__device__ __forceinline__ void trace_finish(const double (&acc)[9],
                                             const typename K::Params &params, double (&w)[3]) {
    w[0] += K::finish(acc[7], params) - K::finish(acc[5], params);
    w[1] += K::finish(acc[2], params) - K::finish(acc[6], params);
    w[2] += K::finish(acc[3], params) - K::finish(acc[1], params);
}

/* This thread's share of one set through the functor K: records tid, tid + B,
 * ... of a buffer with STRIDE doubles a record onto the point x, finished by
 * the trace_finish of K's OUTDIM and added to part. The accumulators are the
 * walk's own locals: handed in by the caller they get other registers (as
 * many), and the kernels are no longer the bytes that were measured
 * (profiles/csrc_layout.md). */
template <typename K, int STRIDE, int B>
__device__ __forceinline__ void trace_walk(const double *__restrict__ rec, const long long n,
                                           const double (&x)[3],
                                           const typename K::Params &params,
                                           double (&part)[3]) {
    constexpr int R = rec_doubles<K>();
    double acc[K::OUTDIM];
#pragma unroll
    for (int j = 0; j < K::OUTDIM; ++j)
        acc[j] = 0.0;
    unsigned zmin = ~0u;
    for (long long s = threadIdx.x; s < n; s += B) {
        const double *__restrict__ p = rec + STRIDE * s;
        double v[R];
#pragma unroll
        for (int i = 0; i < R; ++i)
            v[i] = p[i];
        K::template pair<true>(x, v, v + 3, v + 3 + K::SRCDIM, acc, params, zmin);
    }
    trace_finish<K>(acc, params, part);
}

/* This thread's share of one set, added to part: through the velocity functor
 * V for the velocity, through the gradient functor G for the vorticity. G
 * walks V's records (same {r, f} prefix) at V's stride. */
template <int FIELD, typename V, typename G, int B>
__device__ __forceinline__ void trace_add_set(const double *__restrict__ rec, const long long n,
                                              const double (&x)[3],
                                              const typename V::Params &pv,
                                              const typename G::Params &pg, double (&part)[3]) {
    static_assert(G::SRCDIM == V::SRCDIM && G::AUXDIM == 0, "G reads the prefix of V's record");
    if constexpr (FIELD == TRACE_VORTICITY)
        trace_walk<G, rec_doubles<V>(), B>(rec, n, x, pg, part);
    else
        trace_walk<V, rec_doubles<V>(), B>(rec, n, x, pv, part);
}

/* The workgroup's sum of every thread's part, the same bits in every thread.
 * `red` is the workgroup's [2][B / 64][3] LDS block and `phase` its evaluation
 * counter. Must be called by all threads (uniform control flow). */
template <int B>
__device__ __forceinline__ void trace_reduce(double (&part)[3], double (*red)[B / 64][3],
                                             int &phase, double (&sum)[3]) {
    /* inside the wave: xor butterfly, all 64 lanes end with the same sum */
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            part[j] += __shfl_xor(part[j], m, 64);
    }
    /* across the waves: through LDS, summed in wave order by every thread */
    constexpr int NW = B / 64;
    const int buf = phase & 1;
    ++phase;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            red[buf][threadIdx.x >> 6][j] = part[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double s = red[buf][0][j];
#pragma unroll
        for (int w = 1; w < NW; ++w)
            s += red[buf][w][j];
        sum[j] = s;
    }
}

/* The body whose sphere holds x, the last one if several do, or -1; a scalar. */
__device__ __forceinline__ int trace_body_at(const TraceField &f, const double (&x)[3]) {
    int inside = -1;
    for (int b = 0; b < f.n_bodies; ++b) {
        const double *q = f.bodies + SKELLY_TRACE_BODY_DOUBLES * b;
        const double dx = x[0] - q[0], dy = x[1] - q[1], dz = x[2] - q[2];
        if (sqrt(dx * dx + dy * dy + dz * dz) < q[3])
            inside = b;
    }
    return __builtin_amdgcn_readfirstlane(inside);
}

/* The field that instantiation FIELD integrates and records, u(x) or
 * curl u(x), the same bits in every thread of the workgroup. `red` is the
 * workgroup's [2][B / 64][3] LDS block and `phase` its evaluation counter.
 * Must be called by all threads with the same x (uniform control flow). */
template <int B, int FIELD>
__device__ __forceinline__ void trace_rhs(const TraceField &f, const double (&x)[3],
                                          double (*red)[B / 64][3], int &phase, double (&k)[3]) {
    /* rigid motion inside a body: U_b + w_b x (x - c_b), whose curl is 2 w_b */
    const int inside = trace_body_at(f, x);
    if (inside >= 0) {
        const double *q = f.bodies + SKELLY_TRACE_BODY_DOUBLES * inside;
        if constexpr (FIELD == TRACE_VORTICITY) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                k[j] = 2.0 * q[7 + j];
        } else {
            const double dx = x[0] - q[0], dy = x[1] - q[1], dz = x[2] - q[2];
            k[0] = q[4] + (q[8] * dz - q[9] * dy);
            k[1] = q[5] + (q[9] * dx - q[7] * dz);
            k[2] = q[6] + (q[7] * dy - q[8] * dx);
        }
        return;
    }

    /* the regularized point forces go through StokesletGrad with reg and eps */
    double part[3] = {0.0, 0.0, 0.0};
    trace_add_set<FIELD, Stokeslet, StokesletGrad, B>(f.rec[0], f.n[0], x, f.sl, f.gsl, part);
    trace_add_set<FIELD, Stresslet, StressletGrad, B>(f.rec[1], f.n[1], x, f.dl, f.gdl, part);
    trace_add_set<FIELD, Rotlet, RotletGrad, B>(f.rec[2], f.n[2], x, f.rot, f.grot, part);
    trace_add_set<FIELD, OseenContract, StokesletGrad, B>(f.rec[3], f.n[3], x, f.os, f.gos, part);

    double sum[3];
    trace_reduce<B>(part, red, phase, sum);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if constexpr (FIELD == TRACE_VORTICITY)
            k[j] = sum[j] + f.bg_curl[j];
        else
            k[j] = sum[j] + (f.uniform[j] + x[f.components[j]] * f.bg_scale[j]);
    }
}

/* u(x), for the singularity stop of every FIELD. */
template <int B>
__device__ __forceinline__ void trace_field(const TraceField &f, const double (&x)[3],
                                            double (*red)[B / 64][3], int &phase,
                                            double (&u)[3]) {
    trace_rhs<B, TRACE_VELOCITY>(f, x, red, phase, u);
}

template <int B, int FIELD>
__global__ __launch_bounds__(B) void trace_lines_kernel(const TraceField f, const TraceJobs jobs) {
    __shared__ double red[2][B / 64][3];
    int phase = 0;

    const long long job = blockIdx.x;
    const bool backward = job >= jobs.n_seeds;
    const long long seed = backward ? job - jobs.n_seeds : job;
    const double t_final = backward ? -jobs.t_final : jobs.t_final;
    const double sgn = t_final < 0.0 ? -1.0 : 1.0;
    const int max_points = jobs.max_points;
    const long long max_tries = 4LL * max_points + 1000;
    constexpr double EPS = 2.220446049250313e-16; /* DBL_EPSILON */

    double x[3] = {jobs.seeds[3 * seed + 0], jobs.seeds[3 * seed + 1], jobs.seeds[3 * seed + 2]};
    double t = 0.0;
    double dt = backward ? -jobs.dt_init : jobs.dt_init;

    double *out_x = jobs.x + 3 * job * max_points;
    double *out_v = jobs.val + 3 * job * max_points;
    double *out_t = jobs.t + job * max_points;

    int count = 0, status = 0;
    long long tries = 0;
    bool running = true;
    while (running) {
        /* the point to record: the next start of a step, or the end point */
        const bool at_end = !(sgn * (t_final - t) > EPS);
        if (count == max_points) {
            status = 2;
            break;
        }
        double k1[3];
        trace_rhs<B, FIELD>(f, x, red, phase, k1);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                out_x[3 * count + j] = x[j];
                out_v[3 * count + j] = k1[j];
            }
            out_t[count] = t;
        }
        ++count;
        if (at_end)
            break;
        /* the stop is on the velocity, whatever the line follows */
        double u[3] = {k1[0], k1[1], k1[2]};
        if (FIELD != TRACE_VELOCITY)
            trace_field<B>(f, x, red, phase, u);
        const double speed = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        if (__builtin_amdgcn_readfirstlane(speed > 1e3)) {
            status = 1;
            break;
        }
        if (sgn * (t + dt - t_final) > EPS)
            dt = t_final - t;

        /* one step, retried with a smaller dt until its error passes */
        for (int fails = 0;;) {
            if (__builtin_amdgcn_readfirstlane(++tries > max_tries || fails >= 1000 ||
                                               t + dt == t)) {
                status = 3;
                running = false;
                break;
            }
            double k2[3], k3[3], k4[3], k5[3], k6[3], y[3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
                y[j] = x[j] + dt * ((1.0 / 5.0) * k1[j]);
            trace_rhs<B, FIELD>(f, y, red, phase, k2);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                y[j] = x[j] + dt * ((3.0 / 40.0) * k1[j] + (9.0 / 40.0) * k2[j]);
            trace_rhs<B, FIELD>(f, y, red, phase, k3);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                y[j] = x[j] + dt * ((3.0 / 10.0) * k1[j] + (-9.0 / 10.0) * k2[j] +
                                    (6.0 / 5.0) * k3[j]);
            trace_rhs<B, FIELD>(f, y, red, phase, k4);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                y[j] = x[j] + dt * ((-11.0 / 54.0) * k1[j] + (5.0 / 2.0) * k2[j] +
                                    (-70.0 / 27.0) * k3[j] + (35.0 / 27.0) * k4[j]);
            trace_rhs<B, FIELD>(f, y, red, phase, k5);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                y[j] = x[j] + dt * ((1631.0 / 55296.0) * k1[j] + (175.0 / 512.0) * k2[j] +
                                    (575.0 / 13824.0) * k3[j] + (44275.0 / 110592.0) * k4[j] +
                                    (253.0 / 4096.0) * k5[j]);
            trace_rhs<B, FIELD>(f, y, red, phase, k6);

            double x5[3], err = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                x5[j] = x[j] + dt * ((37.0 / 378.0) * k1[j] + (250.0 / 621.0) * k3[j] +
                                     (125.0 / 594.0) * k4[j] + (512.0 / 1771.0) * k6[j]);
                /* x5 - x4 */
                const double d =
                    dt * ((37.0 / 378.0 - 2825.0 / 27648.0) * k1[j] +
                          (250.0 / 621.0 - 18575.0 / 48384.0) * k3[j] +
                          (125.0 / 594.0 - 13525.0 / 55296.0) * k4[j] +
                          (-277.0 / 14336.0) * k5[j] + (512.0 / 1771.0 - 1.0 / 4.0) * k6[j]);
                const double e =
                    fabs(d) / (jobs.abs_err + jobs.rel_err * (fabs(x[j]) + fabs(dt) * fabs(k1[j])));
                err = (e > err || e != e) ? e : err; /* a NaN stays */
            }
            /* anything but err <= 1 (a NaN included) is a rejection */
            if (__builtin_amdgcn_readfirstlane(!(err <= 1.0))) {
                const double shrink = 0.9 * pow(err, -1.0 / 3.0);
                dt *= shrink > 0.2 ? shrink : 0.2; /* NaN -> 0.2 */
                ++fails;
                continue;
            }
            t += dt;
#pragma unroll
            for (int j = 0; j < 3; ++j)
                x[j] = x5[j];
            if (err < 0.5) {
                const double floor5 = 1.0 / 3125.0; /* 5^-5: growth at most 0.9 * 5 */
                dt *= 0.9 * pow(err > floor5 ? err : floor5, -1.0 / 5.0);
            }
            break;
        }
    }
    if (threadIdx.x == 0) {
        jobs.count[job] = count;
        jobs.status[job] = status;
    }
}

namespace skelly {

/* Doubles of a set's record buffer (none for an empty set, which is not packed). */
template <typename K>
static size_t trace_rec_doubles(long long n) {
    return n > 0 ? (size_t)rec_doubles<K>() * rec_count<K>(n) : 0;
}

/* curl of u_j = uniform_j + x[components_j] * scale_j: with the gradient
 * Gb[j][components_j] += scale_j it is (Gb21 - Gb12, Gb02 - Gb20, Gb10 - Gb01). */
static void trace_background_curl(const double scale[3], const int components[3], double curl[3]) {
    double g[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (int j = 0; j < 3; ++j)
        g[j][components[j]] += scale[j];
    curl[0] = g[2][1] - g[1][2];
    curl[1] = g[0][2] - g[2][0];
    curl[2] = g[1][0] - g[0][1];
}

hipError_t launch_trace_streamlines(const TraceRequest &q, hipStream_t stream) {
    const long long n_jobs = q.n_seeds * (q.back_integrate ? 2 : 1);
    if (n_jobs <= 0)
        return hipSuccess;
    if (q.max_points < 1 || q.max_points > (1 << 28) || n_jobs > 0x7fffffffLL ||
        q.n_bodies > 0x7fffffffLL)
        return hipErrorInvalidValue;
    for (int j = 0; j < 3; ++j)
        if (q.components[j] < 0 || q.components[j] > 2)
            return hipErrorInvalidValue;

    /* workspace: the four record buffers, back to back */
    const size_t len[4] = {trace_rec_doubles<Stokeslet>(q.n[0]), trace_rec_doubles<Stresslet>(q.n[1]),
                           trace_rec_doubles<Rotlet>(q.n[2]),
                           trace_rec_doubles<OseenContract>(q.n[3])};
    const size_t ws_bytes = (len[0] + len[1] + len[2] + len[3] + 1) * sizeof(double);
    LaunchWorkspace workspace;
    hipError_t err = workspace.acquire(stream, ws_bytes);
    if (err != hipSuccess)
        return err;

    TraceField f;
    const PairKernel set[4] = {PairKernel::Stokeslet, PairKernel::Stresslet, PairKernel::Rotlet,
                               PairKernel::OseenContract};
    double *at = workspace.get();
    for (int k = 0; k < 4; ++k) {
        f.rec[k] = at;
        f.n[k] = q.n[k];
        if (q.n[k] > 0)
            launch_pack_sources(set[k], q.r[k], q.f[k], q.n[k], at, stream);
        at += len[k];
    }
    f.sl = launch_params<Stokeslet>(q.scale_stokes, q.reg, q.eps);
    f.dl = launch_params<Stresslet>(q.scale_stokes, q.reg, q.eps);
    f.rot = launch_params<Rotlet>(q.scale_oseen, q.reg, q.eps);
    f.os = launch_params<OseenContract>(q.scale_oseen, q.reg, q.eps);
    /* the vorticity's functors: the prefactors of the gradient entry points */
    f.gsl = launch_params<StokesletGrad>(q.scale_stokes, 0.0, 0.0);
    f.gdl = launch_params<StressletGrad>(q.scale_stokes, q.reg, q.eps);
    f.grot = launch_params<RotletGrad>(q.scale_oseen, q.reg, q.eps);
    f.gos = launch_params<StokesletGrad>(q.scale_oseen, q.reg, q.eps);
    for (int j = 0; j < 3; ++j) {
        f.uniform[j] = q.uniform[j];
        f.bg_scale[j] = q.bg_scale[j];
        f.components[j] = q.components[j];
    }
    trace_background_curl(q.bg_scale, q.components, f.bg_curl);
    f.bodies = q.bodies;
    f.n_bodies = (int)q.n_bodies;

    TraceJobs jobs;
    jobs.seeds = q.seeds;
    jobs.n_seeds = q.n_seeds;
    jobs.dt_init = fabs(q.dt_init);
    jobs.t_final = q.t_final;
    jobs.abs_err = q.abs_err;
    jobs.rel_err = q.rel_err;
    jobs.max_points = (int)q.max_points;
    jobs.x = q.x;
    jobs.t = q.t;
    jobs.val = q.val;
    jobs.count = q.count;
    jobs.status = q.status;

    /* a job that never ran shows as count -1 (all bits set) */
    err = hipMemsetAsync(q.count, 0xFF, (size_t)n_jobs * sizeof(int), stream);
    if (err == hipSuccess) {
        const dim3 grid((unsigned)n_jobs), block(SKELLY_TRACE_BLOCK);
        if (q.vorticity)
            hipLaunchKernelGGL((trace_lines_kernel<SKELLY_TRACE_BLOCK, TRACE_VORTICITY>), grid,
                               block, 0, stream, f, jobs);
        else
            hipLaunchKernelGGL((trace_lines_kernel<SKELLY_TRACE_BLOCK, TRACE_VELOCITY>), grid,
                               block, 0, stream, f, jobs);
        err = hipGetLastError();
    }
    return workspace.finish(err);
}

int trace_block_size() { return SKELLY_TRACE_BLOCK; }

} // namespace skelly
