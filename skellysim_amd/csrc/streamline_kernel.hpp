/* streamline_kernel.hpp — the field-line tracer: one persistent workgroup per
 * job integrates dx/dt = u(x) (streamlines) or dx/dt = curl u(x) (vortex
 * lines) with adaptive Cash-Karp 5(4), every field evaluation, step decision
 * and record inside the one launch.
 *
 * Included by pair_kernels.hip (and by nothing else) behind its functors,
 * pack_sources and the workspace: the field is summed with the functors'
 * own K::pair<true> / K::finish over records that pack_sources<K> wrote, so
 * the per-pair arithmetic is the tested one.
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
 * Vorticity (trace_vorticity, the field of a vortex line): the curl of the
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

/* This thread's share of one set: records tid, tid + B, ... onto the point x,
 * finished (scaled), added to u. */
template <typename K, int B>
__device__ __forceinline__ void trace_add_set(const double *__restrict__ rec, const long long n,
                                              const double (&x)[3],
                                              const typename K::Params &params, double (&u)[3]) {
    constexpr int R = rec_doubles<K>();
    double acc[3] = {0.0, 0.0, 0.0};
    unsigned zmin = ~0u;
    for (long long s = threadIdx.x; s < n; s += B) {
        const double *__restrict__ p = rec + R * s;
        double v[R];
#pragma unroll
        for (int i = 0; i < R; ++i)
            v[i] = p[i];
        K::template pair<true>(x, v, v + 3, v + 3 + K::SRCDIM, acc, params, zmin);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
        u[j] += K::finish(acc[j], params);
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

/* u(x), the same bits in every thread of the workgroup. `red` is the
 * workgroup's [2][B / 64][3] LDS block and `phase` its evaluation counter.
 * Must be called by all threads with the same x (uniform control flow). */
template <int B>
__device__ __forceinline__ void trace_field(const TraceField &f, const double (&x)[3],
                                            double (*red)[B / 64][3], int &phase,
                                            double (&u)[3]) {
    /* rigid motion inside a body */
    const int inside = trace_body_at(f, x);
    if (inside >= 0) {
        const double *q = f.bodies + SKELLY_TRACE_BODY_DOUBLES * inside;
        const double dx = x[0] - q[0], dy = x[1] - q[1], dz = x[2] - q[2];
        u[0] = q[4] + (q[8] * dz - q[9] * dy);
        u[1] = q[5] + (q[9] * dx - q[7] * dz);
        u[2] = q[6] + (q[7] * dy - q[8] * dx);
        return;
    }

    double part[3] = {0.0, 0.0, 0.0};
    trace_add_set<Stokeslet, B>(f.rec[0], f.n[0], x, f.sl, part);
    trace_add_set<Stresslet, B>(f.rec[1], f.n[1], x, f.dl, part);
    trace_add_set<Rotlet, B>(f.rec[2], f.n[2], x, f.rot, part);
    trace_add_set<OseenContract, B>(f.rec[3], f.n[3], x, f.os, part);

    double sum[3];
    trace_reduce<B>(part, red, phase, sum);
#pragma unroll
    for (int j = 0; j < 3; ++j)
        u[j] = sum[j] + (f.uniform[j] + x[f.components[j]] * f.bg_scale[j]);
}

/* This thread's share of one set's vorticity: records tid, tid + B, ... of the
 * velocity functor V's buffer through the gradient functor K (same {r, f}
 * prefix), the partial gradient finished, its curl added to w. */
template <typename K, typename V, int B>
__device__ __forceinline__ void trace_add_curl(const double *__restrict__ rec, const long long n,
                                               const double (&x)[3],
                                               const typename K::Params &params, double (&w)[3]) {
    static_assert(K::SRCDIM == V::SRCDIM && K::AUXDIM == 0, "K reads the prefix of V's record");
    constexpr int STRIDE = rec_doubles<V>();
    constexpr int R = rec_doubles<K>();
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    unsigned zmin = ~0u;
    for (long long s = threadIdx.x; s < n; s += B) {
        const double *__restrict__ p = rec + STRIDE * s;
        double v[R];
#pragma unroll
        for (int i = 0; i < R; ++i)
            v[i] = p[i];
        K::template pair<true>(x, v, v + 3, v + 3 + K::SRCDIM, acc, params, zmin);
    }
    w[0] += K::finish(acc[7], params) - K::finish(acc[5], params);
    w[1] += K::finish(acc[2], params) - K::finish(acc[6], params);
    w[2] += K::finish(acc[3], params) - K::finish(acc[1], params);
}

/* curl u(x), the same bits in every thread; arguments and calling rule as
 * trace_field. */
template <int B>
__device__ __forceinline__ void trace_vorticity(const TraceField &f, const double (&x)[3],
                                                double (*red)[B / 64][3], int &phase,
                                                double (&w)[3]) {
    /* rigid rotation inside a body */
    const int inside = trace_body_at(f, x);
    if (inside >= 0) {
        const double *q = f.bodies + SKELLY_TRACE_BODY_DOUBLES * inside;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            w[j] = 2.0 * q[7 + j];
        return;
    }

    double part[3] = {0.0, 0.0, 0.0};
    trace_add_curl<StokesletGrad, Stokeslet, B>(f.rec[0], f.n[0], x, f.gsl, part);
    trace_add_curl<StressletGrad, Stresslet, B>(f.rec[1], f.n[1], x, f.gdl, part);
    trace_add_curl<RotletGrad, Rotlet, B>(f.rec[2], f.n[2], x, f.grot, part);
    trace_add_curl<StokesletGrad, OseenContract, B>(f.rec[3], f.n[3], x, f.gos, part);

    double sum[3];
    trace_reduce<B>(part, red, phase, sum);
#pragma unroll
    for (int j = 0; j < 3; ++j)
        w[j] = sum[j] + f.bg_curl[j];
}

/* The field that instantiation FIELD integrates and records. */
template <int B, int FIELD>
__device__ __forceinline__ void trace_rhs(const TraceField &f, const double (&x)[3],
                                          double (*red)[B / 64][3], int &phase, double (&k)[3]) {
    if (FIELD == TRACE_VORTICITY)
        trace_vorticity<B>(f, x, red, phase, k);
    else
        trace_field<B>(f, x, red, phase, k);
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

/* Pack one set into the workspace at `rec` (nothing for an empty set). */
template <typename K>
static void trace_pack(const double *r_src, const double *f_src, long long n, double *rec,
                       hipStream_t stream) {
    if (n <= 0)
        return;
    const long long total = (long long)rec_doubles<K>() * rec_count<K>(n);
    hipLaunchKernelGGL((pack_sources<K>), dim3((unsigned)((total + BLOCK - 1) / BLOCK)),
                       dim3(BLOCK), 0, stream, r_src, f_src, rec, n);
}

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

    TraceField f;
    double *at = workspace;
    for (int k = 0; k < 4; ++k) {
        f.rec[k] = at;
        f.n[k] = q.n[k];
        at += len[k];
    }
    trace_pack<Stokeslet>(q.r[0], q.f[0], q.n[0], workspace, stream);
    trace_pack<Stresslet>(q.r[1], q.f[1], q.n[1], workspace + len[0], stream);
    trace_pack<Rotlet>(q.r[2], q.f[2], q.n[2], workspace + len[0] + len[1], stream);
    trace_pack<OseenContract>(q.r[3], q.f[3], q.n[3], workspace + len[0] + len[1] + len[2],
                              stream);
    /* the functors accumulate ACC_FOLD x the sum (launch_pair) */
    f.sl = Stokeslet::make_params(q.scale_stokes, q.reg, q.eps);
    f.sl.scale /= Stokeslet::ACC_FOLD;
    f.dl = Stresslet::make_params(q.scale_stokes, q.reg, q.eps);
    f.dl.scale /= Stresslet::ACC_FOLD;
    f.rot = Rotlet::make_params(q.scale_oseen, q.reg, q.eps);
    f.rot.scale /= Rotlet::ACC_FOLD;
    f.os = OseenContract::make_params(q.scale_oseen, q.reg, q.eps);
    f.os.scale /= OseenContract::ACC_FOLD;
    /* the vorticity's functors: the prefactors of the gradient entry points */
    f.gsl = StokesletGrad::make_params(q.scale_stokes, 0.0, 0.0);
    f.gsl.scale /= StokesletGrad::ACC_FOLD;
    f.gdl = StressletGrad::make_params(q.scale_stokes, q.reg, q.eps);
    f.gdl.scale /= StressletGrad::ACC_FOLD;
    f.grot = RotletGrad::make_params(q.scale_oseen, q.reg, q.eps);
    f.grot.scale /= RotletGrad::ACC_FOLD;
    f.gos = StokesletGrad::make_params(q.scale_oseen, q.reg, q.eps);
    f.gos.scale /= StokesletGrad::ACC_FOLD;
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
    hipError_t err = hipMemsetAsync(q.count, 0xFF, (size_t)n_jobs * sizeof(int), stream);
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
    if (pooled)
        return err;
    hipError_t err2 = hipFreeAsync(workspace, stream);
    return err != hipSuccess ? err : err2;
}

int trace_block_size() { return SKELLY_TRACE_BLOCK; }

} // namespace skelly
