/* pair_kernels.hpp — the seam between the C-ABI layer (skelly_hip.cpp) and the
 * kernel units (pair_kernels.hip, trace_kernels.hip, probe_kernels.hip), and
 * between those units. Each includes it, so a changed signature fails to
 * compile instead of failing when the library loads. */

#ifndef SKELLY_PAIR_KERNELS_HPP
#define SKELLY_PAIR_KERNELS_HPP

#include <hip/hip_runtime.h>

namespace skelly {

/* The pair functors of pair_functors.hpp, by name. */
enum class PairKernel {
    Stokeslet,
    Stresslet,
    OseenContract,
    Rotlet,
    StressletNormalDensity,
    StokesletGrad, /* also the regularized Oseen gradient (reg, eps != 0) */
    StressletGrad,
    RotletGrad,
    StokesletPressure, /* also the regularized Oseen pressure (reg, eps != 0) */
    StressletPressure,
    Nearest, /* arg-min, not a sum: strengths {index, group}, 4-wide targets {r, group} */
};

/* Doubles per source of the strength array and per target of the output
 * (K::SRCDIM, K::OUTDIM). */
struct PairDims {
    int srcdim;
    int outdim;
};
PairDims pair_kernel_dims(PairKernel kernel);

/* One launch of `kernel` on device pointers: f_src is (n_src, srcdim), out
 * (n_trg, outdim). scale is the kernel's prefactor as the caller computed it;
 * reg and eps are read by the regularized functors only (K::make_params). */
hipError_t launch_pair_kernel(PairKernel kernel, const double *r_src, const double *f_src,
                              const double *r_trg, double *out, long long n_src, long long n_trg,
                              double scale, double reg, double eps, hipStream_t stream);

/* Per target the nearest source whose group differs from the target's (every
 * source without groups: both group pointers null): d2[t] = min |t - s|^2 and
 * index[t] the lowest source index that attains it, +inf and -1 without an
 * eligible source. Device pointers, asynchronous on `stream`; every
 * intermediate lives in the stream's launch workspace. */
hipError_t launch_nearest(const double *r_src, const long long *src_group, long long n_src,
                          const double *r_trg, const long long *trg_group, long long n_trg,
                          double *d2, long long *index, hipStream_t stream);

/* n_src sources as `kernel`'s packed records into `rec`, which holds
 * rec_doubles<K>() * rec_count<K>(n_src) doubles (pair_functors.hpp):
 * pack_sources<K>, asynchronous on `stream`. The tracer packs its sets here. */
void launch_pack_sources(PairKernel kernel, const double *r_src, const double *f_src,
                         long long n_src, double *rec, hipStream_t stream);

/* One launch of the field-line tracer (trace_kernels.hip), asynchronous on
 * `stream`: the four source sets are packed into the stream's workspace and
 * every seed is integrated forward (and backward with back_integrate) by a
 * workgroup of its own. All pointers are device pointers. */
struct TraceRequest {
    /* 0: streamlines, dx/dt = u, val = u. Else vortex lines: dx/dt = curl u and
     * val = curl u, the |u| > 1e3 stop still on the velocity. */
    int vorticity;
    /* Stokeslet, Stresslet (9 doubles a source), Rotlet, OseenContract */
    const double *r[4], *f[4];
    long long n[4];
    double scale_stokes, scale_oseen; /* the prefactors of the velocity entry points */
    double reg, eps;
    double uniform[3], bg_scale[3]; /* background: uniform_j + x[components_j] * bg_scale_j */
    int components[3];
    const double *bodies; /* (n_bodies, 10): centre, radius, velocity, angular velocity */
    long long n_bodies;
    const double *seeds; /* (n_seeds, 3) */
    long long n_seeds;
    int back_integrate; /* jobs: n_seeds forward, then n_seeds backward */
    double dt_init, t_final, abs_err, rel_err;
    long long max_points;
    double *x, *t, *val; /* (n_jobs, max_points, 3), (n_jobs, max_points), as x */
    int *count, *status; /* (n_jobs) */
};
hipError_t launch_trace_streamlines(const TraceRequest &q, hipStream_t stream);
/* Threads of a tracer workgroup (compile-time, SKELLY_TRACE_BLOCK). */
int trace_block_size();

/* Dense builders (pair_kernels.hip). */
hipError_t launch_oseen_tensor_batched(const double *pts, double *G, long long nf, long long n,
                                       double eta, double reg, double eps, hipStream_t stream);
hipError_t launch_stresslet_times_normal(const double *pts, const double *normals, double *G,
                                         long long n, double reg, double eps, hipStream_t stream);

/* Microbenchmarks and probes (probe_kernels.hip): the fp64 FMA peak. */
hipError_t run_fp64_peak(double *out_tflops);
/* out[3]: cost of a v_rsq_f64 and of a broadcast ds_read_b128 in v_fma_f64
 * issue slots, and the base run's TFLOP/s. */
hipError_t run_issue_cost_probe(double *out);
/* seed[i] = v_rsq_f64(x[i]), refined[i] = rsq_x2(x[i]) = 2/sqrt(x[i]) as the
 * functors compute it; device pointers of n doubles each. */
hipError_t launch_rsq_probe(const double *x, double *seed, double *refined, long long n,
                            hipStream_t stream);

} // namespace skelly

#endif /* SKELLY_PAIR_KERNELS_HPP */
