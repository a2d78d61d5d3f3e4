/* skelly_hip.h — C-ABI boundary of the MI355X-native SkellySim hot-path engine.
 *
 * This is the drop-in seam for SkellySim's pair-kernel evaluators
 * (flatironinstitute/SkellySim, read-only reference at /root/reference):
 * the reference selects an Evaluator backend by string ("CPU"/"GPU"/"FMM") at
 * src/core/fiber_container_base.cpp:20-33, src/core/body_container.cpp:552-573
 * and src/core/periphery.cpp:337-352; the "GPU" branch bottoms out in the two
 * C-linkage-style entry points declared at include/kernels.hpp:17-20. This
 * library exports those two entry points (same names, same argument meaning)
 * plus extended device-pointer forms for multi-GPU sharding. See
 * INTEGRATION.md for the reference-side binding a maintainer would add.
 *
 * Layout contract (include/kernels.hpp:14-15): all matrices are fp64,
 * col-major 3 x n — i.e. per-point xyz contiguous. Stresslet strengths are
 * 9 x n (the 9-component double-layer tensor, kernels.cu:41-43).
 *
 * Scaling contract: the *_direct_gpu_impl results INCLUDE the 1/(8*pi) kernel
 * prefactor (applied per target, kernels.cu:59,122) and EXCLUDE the 1/eta
 * division (the reference host wrapper divides, kernels.cpp:358,365). The
 * skelly_*_device / skelly_*_host forms take eta and return fully scaled
 * velocities (1/(8*pi*eta)).
 *
 * Error contract: the reference exits the process on CUDA failure
 * (kernels.cu:9-15); this library instead returns nonzero error codes
 * (int-returning functions) and records a message retrievable via
 * skelly_hip_last_error(). The void reference-signature wrappers record the
 * error and leave u_trg untouched. A negative count is such an error in every
 * entry point, found before any HIP call ("<entry point>: negative size"); a
 * zero count is not one.
 *
 * Threading: calls are serialized by an internal mutex per the reference's
 * MPI_THREAD_FUNNELED usage (src/skelly_sim.cpp:14) — re-entrant per
 * evaluation, not concurrently invoked.
 *
 * Determinism: accumulation order per target is fixed (source-tile order), so
 * results are bit-reproducible for a given device count and shard layout.
 */

#ifndef SKELLY_HIP_H
#define SKELLY_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library / device management ---- */

/* Where every pair launch, host and device forms alike, takes its workspace
 * (source records and slice partials) from, overriding the SKELLY_PERSISTENT_WS
 * env var (on=-1 follows it again): on=1 (default) a grow-only hipMalloc block
 * kept per (device, stream), on=0 a hipMallocAsync/hipFreeAsync pair per
 * launch. Leave it on:
 * with the mempool workspace synchronised back-to-back calls of different
 * kernels have returned wrong results ("Launch workspace"), and
 * its allocations cannot be captured into a hipGraph, while the persistent
 * block allocates only when a launch outgrows it (in uncaptured warmup). A
 * block lives as long as its stream is in use by this library; the host
 * forms' own is released by skelly_hip_shutdown(). */
void skelly_set_persistent_ws(int on);

/* Capacity in bytes of the persistent workspace block kept for `stream` on
 * the current device, 0 if there is none, into *out_bytes. For tests and
 * memory accounting. 0 on success. */
int skelly_persistent_ws_bytes(void *stream, long long *out_bytes);

/* Mode of the pair kernels' unmasked fast path, overriding the
 * SKELLY_PAIR_FASTPATH env var: 0 = off (every pair goes through the r==0
 * mask), 1 = auto (default: on for launches whose blocks each walk >= 8192
 * sources, where its rerun of chunks that hold coincident points cannot
 * outweigh its gain), 2 = always on. Results are bit-identical in every
 * mode; the switch exists for A/B timing and for the tests that check that. */
void skelly_set_pair_fastpath(int mode);

/* Source-slice count of the pair kernels' split launches (overrides the env
 * var SKELLY_PAIR_SLICES). 0 = chosen per launch by the CU load-balance
 * planner (default); n >= 1 = exactly n slices, clamped only to the source
 * count (and the grid limit 65535), for sweeps and tests. The slice count
 * fixes the per-target summation order: results are bit-reproducible for a
 * given count and agree to rounding between counts. */
void skelly_set_pair_slices(int n);

/* Human-readable build id ("skelly-hip <ver> gfx950"). */
const char *skelly_hip_version(void);

/* Last error message for this thread; empty string if none. */
const char *skelly_hip_last_error(void);

/* Number of visible HIP devices; <0 on error. */
int skelly_hip_device_count(void);

/* Select the device used by subsequent calls (default 0). 0 on success. */
int skelly_hip_set_device(int device);

/* Release all persistent device buffers and streams, the host forms' launch
 * workspace included. 0 on success; the next call sets everything up again. */
int skelly_hip_shutdown(void);

/* ---- reference drop-in entry points (include/kernels.hpp:17-20) ----
 *
 * Host pointers in/out; this library owns all device management. Unlike the
 * reference CUDA path (cudaMalloc/copy/free on every call, kernels.cu:149-178)
 * device buffers are persistent and grow-only across calls.
 * f_src is 3 doubles/point for the stokeslet, 9 for the stresslet.
 * u_trg (3 x n_trg) is overwritten (not accumulated), scaled by 1/(8*pi),
 * NOT divided by eta. On failure u_trg is untouched and
 * skelly_hip_last_error() is set. */
void stokeslet_direct_gpu_impl(const double *r_src, const double *f_src, int n_src,
                               const double *r_trg, double *u_trg, int n_trg);
void stresslet_direct_gpu_impl(const double *r_src, const double *f_src, int n_src,
                               const double *r_trg, double *u_trg, int n_trg);

/* ---- extended host-pointer API (fully scaled, returns error codes) ---- */

int skelly_stokeslet_host(const double *r_src, const double *f_src, long long n_src,
                          const double *r_trg, double *u_trg, long long n_trg, double eta);
int skelly_stresslet_host(const double *r_src, const double *f_src, long long n_src,
                          const double *r_trg, double *u_trg, long long n_trg, double eta);
/* Regularized Oseen contraction (kernels.cpp:85-131; defaults reg=5e-3,
 * epsilon_distance=1e-5 per kernels.hpp:34-35). */
int skelly_oseen_contract_host(const double *r_src, const double *r_trg, const double *density,
                               double *u_trg, long long n_src, long long n_trg,
                               double eta, double reg, double epsilon_distance);
/* Rotlet (kernels.cpp:206-242). */
int skelly_rotlet_host(const double *r_src, const double *r_trg, const double *density,
                       double *u_trg, long long n_src, long long n_trg,
                       double eta, double reg, double epsilon_distance);

/* ---- device-pointer API (for torch/RCCL plumbing; async on `stream`) ----
 *
 * All pointers are DEVICE pointers on the current device; `stream` is a
 * hipStream_t (pass e.g. torch.cuda.current_stream().cuda_stream), or NULL
 * for the null stream. No synchronization is performed. Results are fully
 * scaled (1/(8*pi*eta); oseen/rotlet regularization per the reference). */
int skelly_stokeslet_device(const double *d_r_src, const double *d_f_src, long long n_src,
                            const double *d_r_trg, double *d_u_trg, long long n_trg,
                            double eta, void *stream);
int skelly_stresslet_device(const double *d_r_src, const double *d_f_src, long long n_src,
                            const double *d_r_trg, double *d_u_trg, long long n_trg,
                            double eta, void *stream);
int skelly_oseen_contract_device(const double *d_r_src, const double *d_r_trg,
                                 const double *d_density, double *d_u_trg,
                                 long long n_src, long long n_trg,
                                 double eta, double reg, double epsilon_distance, void *stream);
int skelly_rotlet_device(const double *d_r_src, const double *d_r_trg,
                         const double *d_density, double *d_u_trg,
                         long long n_src, long long n_trg,
                         double eta, double reg, double epsilon_distance, void *stream);

/* ---- velocity gradients (analytic, one pass) ----
 *
 * G[i][j] = d u_i / d x_j of the matching velocity entry point, differentiated
 * at the target: g_trg is double[9 * n_trg], row-major per target
 * (G[i][j] at 9*it + 3*i + j), overwritten, fully scaled (1/(8*pi*eta)).
 * Argument order and error contract are those of the velocity forms. Each
 * formula is the exact derivative inside each branch of its kernel:
 * coincident pairs contribute zero for stokeslet/stresslet/oseen, pairs
 * under epsilon_distance differentiate the regularized expression. Results
 * are bit-reproducible and independent of skelly_set_pair_fastpath. */
int skelly_stokeslet_grad_host(const double *r_src, const double *f_src, long long n_src,
                               const double *r_trg, double *g_trg, long long n_trg, double eta);
int skelly_stresslet_grad_host(const double *r_src, const double *f_src, long long n_src,
                               const double *r_trg, double *g_trg, long long n_trg, double eta);
int skelly_oseen_contract_grad_host(const double *r_src, const double *r_trg,
                                    const double *density, double *g_trg,
                                    long long n_src, long long n_trg,
                                    double eta, double reg, double epsilon_distance);
int skelly_rotlet_grad_host(const double *r_src, const double *r_trg, const double *density,
                            double *g_trg, long long n_src, long long n_trg,
                            double eta, double reg, double epsilon_distance);
int skelly_stokeslet_grad_device(const double *d_r_src, const double *d_f_src, long long n_src,
                                 const double *d_r_trg, double *d_g_trg, long long n_trg,
                                 double eta, void *stream);
int skelly_stresslet_grad_device(const double *d_r_src, const double *d_f_src, long long n_src,
                                 const double *d_r_trg, double *d_g_trg, long long n_trg,
                                 double eta, void *stream);
int skelly_oseen_contract_grad_device(const double *d_r_src, const double *d_r_trg,
                                      const double *d_density, double *d_g_trg,
                                      long long n_src, long long n_trg,
                                      double eta, double reg, double epsilon_distance,
                                      void *stream);
int skelly_rotlet_grad_device(const double *d_r_src, const double *d_r_trg,
                              const double *d_density, double *d_g_trg,
                              long long n_src, long long n_trg,
                              double eta, double reg, double epsilon_distance, void *stream);

/* ---- pressures ----
 *
 * The Stokes pressure p that belongs to the velocity entry points, so that
 * the stress is sigma = -p I + eta (G + G^T) with G from the gradient forms.
 * With d = t - s and y = 1/sqrt(den):
 *   stokeslet        p = 1/(4 pi) sum (f.d) y^3,                 den = r^2
 *   oseen_contract   the same expression with the velocity kernel's den
 *                    (r^2 > eps^2 ? r^2 : r^2 + reg^2): the definition of the
 *                    regularized branch
 *   stresslet        p = 1/(4 pi) sum [ tr(S) y^3 - 3 (d^T S d) y^5 ],
 *                    S_kl = f_src[9 s + 3 k + l],                den = r^2
 * Coincident pairs (r == 0) contribute exactly 0. No pressure depends on eta,
 * so these forms take none (a double layer's f_dl = 2 eta n (x) rho carries
 * its own). The rotlet's pressure is zero: it has no entry point.
 * p_trg is double[n_trg], overwritten. Argument order and error contract are
 * those of the velocity forms without eta; the device forms are asynchronous
 * on `stream`, perform no synchronization and use the persistent workspace.
 * Results are bit-reproducible and independent of skelly_set_pair_fastpath. */
int skelly_stokeslet_pressure_host(const double *r_src, const double *f_src, long long n_src,
                                   const double *r_trg, double *p_trg, long long n_trg);
int skelly_stresslet_pressure_host(const double *r_src, const double *f_src, long long n_src,
                                   const double *r_trg, double *p_trg, long long n_trg);
int skelly_oseen_contract_pressure_host(const double *r_src, const double *r_trg,
                                        const double *density, double *p_trg,
                                        long long n_src, long long n_trg,
                                        double reg, double epsilon_distance);
int skelly_stokeslet_pressure_device(const double *d_r_src, const double *d_f_src,
                                     long long n_src, const double *d_r_trg, double *d_p_trg,
                                     long long n_trg, void *stream);
int skelly_stresslet_pressure_device(const double *d_r_src, const double *d_f_src,
                                     long long n_src, const double *d_r_trg, double *d_p_trg,
                                     long long n_trg, void *stream);
int skelly_oseen_contract_pressure_device(const double *d_r_src, const double *d_r_trg,
                                          const double *d_density, double *d_p_trg,
                                          long long n_src, long long n_trg,
                                          double reg, double epsilon_distance, void *stream);

/* ---- nearest source ----
 *
 * For every target the nearest eligible source: d2[t] = min |r_trg[t] -
 * r_src[s]|^2 (squared, no root is taken) and index[t] the s that attains it.
 * A source is eligible when its group id differs from the target's; with both
 * group pointers NULL every source is eligible. Exactly one NULL group pointer
 * is an error, found like a negative count before any HIP call
 * ("<entry point>: one group array without the other").
 *   Ties     among equal d2 the lowest source index wins.
 *   Nothing  no eligible source (n_src == 0, every source in the target's
 *            group, a target with a NaN coordinate): d2 = +inf, index = -1.
 *   NaN      a source with a NaN coordinate is never returned.
 *   Zero     a coincident eligible source is a hit with d2 == 0.
 * d2 is computed as fma(dz, dz, fma(dy, dy, dx * dx)), d = r_trg - r_src.
 * Results are bit-identical for every source-slice count
 * (skelly_set_pair_slices) and from run to run: a minimum has no summation
 * order. d_d2 is double[n_trg], d_index long long[n_trg], both overwritten.
 * The device form is asynchronous on `stream`, performs no synchronization and
 * takes all its scratch (packed records, partials, the converted group ids)
 * from the stream's persistent workspace, so after one warm-up call it
 * allocates nothing and can be captured. n_trg == 0 returns 0 and touches
 * nothing. */
int skelly_nearest_device(const double *d_r_src, const long long *d_src_group, long long n_src,
                          const double *d_r_trg, const long long *d_trg_group, long long n_trg,
                          double *d_d2, long long *d_index, void *stream);
int skelly_nearest_host(const double *r_src, const long long *src_group, long long n_src,
                        const double *r_trg, const long long *trg_group, long long n_trg,
                        double *d2, long long *index);

/* Contraction of the stresslet with a normal and a density field over one
 * point set (kernels::stresslet_times_normal_times_density,
 * src/core/kernels.cpp:307-334; no eta dependence, factor -3/(4*pi)):
 * out_i = factor * sum_{j != i} (d.rho_j)(d.n_j)/|d|^5 d, d = r_i - r_j,
 * |d| < epsilon_distance regularized to sqrt(|d|^2 + reg^2).
 * Used by the body/fiber operator assembly. Defaults reg=5e-3, eps=1e-5
 * (include/kernels.hpp:50-51). */
int skelly_stresslet_normal_density_host(const double *r_src, const double *normals,
                                         const double *density, double *out, long long n,
                                         double reg, double epsilon_distance);
/* device form: nd is the interleaved (n, 6) [normal | density] array */
int skelly_stresslet_normal_density_device(const double *d_r_src, const double *d_nd,
                                           const double *d_r_trg, double *d_out,
                                           long long n_src, long long n_trg,
                                           double reg, double epsilon_distance, void *stream);

/* Dense stresslet_times_normal builder (kernels::stresslet_times_normal,
 * src/core/kernels.cpp:264-287; body operator assembly): pts/normals (n, 3)
 * -> Snormal (3n, 3n) C row-major, diagonal blocks zero. Device pointers. */
int skelly_stresslet_times_normal_device(const double *d_pts, const double *d_normals,
                                         double *d_out, long long n, double reg,
                                         double epsilon_distance, void *stream);

/* Batched oseen_tensor_direct dense builder (kernels::oseen_tensor_direct,
 * src/core/kernels.cpp:146-195, square/self form — the per-fiber
 * self-stokeslet build, src/core/fiber_finite_difference.cpp:56):
 * pts (nf, n, 3) -> G (nf, 3n, 3n) row-major; coincident blocks zero. */
int skelly_oseen_tensor_batched_device(const double *d_pts, double *d_G, long long nf,
                                       long long n, double eta, double reg,
                                       double epsilon_distance, void *stream);

/* ---- streamlines ----
 *
 * Integrates dx/dt = u(x) from every seed with adaptive Cash-Karp 5(4) in one
 * kernel launch, a workgroup per job, no host round trip per step. A job is
 * one seed in one direction: job j < n_seeds runs seed j from t = 0 to
 * +t_final, and with back_integrate != 0 job n_seeds + j runs it to -t_final
 * (n_jobs = n_seeds or 2 n_seeds).
 *
 * u is the sum of four source sets, each possibly empty (n = 0, pointers
 * unread): Stokeslets (sl: 3 doubles a source, skelly_stokeslet_*'s field),
 * stresslets (dl: 9, skelly_stresslet_*), rotlets (rot: 3, skelly_rotlet_*)
 * and regularized Stokeslets (os: 3, skelly_oseen_contract_*), scaled and
 * regularized as those entry points do with (eta, reg, epsilon_distance);
 * plus the background, `background` = {uniform[3], scale[3], components[3]}
 * (9 doubles ON THE HOST in both forms, read during the call, components as
 * 0.0/1.0/2.0; NULL for none): u_j += uniform_j + x[components_j] * scale_j.
 * A point inside a body, |x - c_b| < radius_b, has u = U_b + w_b x (x - c_b)
 * instead, the last such body deciding; bodies is (n_bodies, 10) rows
 * {c[3], radius, U[3], w[3]}.
 *
 * Step control (Boost.Odeint controlled_runge_kutta with
 * default_error_checker(abs_err, rel_err, 1, 1) under integrate_adaptive;
 * DESIGN.md, "Streamlines on the device"): the first step is dt_init, the
 * start of every step is recorded with its velocity, a step is retried with
 * dt * max(0.9 err^(-1/3), 0.2) while err > 1, and the next one grows by
 * 0.9 max(5^-5, err)^(-1/5) when err < 0.5; the last step is clipped to end
 * on t_final and the end point is recorded.
 *
 * Outputs per job: x (max_points x 3), t (max_points), val (max_points x 3,
 * the velocity at each recorded point), of which the first count[job] rows are
 * written, and status[job]:
 *   0  t_final reached;
 *   1  |u| > 1e3 at a recorded point (a singularity; the point is the last
 *      one recorded);
 *   2  the buffer is full: count == max_points;
 *   3  the step control gave up (1000 rejections of one step, a step that
 *      does not move t, or more than 4 max_points + 1000 tries).
 * count is written as -1 before the launch, so a job that never ran shows.
 * Results are bit-reproducible, independent of which other seeds share the
 * call and of the pair kernels' slice and fast-path switches.
 *
 * The device form is asynchronous on `stream`, performs no synchronization
 * and packs the sources into the stream's persistent workspace; the host form
 * takes host pointers throughout. A negative count (max_points included) is an
 * error before any HIP call; n_seeds == 0 returns 0 and touches nothing. */
int skelly_trace_streamlines_device(
    const double *d_sl_r, const double *d_sl_f, long long n_sl,
    const double *d_dl_r, const double *d_dl_f, long long n_dl,
    const double *d_rot_r, const double *d_rot_f, long long n_rot,
    const double *d_os_r, const double *d_os_f, long long n_os,
    const double *background, const double *d_bodies, long long n_bodies,
    const double *d_seeds, long long n_seeds, int back_integrate,
    double eta, double reg, double epsilon_distance,
    double dt_init, double t_final, double abs_err, double rel_err, long long max_points,
    double *d_x, double *d_t, double *d_val, int *d_count, int *d_status, void *stream);
int skelly_trace_streamlines_host(
    const double *sl_r, const double *sl_f, long long n_sl,
    const double *dl_r, const double *dl_f, long long n_dl,
    const double *rot_r, const double *rot_f, long long n_rot,
    const double *os_r, const double *os_f, long long n_os,
    const double *background, const double *bodies, long long n_bodies,
    const double *seeds, long long n_seeds, int back_integrate,
    double eta, double reg, double epsilon_distance,
    double dt_init, double t_final, double abs_err, double rel_err, long long max_points,
    double *x, double *t, double *val, int *count, int *status);

/* ---- vortex lines ----
 *
 * The same tracer on the vorticity: dx/dt = w(x), w = curl u of the field
 * above, summed analytically through the velocity-gradient kernels
 * (skelly_stokeslet_grad_*, skelly_stresslet_grad_*, skelly_rotlet_grad_* and
 * skelly_oseen_contract_grad_* with the same eta, reg, epsilon_distance) plus
 * the constant curl of the background. A point inside a body has w = 2 w_b,
 * the last such body deciding. Arguments, jobs, step control, outputs and
 * the contract of the two forms are those of skelly_trace_streamlines_*, with
 * two differences: val is the vorticity at each recorded point, and status 1
 * is still a stop on the VELOCITY (|u| > 1e3 at a recorded point, evaluated
 * there beside w, as the reference's observer does), so a line may run through
 * a large vorticity and stops where a streamline would. */
int skelly_trace_vortexlines_device(
    const double *d_sl_r, const double *d_sl_f, long long n_sl,
    const double *d_dl_r, const double *d_dl_f, long long n_dl,
    const double *d_rot_r, const double *d_rot_f, long long n_rot,
    const double *d_os_r, const double *d_os_f, long long n_os,
    const double *background, const double *d_bodies, long long n_bodies,
    const double *d_seeds, long long n_seeds, int back_integrate,
    double eta, double reg, double epsilon_distance,
    double dt_init, double t_final, double abs_err, double rel_err, long long max_points,
    double *d_x, double *d_t, double *d_val, int *d_count, int *d_status, void *stream);
int skelly_trace_vortexlines_host(
    const double *sl_r, const double *sl_f, long long n_sl,
    const double *dl_r, const double *dl_f, long long n_dl,
    const double *rot_r, const double *rot_f, long long n_rot,
    const double *os_r, const double *os_f, long long n_os,
    const double *background, const double *bodies, long long n_bodies,
    const double *seeds, long long n_seeds, int back_integrate,
    double eta, double reg, double epsilon_distance,
    double dt_init, double t_final, double abs_err, double rel_err, long long max_points,
    double *x, double *t, double *val, int *count, int *status);

/* Threads of a tracer workgroup: a compile-time constant of the library
 * (SKELLY_TRACE_BLOCK), for the record of a measurement. */
int skelly_trace_block_size(void);

/* ---- measurement helpers ---- */

/* Measured fp64 FMA throughput (TFLOP/s) of the current device via a pure
 * register FMA chain — used to pin the roofline denominator. 0 on success. */
int skelly_fp64_peak_tflops(double *out_tflops);

/* What the pair loop's two non-FMA instruction kinds cost on the current
 * device, measured as the fp64 FMA rate they take away when interleaved with
 * independent v_fma_f64 (4 to 64): out3[0] one independent v_rsq_f64 and
 * out3[1] one broadcast ds_read_b128, both in issue slots of a v_fma_f64
 * (4 SIMD cycles each); out3[2] the TFLOP/s of the run without insertions.
 * 0 on success. */
int skelly_issue_cost_probe(double *out3);

/* The pair kernels' reciprocal square root, argument by argument: for each of
 * the n doubles of d_x, d_seed gets the raw v_rsq_f64 and d_refined the
 * refined R = 2/sqrt(x) that every functor and dense builder computes with
 * (x == 0 gives inf and NaN, x == inf gives 0 and NaN: what the r == 0 mask
 * relies on). Device pointers, async on `stream`, no synchronization.
 * 0 on success. */
int skelly_rsq_accuracy_probe(const double *d_x, double *d_seed, double *d_refined, long long n,
                              void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SKELLY_HIP_H */
