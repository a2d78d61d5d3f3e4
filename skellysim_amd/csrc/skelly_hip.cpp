/* skelly_hip.cpp — C-ABI host layer over the CDNA4 pair kernels.
 *
 * Implements include/skelly_hip.h: the reference drop-in entry points
 * (SkellySim include/kernels.hpp:17-20) plus extended host/device forms.
 * Replaces the reference's per-call cudaMalloc/copy/free round trip
 * (src/core/kernels.cu:149-178) with persistent grow-only device buffers and
 * a dedicated HIP stream.
 */

#include "skelly_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <mutex>
#include <string>

#include "launch_workspace.hpp"
#include "pair_kernels.hpp"

using skelly::PairKernel;

namespace {

constexpr double kOneOver8Pi = 1.0 / 8.0 / M_PI; /* kernels.cu:59 */
constexpr double kOneOver4Pi = 1.0 / (4.0 * M_PI); /* the pressures' prefactor */

thread_local std::string g_last_error;

void set_error(const char *where, const char *what) {
    g_last_error = std::string(where) + ": " + what;
    std::fprintf(stderr, "[skelly-hip] %s\n", g_last_error.c_str());
}

void set_error(const char *where, hipError_t err) { set_error(where, hipGetErrorString(err)); }

/* The argument check every entry point makes before its first HIP call: a
 * negative count is an error of the caller's (message recorded, -1), never a
 * launch and never a buffer size. */
bool negative_size(const char *where, long long a, long long b = 0) {
    if (a >= 0 && b >= 0)
        return false;
    set_error(where, "negative size");
    return true;
}

/* The nearest-source entry points take both group arrays or neither: one
 * without the other is an error of the caller's, found like a negative count. */
bool lone_group(const char *where, const void *src_group, const void *trg_group) {
    if ((src_group == nullptr) == (trg_group == nullptr))
        return false;
    set_error(where, "one group array without the other");
    return true;
}

/* Persistent per-process device state. Calls are serialized (the reference is
 * MPI_THREAD_FUNNELED, skelly_sim.cpp:14). */
struct Context {
    std::mutex mu;
    int device = 0;
    bool stream_ready = false;
    hipStream_t stream = nullptr;

    enum Role { R_SRC = 0, F_SRC, R_TRG, U_TRG, N_ROLES };
    void *buf[N_ROLES] = {};
    size_t cap[N_ROLES] = {};

    hipError_t ensure_stream() {
        if (!stream_ready) {
            hipError_t err = hipSetDevice(device);
            if (err != hipSuccess)
                return err;
            err = hipStreamCreate(&stream);
            if (err != hipSuccess)
                return err;
            stream_ready = true;
        }
        return hipSuccess;
    }

    /* grow-only buffer per role (the caching the reference's GPUEvaluator
     * declared but never implemented; kernels.hpp:176-178) */
    hipError_t ensure(Role r, size_t bytes, void **out) {
        if (cap[r] < bytes) {
            if (buf[r]) {
                (void)hipFree(buf[r]);
                buf[r] = nullptr;
                cap[r] = 0;
            }
            hipError_t err = hipMalloc(&buf[r], bytes);
            if (err != hipSuccess)
                return err;
            cap[r] = bytes;
        }
        *out = buf[r];
        return hipSuccess;
    }

    void release() {
        for (auto &b : buf) {
            if (b)
                (void)hipFree(b);
            b = nullptr;
        }
        for (auto &c : cap)
            c = 0;
        if (stream_ready) {
            /* the launch workspace cached for this stream goes with it */
            (void)hipStreamSynchronize(stream);
            skelly::release_persistent_ws(stream);
            (void)hipStreamDestroy(stream);
            stream_ready = false;
        }
    }
};

Context &ctx() {
    static Context c;
    return c;
}

#define CHK(where, call)                                                                           \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            set_error(where, _e);                                                                  \
            return -1;                                                                             \
        }                                                                                          \
    } while (0)

/* Device-pointer form of one pair kernel: launch on the caller's stream, no
 * synchronization. scale is the kernel's prefactor as the entry point computed
 * it; reg and eps reach the regularized kernels only. */
int pair_device(const char *where, PairKernel kernel, const double *d_r_src,
                const double *d_f_src, long long n_src, const double *d_r_trg, double *d_out,
                long long n_trg, double scale, double reg, double eps, void *stream) {
    if (negative_size(where, n_src, n_trg))
        return -1;
    CHK(where, skelly::launch_pair_kernel(kernel, d_r_src, d_f_src, d_r_trg, d_out, n_src, n_trg,
                                          scale, reg, eps, (hipStream_t)stream));
    return 0;
}

/* Host-pointer form: upload, launch, download, sync on the library's stream.
 * The kernel's own widths size the buffers (doubles per source of f_src, per
 * target of out: 3 velocity components, 9 of a gradient, 1 pressure). */
int pair_host(const char *where, PairKernel kernel, const double *r_src, const double *f_src,
              long long n_src, const double *r_trg, double *out, long long n_trg, double scale,
              double reg, double eps) {
    if (negative_size(where, n_src, n_trg))
        return -1;
    if (n_trg == 0)
        return 0;
    const skelly::PairDims dims = skelly::pair_kernel_dims(kernel);
    const size_t src_row = (size_t)dims.srcdim * 8, out_row = (size_t)dims.outdim * 8;
    Context &c = ctx();
    std::lock_guard<std::mutex> lock(c.mu);
    CHK(where, c.ensure_stream());
    double *d_rs = nullptr, *d_fs = nullptr, *d_rt = nullptr, *d_u = nullptr;
    /* hipMalloc(0) quirks avoided: allocate at least 8 bytes */
    CHK(where, c.ensure(Context::R_SRC, (size_t)(n_src ? n_src : 1) * 3 * 8, (void **)&d_rs));
    CHK(where, c.ensure(Context::F_SRC, (size_t)(n_src ? n_src : 1) * src_row, (void **)&d_fs));
    CHK(where, c.ensure(Context::R_TRG, (size_t)n_trg * 3 * 8, (void **)&d_rt));
    CHK(where, c.ensure(Context::U_TRG, (size_t)n_trg * out_row, (void **)&d_u));
    if (n_src) {
        CHK(where, hipMemcpyAsync(d_rs, r_src, (size_t)n_src * 3 * 8, hipMemcpyHostToDevice,
                                  c.stream));
        CHK(where, hipMemcpyAsync(d_fs, f_src, (size_t)n_src * src_row, hipMemcpyHostToDevice,
                                  c.stream));
    }
    CHK(where, hipMemcpyAsync(d_rt, r_trg, (size_t)n_trg * 3 * 8, hipMemcpyHostToDevice, c.stream));
    CHK(where, skelly::launch_pair_kernel(kernel, d_rs, d_fs, d_rt, d_u, n_src, n_trg, scale, reg,
                                          eps, c.stream));
    CHK(where, hipMemcpyAsync(out, d_u, (size_t)n_trg * out_row, hipMemcpyDeviceToHost, c.stream));
    CHK(where, hipStreamSynchronize(c.stream));
    return 0;
}

/* The two ways the reference writes the prefactor; they differ in the last
 * bit for general eta, so each entry point keeps the one it always used. */
double scale_stokes(double eta) { return kOneOver8Pi / eta; }          /* kernels.cu:59 */
double scale_oseen(double eta) { return 1.0 / (8.0 * M_PI * eta); }    /* kernels.cpp:94,213 */

/* The arguments of a field-line entry point as the launcher's request (of
 * streamlines, or of vortex lines with `vorticity`), after the check that
 * comes before any HIP call. True (message recorded) when a count is negative.
 * Each entry point names its 33 arguments here, once. */
bool trace_request(const char *where, int vorticity, skelly::TraceRequest &q, const double *sl_r,
                   const double *sl_f, long long n_sl, const double *dl_r, const double *dl_f,
                   long long n_dl, const double *rot_r, const double *rot_f, long long n_rot,
                   const double *os_r, const double *os_f, long long n_os,
                   const double *background, const double *bodies, long long n_bodies,
                   const double *seeds, long long n_seeds, int back_integrate, double eta,
                   double reg, double eps, double dt_init, double t_final, double abs_err,
                   double rel_err, long long max_points, double *x, double *t, double *val,
                   int *count, int *status) {
    if (negative_size(where, n_sl, n_dl) || negative_size(where, n_rot, n_os) ||
        negative_size(where, n_bodies, n_seeds) || negative_size(where, max_points))
        return true;
    q = skelly::TraceRequest{};
    q.vorticity = vorticity;
    const double *r[4] = {sl_r, dl_r, rot_r, os_r}, *f[4] = {sl_f, dl_f, rot_f, os_f};
    const long long n[4] = {n_sl, n_dl, n_rot, n_os};
    for (int k = 0; k < 4; ++k) {
        q.r[k] = r[k];
        q.f[k] = f[k];
        q.n[k] = n[k];
    }
    q.scale_stokes = scale_stokes(eta);
    q.scale_oseen = scale_oseen(eta);
    q.reg = reg;
    q.eps = eps;
    if (n_seeds == 0)
        background = nullptr; /* nothing is read for a call that does nothing */
    for (int j = 0; j < 3; ++j) {
        q.uniform[j] = background ? background[j] : 0.0;
        q.bg_scale[j] = background ? background[3 + j] : 0.0;
        q.components[j] = background ? (int)background[6 + j] : j;
    }
    q.bodies = bodies;
    q.n_bodies = n_bodies;
    q.seeds = seeds;
    q.n_seeds = n_seeds;
    q.back_integrate = back_integrate;
    q.dt_init = dt_init;
    q.t_final = t_final;
    q.abs_err = abs_err;
    q.rel_err = rel_err;
    q.max_points = max_points;
    q.x = x;
    q.t = t;
    q.val = val;
    q.count = count;
    q.status = status;
    return false;
}

} // namespace

extern "C" {

const char *skelly_hip_version(void) { return "skelly-hip 0.1.0 gfx950"; }

const char *skelly_hip_last_error(void) { return g_last_error.c_str(); }

int skelly_hip_device_count(void) {
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    if (err != hipSuccess) {
        set_error("device_count", err);
        return -1;
    }
    return n;
}

int skelly_hip_set_device(int device) {
    Context &c = ctx();
    std::lock_guard<std::mutex> lock(c.mu);
    if (device != c.device) {
        c.release();
        c.device = device;
    }
    CHK("set_device", hipSetDevice(device));
    return 0;
}

int skelly_hip_shutdown(void) {
    Context &c = ctx();
    std::lock_guard<std::mutex> lock(c.mu);
    c.release();
    return 0;
}

/* ---- reference drop-in entry points (scale 1/(8*pi), no eta) ---- */

void stokeslet_direct_gpu_impl(const double *r_src, const double *f_src, int n_src,
                               const double *r_trg, double *u_trg, int n_trg) {
    (void)pair_host("stokeslet_direct_gpu_impl", PairKernel::Stokeslet, r_src, f_src, n_src,
                    r_trg, u_trg, n_trg, kOneOver8Pi, 0.0, 0.0);
}

void stresslet_direct_gpu_impl(const double *r_src, const double *f_src, int n_src,
                               const double *r_trg, double *u_trg, int n_trg) {
    (void)pair_host("stresslet_direct_gpu_impl", PairKernel::Stresslet, r_src, f_src, n_src,
                    r_trg, u_trg, n_trg, kOneOver8Pi, 0.0, 0.0);
}

/* ---- extended host-pointer API (fully scaled) ---- */

int skelly_stokeslet_host(const double *r_src, const double *f_src, long long n_src,
                          const double *r_trg, double *u_trg, long long n_trg, double eta) {
    return pair_host("skelly_stokeslet_host", PairKernel::Stokeslet, r_src, f_src, n_src, r_trg,
                     u_trg, n_trg, scale_stokes(eta), 0.0, 0.0);
}

int skelly_stresslet_host(const double *r_src, const double *f_src, long long n_src,
                          const double *r_trg, double *u_trg, long long n_trg, double eta) {
    return pair_host("skelly_stresslet_host", PairKernel::Stresslet, r_src, f_src, n_src, r_trg,
                     u_trg, n_trg, scale_stokes(eta), 0.0, 0.0);
}

int skelly_oseen_contract_host(const double *r_src, const double *r_trg, const double *density,
                               double *u_trg, long long n_src, long long n_trg, double eta,
                               double reg, double epsilon_distance) {
    return pair_host("skelly_oseen_contract_host", PairKernel::OseenContract, r_src, density,
                     n_src, r_trg, u_trg, n_trg, scale_oseen(eta), reg, epsilon_distance);
}

int skelly_rotlet_host(const double *r_src, const double *r_trg, const double *density,
                       double *u_trg, long long n_src, long long n_trg, double eta, double reg,
                       double epsilon_distance) {
    return pair_host("skelly_rotlet_host", PairKernel::Rotlet, r_src, density, n_src, r_trg,
                     u_trg, n_trg, scale_oseen(eta), reg, epsilon_distance);
}

/* ---- device-pointer API (async on caller's stream) ---- */

int skelly_stokeslet_device(const double *d_r_src, const double *d_f_src, long long n_src,
                            const double *d_r_trg, double *d_u_trg, long long n_trg, double eta,
                            void *stream) {
    return pair_device("skelly_stokeslet_device", PairKernel::Stokeslet, d_r_src, d_f_src, n_src,
                       d_r_trg, d_u_trg, n_trg, scale_stokes(eta), 0.0, 0.0, stream);
}

int skelly_stresslet_device(const double *d_r_src, const double *d_f_src, long long n_src,
                            const double *d_r_trg, double *d_u_trg, long long n_trg, double eta,
                            void *stream) {
    return pair_device("skelly_stresslet_device", PairKernel::Stresslet, d_r_src, d_f_src, n_src,
                       d_r_trg, d_u_trg, n_trg, scale_stokes(eta), 0.0, 0.0, stream);
}

int skelly_oseen_contract_device(const double *d_r_src, const double *d_r_trg,
                                 const double *d_density, double *d_u_trg, long long n_src,
                                 long long n_trg, double eta, double reg, double epsilon_distance,
                                 void *stream) {
    return pair_device("skelly_oseen_contract_device", PairKernel::OseenContract, d_r_src,
                       d_density, n_src, d_r_trg, d_u_trg, n_trg, scale_oseen(eta), reg,
                       epsilon_distance, stream);
}

int skelly_rotlet_device(const double *d_r_src, const double *d_r_trg, const double *d_density,
                         double *d_u_trg, long long n_src, long long n_trg, double eta, double reg,
                         double epsilon_distance, void *stream) {
    return pair_device("skelly_rotlet_device", PairKernel::Rotlet, d_r_src, d_density, n_src,
                       d_r_trg, d_u_trg, n_trg, scale_oseen(eta), reg, epsilon_distance, stream);
}

/* ---- velocity gradients: 9 doubles per target, G[i][j] at 9*it + 3*i + j ----
 * The oseen forms run StokesletGrad with the regularization switched on. */

int skelly_stokeslet_grad_host(const double *r_src, const double *f_src, long long n_src,
                               const double *r_trg, double *g_trg, long long n_trg, double eta) {
    return pair_host("skelly_stokeslet_grad_host", PairKernel::StokesletGrad, r_src, f_src, n_src,
                     r_trg, g_trg, n_trg, scale_stokes(eta), 0.0, 0.0);
}

int skelly_stresslet_grad_host(const double *r_src, const double *f_src, long long n_src,
                               const double *r_trg, double *g_trg, long long n_trg, double eta) {
    return pair_host("skelly_stresslet_grad_host", PairKernel::StressletGrad, r_src, f_src, n_src,
                     r_trg, g_trg, n_trg, scale_stokes(eta), 0.0, 0.0);
}

int skelly_oseen_contract_grad_host(const double *r_src, const double *r_trg,
                                    const double *density, double *g_trg, long long n_src,
                                    long long n_trg, double eta, double reg,
                                    double epsilon_distance) {
    return pair_host("skelly_oseen_contract_grad_host", PairKernel::StokesletGrad, r_src, density,
                     n_src, r_trg, g_trg, n_trg, scale_oseen(eta), reg, epsilon_distance);
}

int skelly_rotlet_grad_host(const double *r_src, const double *r_trg, const double *density,
                            double *g_trg, long long n_src, long long n_trg, double eta,
                            double reg, double epsilon_distance) {
    return pair_host("skelly_rotlet_grad_host", PairKernel::RotletGrad, r_src, density, n_src,
                     r_trg, g_trg, n_trg, scale_oseen(eta), reg, epsilon_distance);
}

int skelly_stokeslet_grad_device(const double *d_r_src, const double *d_f_src, long long n_src,
                                 const double *d_r_trg, double *d_g_trg, long long n_trg,
                                 double eta, void *stream) {
    return pair_device("skelly_stokeslet_grad_device", PairKernel::StokesletGrad, d_r_src,
                       d_f_src, n_src, d_r_trg, d_g_trg, n_trg, scale_stokes(eta), 0.0, 0.0,
                       stream);
}

int skelly_stresslet_grad_device(const double *d_r_src, const double *d_f_src, long long n_src,
                                 const double *d_r_trg, double *d_g_trg, long long n_trg,
                                 double eta, void *stream) {
    return pair_device("skelly_stresslet_grad_device", PairKernel::StressletGrad, d_r_src,
                       d_f_src, n_src, d_r_trg, d_g_trg, n_trg, scale_stokes(eta), 0.0, 0.0,
                       stream);
}

int skelly_oseen_contract_grad_device(const double *d_r_src, const double *d_r_trg,
                                      const double *d_density, double *d_g_trg, long long n_src,
                                      long long n_trg, double eta, double reg,
                                      double epsilon_distance, void *stream) {
    return pair_device("skelly_oseen_contract_grad_device", PairKernel::StokesletGrad, d_r_src,
                       d_density, n_src, d_r_trg, d_g_trg, n_trg, scale_oseen(eta), reg,
                       epsilon_distance, stream);
}

int skelly_rotlet_grad_device(const double *d_r_src, const double *d_r_trg,
                              const double *d_density, double *d_g_trg, long long n_src,
                              long long n_trg, double eta, double reg, double epsilon_distance,
                              void *stream) {
    return pair_device("skelly_rotlet_grad_device", PairKernel::RotletGrad, d_r_src, d_density,
                       n_src, d_r_trg, d_g_trg, n_trg, scale_oseen(eta), reg, epsilon_distance,
                       stream);
}

/* ---- pressures: 1 double per target, prefactor 1/(4*pi), no eta ----
 * The oseen forms run StokesletPressure with the regularization switched on;
 * the rotlet's pressure is zero and has no entry point. */

int skelly_stokeslet_pressure_host(const double *r_src, const double *f_src, long long n_src,
                                   const double *r_trg, double *p_trg, long long n_trg) {
    return pair_host("skelly_stokeslet_pressure_host", PairKernel::StokesletPressure, r_src,
                     f_src, n_src, r_trg, p_trg, n_trg, kOneOver4Pi, 0.0, 0.0);
}

int skelly_stresslet_pressure_host(const double *r_src, const double *f_src, long long n_src,
                                   const double *r_trg, double *p_trg, long long n_trg) {
    return pair_host("skelly_stresslet_pressure_host", PairKernel::StressletPressure, r_src,
                     f_src, n_src, r_trg, p_trg, n_trg, kOneOver4Pi, 0.0, 0.0);
}

int skelly_oseen_contract_pressure_host(const double *r_src, const double *r_trg,
                                        const double *density, double *p_trg, long long n_src,
                                        long long n_trg, double reg, double epsilon_distance) {
    return pair_host("skelly_oseen_contract_pressure_host", PairKernel::StokesletPressure, r_src,
                     density, n_src, r_trg, p_trg, n_trg, kOneOver4Pi, reg, epsilon_distance);
}

int skelly_stokeslet_pressure_device(const double *d_r_src, const double *d_f_src,
                                     long long n_src, const double *d_r_trg, double *d_p_trg,
                                     long long n_trg, void *stream) {
    return pair_device("skelly_stokeslet_pressure_device", PairKernel::StokesletPressure, d_r_src,
                       d_f_src, n_src, d_r_trg, d_p_trg, n_trg, kOneOver4Pi, 0.0, 0.0, stream);
}

int skelly_stresslet_pressure_device(const double *d_r_src, const double *d_f_src,
                                     long long n_src, const double *d_r_trg, double *d_p_trg,
                                     long long n_trg, void *stream) {
    return pair_device("skelly_stresslet_pressure_device", PairKernel::StressletPressure, d_r_src,
                       d_f_src, n_src, d_r_trg, d_p_trg, n_trg, kOneOver4Pi, 0.0, 0.0, stream);
}

int skelly_oseen_contract_pressure_device(const double *d_r_src, const double *d_r_trg,
                                          const double *d_density, double *d_p_trg,
                                          long long n_src, long long n_trg, double reg,
                                          double epsilon_distance, void *stream) {
    return pair_device("skelly_oseen_contract_pressure_device", PairKernel::StokesletPressure,
                       d_r_src, d_density, n_src, d_r_trg, d_p_trg, n_trg, kOneOver4Pi, reg,
                       epsilon_distance, stream);
}

/* ---- nearest source: d2 and index per target (launch_nearest) ---- */

int skelly_nearest_device(const double *d_r_src, const long long *d_src_group, long long n_src,
                          const double *d_r_trg, const long long *d_trg_group, long long n_trg,
                          double *d_d2, long long *d_index, void *stream) {
    const char *where = "skelly_nearest_device";
    if (negative_size(where, n_src, n_trg) || lone_group(where, d_src_group, d_trg_group))
        return -1;
    CHK(where, skelly::launch_nearest(d_r_src, d_src_group, n_src, d_r_trg, d_trg_group, n_trg,
                                      d_d2, d_index, (hipStream_t)stream));
    return 0;
}

/* Host form: one block for the call (inputs, then d2 and index), upload,
 * launch, download, sync on the library's stream. */
int skelly_nearest_host(const double *r_src, const long long *src_group, long long n_src,
                        const double *r_trg, const long long *trg_group, long long n_trg,
                        double *d2, long long *index) {
    const char *where = "skelly_nearest_host";
    if (negative_size(where, n_src, n_trg) || lone_group(where, src_group, trg_group))
        return -1;
    if (n_trg == 0)
        return 0;
    const bool grouped = src_group != nullptr;
    const size_t ns = (size_t)n_src, nt = (size_t)n_trg;
    /* all items are 8 bytes wide */
    const size_t words = ns * 3 + nt * 3 + (grouped ? ns + nt : 0) + nt * 2;
    Context &c = ctx();
    std::lock_guard<std::mutex> lock(c.mu);
    CHK(where, c.ensure_stream());
    double *block = nullptr;
    CHK(where, hipMalloc((void **)&block, words * 8));
    /* everything below frees the block on its way out */
    hipError_t err = hipSuccess;
    double *at = block;
    auto upload = [&](const void *p, size_t n) {
        double *dst = at;
        if (n && err == hipSuccess)
            err = hipMemcpyAsync(dst, p, n * 8, hipMemcpyHostToDevice, c.stream);
        at += n;
        return dst;
    };
    const double *d_rs = upload(r_src, ns * 3);
    const double *d_rt = upload(r_trg, nt * 3);
    const long long *d_sg = nullptr, *d_tg = nullptr;
    if (grouped) {
        d_sg = reinterpret_cast<const long long *>(upload(src_group, ns));
        d_tg = reinterpret_cast<const long long *>(upload(trg_group, nt));
    }
    double *d_d2 = at;
    long long *d_index = reinterpret_cast<long long *>(at + nt);
    if (err == hipSuccess)
        err = skelly::launch_nearest(d_rs, d_sg, n_src, d_rt, d_tg, n_trg, d_d2, d_index,
                                     c.stream);
    if (err == hipSuccess)
        err = hipMemcpyAsync(d2, d_d2, nt * 8, hipMemcpyDeviceToHost, c.stream);
    if (err == hipSuccess)
        err = hipMemcpyAsync(index, d_index, nt * 8, hipMemcpyDeviceToHost, c.stream);
    const hipError_t sync = hipStreamSynchronize(c.stream);
    (void)hipFree(block);
    CHK(where, err);
    CHK(where, sync);
    return 0;
}

/* stresslet x normal x density: the prefactor -3/(4*pi) is the functor's own
 * (no eta), so the scale argument is not read. */

int skelly_stresslet_normal_density_host(const double *r_src, const double *normals,
                                         const double *density, double *out, long long n,
                                         double reg, double epsilon_distance) {
    if (negative_size("skelly_stresslet_normal_density_host", n))
        return -1;
    /* interleave [normal | density] into the (n, 6) source-strength array */
    std::vector<double> nd((size_t)n * 6);
    for (long long i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) {
            nd[6 * i + k] = normals[3 * i + k];
            nd[6 * i + 3 + k] = density[3 * i + k];
        }
    }
    return pair_host("skelly_stresslet_normal_density_host", PairKernel::StressletNormalDensity,
                     r_src, nd.data(), n, r_src, out, n, 0.0, reg, epsilon_distance);
}

int skelly_stresslet_normal_density_device(const double *d_r_src, const double *d_nd,
                                           const double *d_r_trg, double *d_out, long long n_src,
                                           long long n_trg, double reg, double epsilon_distance,
                                           void *stream) {
    return pair_device("skelly_stresslet_normal_density_device",
                       PairKernel::StressletNormalDensity, d_r_src, d_nd, n_src, d_r_trg, d_out,
                       n_trg, 0.0, reg, epsilon_distance, stream);
}

int skelly_stresslet_times_normal_device(const double *d_pts, const double *d_normals,
                                         double *d_out, long long n, double reg,
                                         double epsilon_distance, void *stream) {
    if (negative_size("skelly_stresslet_times_normal_device", n))
        return -1;
    CHK("skelly_stresslet_times_normal_device",
        skelly::launch_stresslet_times_normal(d_pts, d_normals, d_out, n, reg,
                                              epsilon_distance, (hipStream_t)stream));
    return 0;
}

int skelly_oseen_tensor_batched_device(const double *d_pts, double *d_G, long long nf,
                                       long long n, double eta, double reg,
                                       double epsilon_distance, void *stream) {
    if (negative_size("skelly_oseen_tensor_batched_device", nf, n))
        return -1;
    CHK("skelly_oseen_tensor_batched_device",
        skelly::launch_oseen_tensor_batched(d_pts, d_G, nf, n, eta, reg, epsilon_distance,
                                            (hipStream_t)stream));
    return 0;
}

} /* extern "C" */

/* ---- streamlines and vortex lines ----
 * One body for each form, shared by the two fields (TraceRequest::vorticity);
 * the entry points below differ in the name they report and the field. */

namespace {

/* Device form: q as trace_request() made it, launched on the caller's stream. */
int trace_device(const char *where, const skelly::TraceRequest &q, void *stream) {
    if (q.n_seeds == 0)
        return 0;
    CHK(where, skelly::launch_trace_streamlines(q, (hipStream_t)stream));
    return 0;
}

/* Host form: q's inputs are host arrays and x, t, val, count, status the
 * caller's outputs; upload, launch, download, sync on the library's stream. */
int trace_host(const char *where, skelly::TraceRequest q, double *x, double *t, double *val,
               int *count, int *status) {
    if (q.n_seeds == 0)
        return 0;
    const size_t n_jobs = (size_t)q.n_seeds * (q.back_integrate ? 2 : 1);
    const size_t rows = n_jobs * (size_t)q.max_points;
    /* one block for the call: the inputs, then x, val, t, count, status */
    const int width[4] = {3, 9, 3, 3};
    size_t in_doubles = (size_t)q.n_bodies * 10 + (size_t)q.n_seeds * 3;
    for (int k = 0; k < 4; ++k)
        in_doubles += (size_t)q.n[k] * (3 + width[k]);
    const size_t bytes = (in_doubles + rows * 7) * 8 + n_jobs * 2 * sizeof(int);

    Context &c = ctx();
    std::lock_guard<std::mutex> lock(c.mu);
    CHK(where, c.ensure_stream());
    double *block = nullptr;
    CHK(where, hipMalloc((void **)&block, bytes));
    /* everything below frees the block on its way out */
    hipError_t err = hipSuccess;
    double *at = block;
    auto upload = [&](const double *&p, size_t doubles) {
        if (doubles && err == hipSuccess)
            err = hipMemcpyAsync(at, p, doubles * 8, hipMemcpyHostToDevice, c.stream);
        p = at;
        at += doubles;
    };
    for (int k = 0; k < 4; ++k) {
        upload(q.r[k], (size_t)q.n[k] * 3);
        upload(q.f[k], (size_t)q.n[k] * width[k]);
    }
    upload(q.bodies, (size_t)q.n_bodies * 10);
    upload(q.seeds, (size_t)q.n_seeds * 3);
    q.x = at;
    q.val = q.x + rows * 3;
    q.t = q.val + rows * 3;
    q.count = reinterpret_cast<int *>(q.t + rows);
    q.status = q.count + n_jobs;
    if (err == hipSuccess)
        err = skelly::launch_trace_streamlines(q, c.stream);
    if (err == hipSuccess)
        err = hipMemcpyAsync(x, q.x, rows * 3 * 8, hipMemcpyDeviceToHost, c.stream);
    if (err == hipSuccess)
        err = hipMemcpyAsync(val, q.val, rows * 3 * 8, hipMemcpyDeviceToHost, c.stream);
    if (err == hipSuccess)
        err = hipMemcpyAsync(t, q.t, rows * 8, hipMemcpyDeviceToHost, c.stream);
    if (err == hipSuccess)
        err = hipMemcpyAsync(count, q.count, n_jobs * sizeof(int), hipMemcpyDeviceToHost,
                             c.stream);
    if (err == hipSuccess)
        err = hipMemcpyAsync(status, q.status, n_jobs * sizeof(int), hipMemcpyDeviceToHost,
                             c.stream);
    const hipError_t sync = hipStreamSynchronize(c.stream);
    (void)hipFree(block);
    CHK(where, err);
    CHK(where, sync);
    return 0;
}

} // namespace

extern "C" {

int skelly_trace_streamlines_device(
    const double *d_sl_r, const double *d_sl_f, long long n_sl, const double *d_dl_r,
    const double *d_dl_f, long long n_dl, const double *d_rot_r, const double *d_rot_f,
    long long n_rot, const double *d_os_r, const double *d_os_f, long long n_os,
    const double *background, const double *d_bodies, long long n_bodies, const double *d_seeds,
    long long n_seeds, int back_integrate, double eta, double reg, double epsilon_distance,
    double dt_init, double t_final, double abs_err, double rel_err, long long max_points,
    double *d_x, double *d_t, double *d_val, int *d_count, int *d_status, void *stream) {
    const char *where = "skelly_trace_streamlines_device";
    skelly::TraceRequest q;
    if (trace_request(where, 0, q, d_sl_r, d_sl_f, n_sl, d_dl_r, d_dl_f, n_dl, d_rot_r, d_rot_f,
                      n_rot, d_os_r, d_os_f, n_os, background, d_bodies, n_bodies, d_seeds,
                      n_seeds, back_integrate, eta, reg, epsilon_distance, dt_init, t_final,
                      abs_err, rel_err, max_points, d_x, d_t, d_val, d_count, d_status))
        return -1;
    return trace_device(where, q, stream);
}

int skelly_trace_streamlines_host(
    const double *sl_r, const double *sl_f, long long n_sl, const double *dl_r, const double *dl_f,
    long long n_dl, const double *rot_r, const double *rot_f, long long n_rot, const double *os_r,
    const double *os_f, long long n_os, const double *background, const double *bodies,
    long long n_bodies, const double *seeds, long long n_seeds, int back_integrate, double eta,
    double reg, double epsilon_distance, double dt_init, double t_final, double abs_err,
    double rel_err, long long max_points, double *x, double *t, double *val, int *count,
    int *status) {
    const char *where = "skelly_trace_streamlines_host";
    skelly::TraceRequest q;
    if (trace_request(where, 0, q, sl_r, sl_f, n_sl, dl_r, dl_f, n_dl, rot_r, rot_f, n_rot, os_r,
                      os_f, n_os, background, bodies, n_bodies, seeds, n_seeds, back_integrate,
                      eta, reg, epsilon_distance, dt_init, t_final, abs_err, rel_err, max_points,
                      x, t, val, count, status))
        return -1;
    return trace_host(where, q, x, t, val, count, status);
}

int skelly_trace_vortexlines_device(
    const double *d_sl_r, const double *d_sl_f, long long n_sl, const double *d_dl_r,
    const double *d_dl_f, long long n_dl, const double *d_rot_r, const double *d_rot_f,
    long long n_rot, const double *d_os_r, const double *d_os_f, long long n_os,
    const double *background, const double *d_bodies, long long n_bodies, const double *d_seeds,
    long long n_seeds, int back_integrate, double eta, double reg, double epsilon_distance,
    double dt_init, double t_final, double abs_err, double rel_err, long long max_points,
    double *d_x, double *d_t, double *d_val, int *d_count, int *d_status, void *stream) {
    const char *where = "skelly_trace_vortexlines_device";
    skelly::TraceRequest q;
    if (trace_request(where, 1, q, d_sl_r, d_sl_f, n_sl, d_dl_r, d_dl_f, n_dl, d_rot_r, d_rot_f,
                      n_rot, d_os_r, d_os_f, n_os, background, d_bodies, n_bodies, d_seeds,
                      n_seeds, back_integrate, eta, reg, epsilon_distance, dt_init, t_final,
                      abs_err, rel_err, max_points, d_x, d_t, d_val, d_count, d_status))
        return -1;
    return trace_device(where, q, stream);
}

int skelly_trace_vortexlines_host(
    const double *sl_r, const double *sl_f, long long n_sl, const double *dl_r, const double *dl_f,
    long long n_dl, const double *rot_r, const double *rot_f, long long n_rot, const double *os_r,
    const double *os_f, long long n_os, const double *background, const double *bodies,
    long long n_bodies, const double *seeds, long long n_seeds, int back_integrate, double eta,
    double reg, double epsilon_distance, double dt_init, double t_final, double abs_err,
    double rel_err, long long max_points, double *x, double *t, double *val, int *count,
    int *status) {
    const char *where = "skelly_trace_vortexlines_host";
    skelly::TraceRequest q;
    if (trace_request(where, 1, q, sl_r, sl_f, n_sl, dl_r, dl_f, n_dl, rot_r, rot_f, n_rot, os_r,
                      os_f, n_os, background, bodies, n_bodies, seeds, n_seeds, back_integrate,
                      eta, reg, epsilon_distance, dt_init, t_final, abs_err, rel_err, max_points,
                      x, t, val, count, status))
        return -1;
    return trace_host(where, q, x, t, val, count, status);
}

int skelly_trace_block_size(void) { return skelly::trace_block_size(); }

int skelly_fp64_peak_tflops(double *out_tflops) {
    Context &c = ctx();
    std::lock_guard<std::mutex> lock(c.mu);
    CHK("fp64_peak", c.ensure_stream());
    CHK("fp64_peak", skelly::run_fp64_peak(out_tflops));
    return 0;
}

int skelly_issue_cost_probe(double *out3) {
    Context &c = ctx();
    std::lock_guard<std::mutex> lock(c.mu);
    CHK("issue_cost_probe", c.ensure_stream());
    CHK("issue_cost_probe", skelly::run_issue_cost_probe(out3));
    return 0;
}

int skelly_rsq_accuracy_probe(const double *d_x, double *d_seed, double *d_refined, long long n,
                              void *stream) {
    CHK("skelly_rsq_accuracy_probe",
        skelly::launch_rsq_probe(d_x, d_seed, d_refined, n, (hipStream_t)stream));
    return 0;
}

} /* extern "C" */
