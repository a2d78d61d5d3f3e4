/* skelly_evaluator.hpp — C++ host-side mirror of SkellySim's evaluator API.
 *
 * Header-only. Mirrors the kernels:: evaluator functions the reference host
 * code calls (flatironinstitute/SkellySim include/kernels.hpp:22-51) on top
 * of the C-ABI in skelly_hip.h, so a C++ harness (or the reference itself,
 * see INTEGRATION.md) can call the MI355X engine with the same call shapes.
 *
 * The reference types these signatures with Eigen::MatrixXd / CMatrixRef
 * (col-major fp64, 3 x n, per-point xyz contiguous). Eigen is not vendored
 * here, so the mirror uses a minimal col-major view/owning matrix with the
 * identical memory layout; an Eigen-typed caller binds by pointer+shape
 * (see INTEGRATION.md for the two-line adapters).
 *
 * Semantics mirrored exactly:
 *  - stokeslet consumers pass sources in (r_sl, f_sl) with r_dl/f_dl empty,
 *    stresslet consumers the reverse (kernel_test.cpp:40,65);
 *  - results are 3 x n_trg, already divided by eta (kernels.cpp:358,365);
 *  - oseen/rotlet defaults reg=5e-3, epsilon_distance=1e-5
 *    (kernels.hpp:34-35,44-45).
 */

#ifndef SKELLY_EVALUATOR_HPP
#define SKELLY_EVALUATOR_HPP

#include "skelly_hip.h"

#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

namespace skelly {

/* Minimal col-major fp64 matrix (rows x cols), layout-compatible with the
 * reference's Eigen::MatrixXd. */
class MatrixXd {
  public:
    MatrixXd() = default;
    MatrixXd(long rows, long cols) : rows_(rows), cols_(cols), data_(rows * cols, 0.0) {}
    static MatrixXd Zero(long rows, long cols) { return MatrixXd(rows, cols); }

    long rows() const { return rows_; }
    long cols() const { return cols_; }
    long size() const { return rows_ * cols_; }
    double *data() { return data_.data(); }
    const double *data() const { return data_.data(); }
    double &operator()(long i, long j) { return data_[j * rows_ + i]; }
    double operator()(long i, long j) const { return data_[j * rows_ + i]; }

  private:
    long rows_ = 0, cols_ = 0;
    std::vector<double> data_;
};

/* Read-only view (what the reference calls CMatrixRef). Binds a MatrixXd or
 * any col-major buffer (e.g. an Eigen matrix's data()). */
struct CMatrixRef {
    const double *ptr = nullptr;
    long rows = 0, cols = 0;
    CMatrixRef() = default;
    CMatrixRef(const MatrixXd &m) : ptr(m.data()), rows(m.rows()), cols(m.cols()) {}
    CMatrixRef(const double *p, long r, long c) : ptr(p), rows(r), cols(c) {}
    long size() const { return rows * cols; }
};

/* kernels::Evaluator (reference include/kernels.hpp:14-15). */
using Evaluator = std::function<MatrixXd(const CMatrixRef &r_sl, const CMatrixRef &r_dl,
                                         const CMatrixRef &r_trg, const CMatrixRef &f_sl,
                                         const CMatrixRef &f_dl, double eta)>;

inline void check_rc(int rc, const char *what) {
    if (rc != 0)
        throw std::runtime_error(std::string(what) + ": " + skelly_hip_last_error());
}

/* Mirror of kernels::stokeslet_direct_gpu (kernels.cpp:361-366). */
inline MatrixXd stokeslet_direct_gpu(const CMatrixRef &r_sl, const CMatrixRef & /*r_dl*/,
                                     const CMatrixRef &r_trg, const CMatrixRef &f_sl,
                                     const CMatrixRef & /*f_dl*/, double eta) {
    MatrixXd u(3, r_trg.cols);
    check_rc(skelly_stokeslet_host(r_sl.ptr, f_sl.ptr, r_sl.cols, r_trg.ptr, u.data(),
                                   r_trg.cols, eta),
             "stokeslet_direct_gpu");
    return u;
}

/* Mirror of kernels::stresslet_direct_gpu (kernels.cpp:354-359). */
inline MatrixXd stresslet_direct_gpu(const CMatrixRef & /*r_sl*/, const CMatrixRef &r_dl,
                                     const CMatrixRef &r_trg, const CMatrixRef & /*f_sl*/,
                                     const CMatrixRef &f_dl, double eta) {
    MatrixXd u(3, r_trg.cols);
    check_rc(skelly_stresslet_host(r_dl.ptr, f_dl.ptr, r_dl.cols, r_trg.ptr, u.data(),
                                   r_trg.cols, eta),
             "stresslet_direct_gpu");
    return u;
}

/* Mirror of kernels::oseen_tensor_contract_direct (kernels.cpp:85-131). */
inline MatrixXd oseen_tensor_contract_direct(const CMatrixRef &r_src, const CMatrixRef &r_trg,
                                             const CMatrixRef &density, double eta,
                                             double reg = 5e-3,
                                             double epsilon_distance = 1e-5) {
    MatrixXd u(3, r_trg.size() / 3);
    check_rc(skelly_oseen_contract_host(r_src.ptr, r_trg.ptr, density.ptr, u.data(),
                                        r_src.size() / 3, r_trg.size() / 3, eta, reg,
                                        epsilon_distance),
             "oseen_tensor_contract_direct");
    return u;
}

/* Mirror of kernels::rotlet (kernels.cpp:206-242). */
inline MatrixXd rotlet(const CMatrixRef &r_src, const CMatrixRef &r_trg,
                       const CMatrixRef &density, double eta, double reg = 5e-3,
                       double epsilon_distance = 1e-5) {
    MatrixXd u(3, r_trg.size() / 3);
    check_rc(skelly_rotlet_host(r_src.ptr, r_trg.ptr, density.ptr, u.data(), r_src.size() / 3,
                                r_trg.size() / 3, eta, reg, epsilon_distance),
             "rotlet");
    return u;
}

/* Velocity gradients of the four fields above (no reference counterpart):
 * 9 x n_trg, column t holding G[i][j] = du_i/dx_j at target t in row-major
 * order (row 3*i + j), fully scaled like the velocities. */
inline MatrixXd stokeslet_grad(const CMatrixRef &r_src, const CMatrixRef &r_trg,
                               const CMatrixRef &f_src, double eta) {
    MatrixXd g(9, r_trg.size() / 3);
    check_rc(skelly_stokeslet_grad_host(r_src.ptr, f_src.ptr, r_src.size() / 3, r_trg.ptr,
                                        g.data(), r_trg.size() / 3, eta),
             "stokeslet_grad");
    return g;
}

inline MatrixXd stresslet_grad(const CMatrixRef &r_src, const CMatrixRef &r_trg,
                               const CMatrixRef &f_src, double eta) {
    MatrixXd g(9, r_trg.size() / 3);
    check_rc(skelly_stresslet_grad_host(r_src.ptr, f_src.ptr, r_src.size() / 3, r_trg.ptr,
                                        g.data(), r_trg.size() / 3, eta),
             "stresslet_grad");
    return g;
}

inline MatrixXd oseen_tensor_contract_grad(const CMatrixRef &r_src, const CMatrixRef &r_trg,
                                           const CMatrixRef &density, double eta,
                                           double reg = 5e-3, double epsilon_distance = 1e-5) {
    MatrixXd g(9, r_trg.size() / 3);
    check_rc(skelly_oseen_contract_grad_host(r_src.ptr, r_trg.ptr, density.ptr, g.data(),
                                             r_src.size() / 3, r_trg.size() / 3, eta, reg,
                                             epsilon_distance),
             "oseen_tensor_contract_grad");
    return g;
}

inline MatrixXd rotlet_grad(const CMatrixRef &r_src, const CMatrixRef &r_trg,
                            const CMatrixRef &density, double eta, double reg = 5e-3,
                            double epsilon_distance = 1e-5) {
    MatrixXd g(9, r_trg.size() / 3);
    check_rc(skelly_rotlet_grad_host(r_src.ptr, r_trg.ptr, density.ptr, g.data(),
                                     r_src.size() / 3, r_trg.size() / 3, eta, reg,
                                     epsilon_distance),
             "rotlet_grad");
    return g;
}

/* Pressures of the stokeslet, stresslet and oseen fields above (no reference
 * counterpart on the direct path): 1 x n_trg, prefactor 1/(4 pi), no eta (no
 * pressure depends on it). The rotlet's pressure is zero. */
inline MatrixXd stokeslet_pressure(const CMatrixRef &r_src, const CMatrixRef &r_trg,
                                   const CMatrixRef &f_src) {
    MatrixXd p(1, r_trg.size() / 3);
    check_rc(skelly_stokeslet_pressure_host(r_src.ptr, f_src.ptr, r_src.size() / 3, r_trg.ptr,
                                            p.data(), r_trg.size() / 3),
             "stokeslet_pressure");
    return p;
}

inline MatrixXd stresslet_pressure(const CMatrixRef &r_src, const CMatrixRef &r_trg,
                                   const CMatrixRef &f_src) {
    MatrixXd p(1, r_trg.size() / 3);
    check_rc(skelly_stresslet_pressure_host(r_src.ptr, f_src.ptr, r_src.size() / 3, r_trg.ptr,
                                            p.data(), r_trg.size() / 3),
             "stresslet_pressure");
    return p;
}

inline MatrixXd oseen_tensor_contract_pressure(const CMatrixRef &r_src, const CMatrixRef &r_trg,
                                               const CMatrixRef &density, double reg = 5e-3,
                                               double epsilon_distance = 1e-5) {
    MatrixXd p(1, r_trg.size() / 3);
    check_rc(skelly_oseen_contract_pressure_host(r_src.ptr, r_trg.ptr, density.ptr, p.data(),
                                                 r_src.size() / 3, r_trg.size() / 3, reg,
                                                 epsilon_distance),
             "oseen_tensor_contract_pressure");
    return p;
}

/* Nearest source (no reference counterpart; skelly_nearest_host): per column
 * of r_trg the squared distance to the nearest eligible column of r_src and
 * that column's index, the lowest among equals; +inf and -1 where there is
 * none. With groups (both vectors non-empty, one id per column) a source is
 * eligible when its id differs from the target's; with both empty every
 * source is. */
struct Nearest {
    std::vector<double> d2;
    std::vector<long long> index;
};

inline Nearest nearest(const CMatrixRef &r_src, const CMatrixRef &r_trg,
                       const std::vector<long long> &src_group = {},
                       const std::vector<long long> &trg_group = {}) {
    const long n_src = r_src.size() / 3, n_trg = r_trg.size() / 3;
    const bool grouped = !src_group.empty() || !trg_group.empty();
    if (grouped && ((long)src_group.size() != n_src || (long)trg_group.size() != n_trg))
        throw std::runtime_error("nearest: one group id per source and per target, or none");
    Nearest out;
    out.d2.resize(n_trg);
    out.index.resize(n_trg);
    /* an empty vector's data() may be null: a grouped call never passes it */
    static const long long none = 0;
    check_rc(skelly_nearest_host(r_src.ptr, grouped ? (n_src ? src_group.data() : &none) : nullptr,
                                 n_src, r_trg.ptr,
                                 grouped ? (n_trg ? trg_group.data() : &none) : nullptr, n_trg,
                                 out.d2.data(), out.index.data()),
             "nearest");
    return out;
}

/* Streamlines (mirror of StreamLine::compute, streamline.cpp:67-113, for all
 * seeds in one kernel launch; skelly_trace_streamlines_host). The field is the
 * sum of the four source sets of StreamlineField, each possibly empty, plus
 * the background and the rigid motion inside bodies. */
struct StreamlineField {
    CMatrixRef r_sl, f_sl;     /* Stokeslets: 3 x n, 3 x n */
    CMatrixRef r_dl, f_dl;     /* stresslets: 3 x n, 9 x n */
    CMatrixRef r_rot, torques; /* rotlets: 3 x n, 3 x n */
    CMatrixRef r_os, f_os;     /* regularized Stokeslets: 3 x n, 3 x n */
    bool has_background = false;
    double uniform[3] = {0, 0, 0}, scale_factor[3] = {0, 0, 0};
    int components[3] = {0, 1, 2};
    CMatrixRef bodies; /* 10 x n_bodies: centre, radius, velocity, angular velocity */
    double eta = 1.0, reg = 5e-3, epsilon_distance = 1e-5;
};

/* streamline.hpp:29, plus the tracer's status (skelly_hip.h: the larger of
 * the two directions' codes, 0 when both reached t_final). */
struct StreamLine {
    MatrixXd x, val; /* 3 x n_points */
    std::vector<double> time;
    int status = 0;
};

/* The two tracers' host entry points share one argument list. */
using TraceHostFn = decltype(&skelly_trace_streamlines_host);

/* One joined line per column of x0 (3 x n_seeds), traced by `entry`: the
 * backward path reversed and without the seed it shares, then the forward path
 * (join_back_and_forward, streamline.cpp:56-65). */
inline std::vector<StreamLine> trace_lines(TraceHostFn entry, const char *what,
                                           const StreamlineField &f, const CMatrixRef &x0,
                                           double dt_init, double t_final, double abs_err,
                                           double rel_err, bool back_integrate, long max_points) {
    const long n = x0.size() / 3, n_jobs = n * (back_integrate ? 2 : 1);
    std::vector<double> x(3 * n_jobs * max_points), val(3 * n_jobs * max_points),
        t(n_jobs * max_points);
    std::vector<int> count(n_jobs), status(n_jobs);
    const double background[9] = {f.uniform[0],      f.uniform[1],      f.uniform[2],
                                  f.scale_factor[0], f.scale_factor[1], f.scale_factor[2],
                                  (double)f.components[0], (double)f.components[1],
                                  (double)f.components[2]};
    check_rc(entry(
                 f.r_sl.ptr, f.f_sl.ptr, f.r_sl.size() / 3, f.r_dl.ptr, f.f_dl.ptr,
                 f.r_dl.size() / 3, f.r_rot.ptr, f.torques.ptr, f.r_rot.size() / 3, f.r_os.ptr,
                 f.f_os.ptr, f.r_os.size() / 3, f.has_background ? background : nullptr,
                 f.bodies.ptr, f.bodies.size() / 10, x0.ptr, n, back_integrate ? 1 : 0, f.eta,
                 f.reg, f.epsilon_distance, dt_init, t_final, abs_err, rel_err, max_points,
                 x.data(), t.data(), val.data(), count.data(), status.data()),
             what);
    std::vector<StreamLine> lines(n);
    for (long i = 0; i < n; ++i) {
        const long back = back_integrate ? count[n + i] - 1 : 0; /* without the seed */
        StreamLine &s = lines[i];
        s.x = MatrixXd(3, back + count[i]);
        s.val = MatrixXd(3, back + count[i]);
        s.time.resize(back + count[i]);
        s.status = back_integrate && status[n + i] > status[i] ? status[n + i] : status[i];
        for (long c = 0; c < back + count[i]; ++c) {
            /* row of the job arrays that is column c of the line */
            const long row = c < back ? (n + i) * max_points + (back - c)
                                      : i * max_points + (c - back);
            for (int j = 0; j < 3; ++j) {
                s.x(j, c) = x[3 * row + j];
                s.val(j, c) = val[3 * row + j];
            }
            s.time[c] = t[row];
        }
    }
    return lines;
}

inline std::vector<StreamLine> trace_streamlines(const StreamlineField &f, const CMatrixRef &x0,
                                                 double dt_init = 0.1, double t_final = 1.0,
                                                 double abs_err = 1e-10, double rel_err = 1e-6,
                                                 bool back_integrate = true,
                                                 long max_points = 4096) {
    return trace_lines(skelly_trace_streamlines_host, "trace_streamlines", f, x0, dt_init,
                       t_final, abs_err, rel_err, back_integrate, max_points);
}

/* Vortex lines (mirror of VortexLine::compute, streamline.cpp:115-165, with the
 * analytic curl of the gradient kernels in place of its finite difference;
 * skelly_trace_vortexlines_host): the lines of w = curl u of the same field,
 * val the vorticity at their points, 2 w_b inside a body. The |u| > 1e3 stop
 * (status 1) stays on the velocity, as the reference's observer has it. */
inline std::vector<StreamLine> trace_vortexlines(const StreamlineField &f, const CMatrixRef &x0,
                                                 double dt_init = 0.1, double t_final = 1.0,
                                                 double abs_err = 1e-10, double rel_err = 1e-6,
                                                 bool back_integrate = true,
                                                 long max_points = 4096) {
    return trace_lines(skelly_trace_vortexlines_host, "trace_vortexlines", f, x0, dt_init,
                       t_final, abs_err, rel_err, back_integrate, max_points);
}

/* Mirror of the reference's string-keyed backend selection
 * (fiber_container_base.cpp:20-33, periphery.cpp:337-352): "HIP" is this
 * engine; the reference's "CPU"/"FMM" backends are out of scope. */
inline Evaluator make_stokeslet_evaluator(const std::string &name) {
    if (name == "HIP" || name == "GPU")
        return stokeslet_direct_gpu;
    throw std::runtime_error("evaluator \"" + name + "\": only \"HIP\" is provided");
}

inline Evaluator make_stresslet_evaluator(const std::string &name) {
    if (name == "HIP" || name == "GPU")
        return stresslet_direct_gpu;
    throw std::runtime_error("evaluator \"" + name + "\": only \"HIP\" is provided");
}

} // namespace skelly

#endif /* SKELLY_EVALUATOR_HPP */
