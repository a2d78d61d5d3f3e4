// Stand-alone program for tests/test_gpu_cpp_mirror.py: every function of
// include/skelly_evaluator.hpp on one case, results written as they come back.
//
//   evaluator_probe CASE OUT
//
// CASE: int64 n_src, n_trg; double eta, reg, eps; then r_src (3 x n_src
// col-major, i.e. xyz per point), r_trg (3 x n_trg), f3 (3 x n_src) and f9
// (9 x n_src), raw doubles. OUT gets, as raw doubles in this order:
//   stokeslet_direct_gpu, stresslet_direct_gpu, oseen_tensor_contract_direct,
//   rotlet                                            (3 x n_trg each)
//   stokeslet_grad, stresslet_grad, oseen_tensor_contract_grad, rotlet_grad
//                                                     (9 x n_trg each)
//   make_stokeslet_evaluator("HIP"), make_stresslet_evaluator("GPU")
//                                                     (3 x n_trg each)
// Both factories have to throw for "FMM"; exit status 0 only if they did.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "skelly_evaluator.hpp"

namespace {

std::FILE *open_or_die(const char *path, const char *mode) {
    std::FILE *f = std::fopen(path, mode);
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    return f;
}

template <typename T>
void read_or_die(std::FILE *f, T *dst, size_t n) {
    if (std::fread(dst, sizeof(T), n, f) != n) {
        std::fprintf(stderr, "case file too short\n");
        std::exit(2);
    }
}

skelly::MatrixXd read_matrix(std::FILE *f, long rows, long cols) {
    skelly::MatrixXd m(rows, cols);
    read_or_die(f, m.data(), (size_t)m.size());
    return m;
}

template <typename Factory>
bool throws_for_fmm(Factory make, const char *what) {
    try {
        (void)make("FMM");
    } catch (const std::exception &e) {
        std::printf("%s(\"FMM\") threw: %s\n", what, e.what());
        return true;
    }
    std::fprintf(stderr, "%s(\"FMM\") did not throw\n", what);
    return false;
}

} // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s CASE OUT\n", argv[0]);
        return 2;
    }
    std::FILE *in = open_or_die(argv[1], "rb");
    std::int64_t n[2];
    double par[3];
    read_or_die(in, n, 2);
    read_or_die(in, par, 3);
    if (n[0] < 0 || n[1] < 0 || n[0] > (1 << 20) || n[1] > (1 << 20)) {
        std::fprintf(stderr, "counts out of range\n");
        return 2;
    }
    const long n_src = (long)n[0], n_trg = (long)n[1];
    const double eta = par[0], reg = par[1], eps = par[2];
    const skelly::MatrixXd r_src = read_matrix(in, 3, n_src), r_trg = read_matrix(in, 3, n_trg),
                           f3 = read_matrix(in, 3, n_src), f9 = read_matrix(in, 9, n_src);
    std::fclose(in);
    const skelly::MatrixXd none;

    try {
        const skelly::Evaluator stokeslet = skelly::make_stokeslet_evaluator("HIP");
        const skelly::Evaluator stresslet = skelly::make_stresslet_evaluator("GPU");
        const std::vector<skelly::MatrixXd> results = {
            skelly::stokeslet_direct_gpu(r_src, none, r_trg, f3, none, eta),
            skelly::stresslet_direct_gpu(none, r_src, r_trg, none, f9, eta),
            skelly::oseen_tensor_contract_direct(r_src, r_trg, f3, eta, reg, eps),
            skelly::rotlet(r_src, r_trg, f3, eta, reg, eps),
            skelly::stokeslet_grad(r_src, r_trg, f3, eta),
            skelly::stresslet_grad(r_src, r_trg, f9, eta),
            skelly::oseen_tensor_contract_grad(r_src, r_trg, f3, eta, reg, eps),
            skelly::rotlet_grad(r_src, r_trg, f3, eta, reg, eps),
            stokeslet(r_src, none, r_trg, f3, none, eta),
            stresslet(none, r_src, r_trg, none, f9, eta),
        };
        std::FILE *out = open_or_die(argv[2], "wb");
        for (const skelly::MatrixXd &m : results) {
            std::printf("result %ld x %ld\n", m.rows(), m.cols());
            if (std::fwrite(m.data(), sizeof(double), (size_t)m.size(), out) != (size_t)m.size()) {
                std::fprintf(stderr, "short write\n");
                return 2;
            }
        }
        std::fclose(out);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "evaluator failed: %s\n", e.what());
        return 1;
    }
    const bool a = throws_for_fmm(skelly::make_stokeslet_evaluator, "make_stokeslet_evaluator");
    const bool b = throws_for_fmm(skelly::make_stresslet_evaluator, "make_stresslet_evaluator");
    return a && b ? 0 : 1;
}
