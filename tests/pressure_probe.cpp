// Stand-alone program for tests/test_gpu_pressure.py: the three pressure
// functions of include/skelly_evaluator.hpp on one case, results written as
// they come back.
//
//   pressure_probe CASE OUT
//
// CASE is the file tests/evaluator_probe.cpp reads: int64 n_src, n_trg; double
// eta, reg, eps; then r_src (3 x n_src col-major, i.e. xyz per point), r_trg
// (3 x n_trg), f3 (3 x n_src) and f9 (9 x n_src), raw doubles. eta is read and
// not used: no pressure depends on it. OUT gets, as raw doubles in this order,
//   stokeslet_pressure, stresslet_pressure, oseen_tensor_contract_pressure
//                                                     (1 x n_trg each)
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
    const double reg = par[1], eps = par[2];
    const skelly::MatrixXd r_src = read_matrix(in, 3, n_src), r_trg = read_matrix(in, 3, n_trg),
                           f3 = read_matrix(in, 3, n_src), f9 = read_matrix(in, 9, n_src);
    std::fclose(in);

    try {
        const std::vector<skelly::MatrixXd> results = {
            skelly::stokeslet_pressure(r_src, r_trg, f3),
            skelly::stresslet_pressure(r_src, r_trg, f9),
            skelly::oseen_tensor_contract_pressure(r_src, r_trg, f3, reg, eps),
        };
        std::FILE *out = open_or_die(argv[2], "wb");
        for (const skelly::MatrixXd &m : results) {
            std::printf("result %ld x %ld\n", m.rows(), m.cols());
            if (m.rows() != 1 || m.cols() != n_trg ||
                std::fwrite(m.data(), sizeof(double), (size_t)m.size(), out) != (size_t)m.size()) {
                std::fprintf(stderr, "bad shape or short write\n");
                return 2;
            }
        }
        std::fclose(out);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "evaluator failed: %s\n", e.what());
        return 1;
    }
    return 0;
}
