// Stand-alone program for tests/test_gpu_nearest.py: skelly::nearest of
// include/skelly_evaluator.hpp on one case, results written as they come back.
//
//   nearest_probe CASE OUT
//
// CASE: int64 n_src, n_trg, grouped; r_src (3 x n_src col-major, i.e. xyz per
// point) and r_trg (3 x n_trg) as raw doubles; then, when grouped != 0, n_src
// and n_trg int64 group ids. OUT gets d2 (n_trg doubles), then index (n_trg
// int64).
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

} // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s CASE OUT\n", argv[0]);
        return 2;
    }
    std::FILE *in = open_or_die(argv[1], "rb");
    std::int64_t n[3];
    read_or_die(in, n, 3);
    if (n[0] < 0 || n[1] < 0 || n[0] > (1 << 20) || n[1] > (1 << 20)) {
        std::fprintf(stderr, "counts out of range\n");
        return 2;
    }
    const long n_src = (long)n[0], n_trg = (long)n[1];
    skelly::MatrixXd r_src(3, n_src), r_trg(3, n_trg);
    read_or_die(in, r_src.data(), (size_t)r_src.size());
    read_or_die(in, r_trg.data(), (size_t)r_trg.size());
    std::vector<long long> src_group, trg_group;
    if (n[2]) {
        static_assert(sizeof(long long) == sizeof(std::int64_t), "group ids are 64-bit");
        src_group.resize(n_src);
        trg_group.resize(n_trg);
        read_or_die(in, src_group.data(), (size_t)n_src);
        read_or_die(in, trg_group.data(), (size_t)n_trg);
    }
    std::fclose(in);

    try {
        const skelly::Nearest got = skelly::nearest(r_src, r_trg, src_group, trg_group);
        std::printf("result %zu + %zu\n", got.d2.size(), got.index.size());
        std::FILE *out = open_or_die(argv[2], "wb");
        if ((long)got.d2.size() != n_trg || (long)got.index.size() != n_trg ||
            std::fwrite(got.d2.data(), sizeof(double), (size_t)n_trg, out) != (size_t)n_trg ||
            std::fwrite(got.index.data(), sizeof(long long), (size_t)n_trg, out) !=
                (size_t)n_trg) {
            std::fprintf(stderr, "bad shape or short write\n");
            return 2;
        }
        std::fclose(out);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "nearest failed: %s\n", e.what());
        return 1;
    }
    return 0;
}
