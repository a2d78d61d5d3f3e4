/* fieldline_probe — include/skelly_evaluator.hpp's trace_streamlines or
 * trace_vortexlines called from C++: reads a case written by
 * tests/test_gpu_streamlines.py or tests/test_gpu_vortexlines.py and prints one
 * joined line, a row "t x y z vx vy vz" per point (val is u for a streamline,
 * curl u for a vortex line) with 17 digits, so that the test can compare it
 * with the Python result bit for bit.
 *
 *   fieldline_probe streamlines|vortexlines case.bin seed_index
 *
 * case.bin: int64 {n_sl, n_dl, n_rot, n_os, n_bodies, n_seeds, back_integrate,
 * max_points, has_background}, doubles {eta, reg, eps, dt_init, t_final,
 * abs_err, rel_err, uniform[3], scale_factor[3], components[3]}, then the
 * arrays r_sl, f_sl, r_dl, f_dl (9 a source), r_rot, torques, r_os, f_os,
 * bodies (10 a body), seeds, each point-major. */

#include "skelly_evaluator.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static std::vector<double> read_doubles(std::FILE *f, long n) {
    std::vector<double> v(n);
    if (n && std::fread(v.data(), sizeof(double), n, f) != (size_t)n) {
        std::fprintf(stderr, "short case file\n");
        std::exit(2);
    }
    return v;
}

int main(int argc, char **argv) {
    const bool vortex = argc == 4 && !std::strcmp(argv[1], "vortexlines");
    if (argc != 4 || (!vortex && std::strcmp(argv[1], "streamlines"))) {
        std::fprintf(stderr, "usage: %s streamlines|vortexlines case.bin seed_index\n", argv[0]);
        return 2;
    }
    std::FILE *f = std::fopen(argv[2], "rb");
    if (!f) {
        std::perror(argv[2]);
        return 2;
    }
    long long h[9];
    if (std::fread(h, sizeof(long long), 9, f) != 9)
        return 2;
    const std::vector<double> s = read_doubles(f, 16);
    const int width[4] = {3, 9, 3, 3};
    std::vector<double> r[4], q[4];
    for (int k = 0; k < 4; ++k) {
        r[k] = read_doubles(f, 3 * h[k]);
        q[k] = read_doubles(f, width[k] * h[k]);
    }
    const std::vector<double> bodies = read_doubles(f, 10 * h[4]);
    const std::vector<double> seeds = read_doubles(f, 3 * h[5]);
    std::fclose(f);

    skelly::StreamlineField field;
    field.r_sl = {r[0].data(), 3, (long)h[0]};
    field.f_sl = {q[0].data(), 3, (long)h[0]};
    field.r_dl = {r[1].data(), 3, (long)h[1]};
    field.f_dl = {q[1].data(), 9, (long)h[1]};
    field.r_rot = {r[2].data(), 3, (long)h[2]};
    field.torques = {q[2].data(), 3, (long)h[2]};
    field.r_os = {r[3].data(), 3, (long)h[3]};
    field.f_os = {q[3].data(), 3, (long)h[3]};
    field.bodies = {bodies.data(), 10, (long)h[4]};
    field.has_background = h[8] != 0;
    for (int j = 0; j < 3; ++j) {
        field.uniform[j] = s[7 + j];
        field.scale_factor[j] = s[10 + j];
        field.components[j] = (int)s[13 + j];
    }
    field.eta = s[0];
    field.reg = s[1];
    field.epsilon_distance = s[2];

    try {
        const auto trace = vortex ? skelly::trace_vortexlines : skelly::trace_streamlines;
        const std::vector<skelly::StreamLine> lines = trace(
            field, {seeds.data(), 3, (long)h[5]}, s[3], s[4], s[5], s[6], h[6] != 0, (long)h[7]);
        const skelly::StreamLine &line = lines.at(std::atol(argv[3]));
        std::printf("lines %zu status %d points %ld\n", lines.size(), line.status, line.x.cols());
        for (long c = 0; c < line.x.cols(); ++c)
            std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", line.time[c], line.x(0, c),
                        line.x(1, c), line.x(2, c), line.val(0, c), line.val(1, c),
                        line.val(2, c));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "trace_%s threw: %s\n", argv[1], e.what());
        return 1;
    }
    return 0;
}
