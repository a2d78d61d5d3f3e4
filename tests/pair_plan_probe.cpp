// Stand-alone host program for tests/test_pair_plan.py: reads one shape per
// line from stdin,
//   n_src n_trg max_tpt outdim fast_mode fast_min_src n_cu wg_per_cu forced
// and prints the plan of skellysim_amd/csrc/pair_plan.hpp for it,
//   plan tpt n_slices fast s_max blocks time
// followed by one "cand S time" line per slice count the planner may choose
// from (none when the count is forced).
#include <cstdio>

#include "pair_plan.hpp"

int main() {
    long long n_src, n_trg, fast_min_src;
    int max_tpt, outdim, fast_mode, n_cu, wg_per_cu, forced;
    while (std::scanf("%lld %lld %d %d %d %lld %d %d %d", &n_src, &n_trg, &max_tpt, &outdim,
                      &fast_mode, &fast_min_src, &n_cu, &wg_per_cu, &forced) == 9) {
        const skelly::PairPlan p = skelly::pair_plan(n_src, n_trg, max_tpt, outdim, fast_mode,
                                                     fast_min_src, n_cu, wg_per_cu, forced);
        const long long blocks = skelly::pair_plan_blocks(n_trg, p.tpt);
        const int s_max = skelly::pair_plan_max_slices(n_src, n_trg, outdim);
        const int auto_fast = skelly::pair_plan_fast(n_src, p.n_slices, 1, fast_min_src);
        std::printf("plan %d %d %d %d %lld %.17g\n", p.tpt, p.n_slices, p.fast, s_max, blocks,
                    skelly::pair_plan_time(n_src, n_trg, blocks, outdim, p.n_slices, auto_fast,
                                           n_cu, wg_per_cu));
        if (forced == 0)
            for (int S = 1; S <= s_max; ++S)
                std::printf("cand %d %.17g\n", S,
                            skelly::pair_plan_time(
                                n_src, n_trg, blocks, outdim, S,
                                skelly::pair_plan_fast(n_src, S, 1, fast_min_src), n_cu,
                                wg_per_cu));
        std::printf("end\n");
    }
    return 0;
}
