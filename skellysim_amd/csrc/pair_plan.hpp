/* pair_plan.hpp — launch planner of the pair kernels (host only, no HIP).
 *
 * Picks how many source slices (gridDim.y of pair_driver) a launch gets from
 * a load-balance model of the compute units (CUs), instead of aiming at a
 * fixed workgroup count. A pure function of its arguments: no timing
 * feedback, no state, so a given (shape, CU count, occupancy) always gets
 * the same plan and with it the same summation order.
 *
 * Model. The pair loop is issue-bound and every workgroup (WG) of a launch
 * walks the same number of sources, so a CU finishes after a time
 * proportional to the number of WGs it is handed. W = blocks * S equal WGs
 * on n_cu CUs cost ceil(W / n_cu) WG-times against an ideal W / n_cu:
 *
 *   time(S) = q * L * c_path * c_fill + S * n_trg * OUTDIM * c_reduce,
 *             q = ceil(blocks*S / n_cu),  L = ceil(n_src / S)
 *
 * in units of one WG walking one source on the fast path. c_path is 1 on the
 * unmasked fast path and the measured masked/fast ratio on the masked one;
 * c_reduce is the partial-buffer round trip of one output double of one
 * slice. A fixed cost per WG was fitted too and came out as zero within the
 * noise (either sign at the two sizes swept), so the model has none.
 * Measured times follow ceil(W / n_cu) down to one WG a CU, for 1, 2 and 4
 * targets a thread, but a CU with fewer WGs than wg_per_cu (the functor's
 * launch bound K::MIN_WAVES: what a CU held at once when this was fitted,
 * with the sources still staged through LDS tiles) hid a little less of that
 * staging: c_fill = 1 + c_underfill * (wg_per_cu - q) / (wg_per_cu - 1) for
 * q < wg_per_cu, else 1 (3 % at one WG a CU, 1.5 % at two of three). The
 * constant has not been refitted since the sources moved to scalar loads.
 * Constants and what they were measured on: profiles/pair_balance.md.
 *
 * While a launch has no more WGs than CUs, ceil() is 1 and every further
 * slice shortens it: launches that underfill the chip are sliced as far as
 * the constraints allow, as they were under the old "at least 1024 WGs"
 * rule.
 *
 * Constraints: at least ~2048 sources a slice (S <= ceil(n_src / 2048), the
 * rule every small launch already followed, so their plans are unchanged),
 * the partial workspace S * OUTDIM * n_trg * 8 bytes within
 * PAIR_PLAN_WS_CAP, S <= PAIR_PLAN_MAX_SLICES. The smallest modelled time
 * wins, ties go to the smaller S.
 */
#ifndef SKELLY_PAIR_PLAN_HPP
#define SKELLY_PAIR_PLAN_HPP

namespace skelly {

constexpr int PAIR_PLAN_BLOCK = 256;               /* threads a WG (BLOCK) */
constexpr long long PAIR_PLAN_MIN_SRC = 2048;      /* sources a slice, floor */
constexpr long long PAIR_PLAN_WS_CAP = 144LL << 20; /* partial workspace, bytes */
constexpr int PAIR_PLAN_MAX_SLICES = 1024;         /* planner's search bound */
constexpr int PAIR_PLAN_MAX_GRID_Y = 65535;        /* gridDim.y limit */

/* Fitted on one MI355X (256 CUs), profiles/pair_balance.md. */
constexpr double PAIR_PLAN_C_MASKED = 1.07;   /* masked / fast time a source */
constexpr double PAIR_PLAN_C_REDUCE = 1.6e-5; /* a slice's double through the
                                                 workspace, in WG-sources */
constexpr double PAIR_PLAN_C_UNDERFILL = 0.03; /* one WG on a CU against a full CU */

struct PairPlan {
    int tpt;      /* targets a thread */
    int n_slices; /* source slices (gridDim.y); 1 = unsplit launch */
    int fast;     /* unmasked fast path on */
};

/* Targets per thread: 4 where the functor's registers hold them and there
 * are targets to fill a block, else 2, else 1. */
inline int pair_plan_tpt(int max_tpt, long long n_trg) {
    if (max_tpt >= 4 && n_trg >= PAIR_PLAN_BLOCK * 4)
        return 4;
    if (max_tpt >= 2 && n_trg >= PAIR_PLAN_BLOCK * 2)
        return 2;
    return 1;
}

inline long long pair_plan_blocks(long long n_trg, int tpt) {
    const long long per = (long long)PAIR_PLAN_BLOCK * tpt;
    return (n_trg + per - 1) / per;
}

/* fast_mode: 0 off, 1 auto (on when a slice holds >= fast_min_src sources),
 * 2 always on. */
inline int pair_plan_fast(long long n_src, int n_slices, int fast_mode,
                          long long fast_min_src) {
    const long long src_per_slice = (n_src + n_slices - 1) / n_slices;
    return fast_mode == 2 || (fast_mode == 1 && src_per_slice >= fast_min_src);
}

/* Modelled time of a launch with S slices (see the file header). */
inline double pair_plan_time(long long n_src, long long n_trg, long long blocks, int outdim,
                             int S, int fast, int n_cu, int wg_per_cu) {
    const long long L = (n_src + S - 1) / S;
    const long long q = (blocks * S + n_cu - 1) / n_cu;
    const double c_path = fast ? 1.0 : PAIR_PLAN_C_MASKED;
    double t = (double)q * (double)L * c_path;
    if (q < wg_per_cu)
        t *= 1.0 + PAIR_PLAN_C_UNDERFILL * (double)(wg_per_cu - q) / (double)(wg_per_cu - 1);
    if (S > 1)
        t += (double)S * (double)n_trg * outdim * PAIR_PLAN_C_REDUCE;
    return t;
}

/* Upper bound of the planner's slice count for a shape. */
inline int pair_plan_max_slices(long long n_src, long long n_trg, int outdim) {
    long long m = (n_src + PAIR_PLAN_MIN_SRC - 1) / PAIR_PLAN_MIN_SRC;
    const long long by_ws = PAIR_PLAN_WS_CAP / ((long long)outdim * n_trg * 8);
    if (m > by_ws)
        m = by_ws;
    if (m > PAIR_PLAN_MAX_SLICES)
        m = PAIR_PLAN_MAX_SLICES;
    return m < 1 ? 1 : (int)m;
}

/* forced_slices >= 1 bypasses the model and the constraints above (sweeps,
 * tests): exactly that many slices, clamped to n_src and to gridDim.y. */
inline PairPlan pair_plan(long long n_src, long long n_trg, int max_tpt, int outdim,
                          int fast_mode, long long fast_min_src, int n_cu, int wg_per_cu,
                          int forced_slices = 0) {
    PairPlan p;
    p.tpt = pair_plan_tpt(max_tpt, n_trg);
    if (n_cu < 1)
        n_cu = 1;
    if (wg_per_cu < 1)
        wg_per_cu = 1;
    if (n_trg < 1)
        n_trg = 1;
    if (forced_slices >= 1) {
        long long s = forced_slices;
        if (s > n_src)
            s = n_src;
        if (s > PAIR_PLAN_MAX_GRID_Y)
            s = PAIR_PLAN_MAX_GRID_Y;
        p.n_slices = s < 1 ? 1 : (int)s;
        p.fast = pair_plan_fast(n_src, p.n_slices, fast_mode, fast_min_src);
        return p;
    }
    const long long blocks = pair_plan_blocks(n_trg, p.tpt);
    const int s_max = pair_plan_max_slices(n_src, n_trg, outdim);
    int best = 1;
    double best_t = 0.0;
    for (int S = 1; S <= s_max; ++S) {
        /* costed as in auto mode whatever fast_mode says: the slice count,
         * hence the summation order, must not depend on that switch */
        const int fast = pair_plan_fast(n_src, S, 1, fast_min_src);
        const double t = pair_plan_time(n_src, n_trg, blocks, outdim, S, fast, n_cu, wg_per_cu);
        if (S == 1 || t < best_t) {
            best = S;
            best_t = t;
        }
    }
    p.n_slices = best;
    p.fast = pair_plan_fast(n_src, best, fast_mode, fast_min_src);
    return p;
}

} // namespace skelly

#endif
