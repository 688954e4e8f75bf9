// cox_plan.hpp -- the host-only arithmetic of the Cox step (cox_kernels.hpp: cdh_glm_set_survival, cdh_glm_cox_irls): the tile of
// a scan, how the tiles are dealt to the workgroups, the layout of the step's scratch, and the time order with its tie groups
// as cdh_glm_set_survival uploads them -- and, for cdh_glm_set_survival_strata, the order by (stratum, time) with the bounds of
// every position's stratum; for cdh_glm_set_survival_interval, the second order by (stratum, start) and the two static lookups
// that turn the scans into the sums over (start, stop]; the scratch of the post-estimation exports (cox_post_layout); and, for
// cdh_glm_cox_concordance, the concordance order with every event's range of comparable positions, the level arithmetic of the
// merge sort the counts are read off, and that call's scratch (cox_conc_layout); and, for cdh_glm_cox_score, that call's scratch
// (cox_score_layout), the pair tiles of its matrix and the regrowth of the group.  No HIP
// in here: tests/test_cox_plan_host.py, tests/test_cox_strata_plan_host.py, tests/test_cox_interval_plan_host.py,
// tests/test_cox_efron_plan_host.py, tests/test_cox_post_plan_host.py, tests/test_cox_concordance_plan_host.py and
// tests/test_cox_score_plan_host.py compile it with
// g++ (tests/cox_plan_main.cpp, tests/cox_strata_plan_main.cpp, tests/cox_interval_plan_main.cpp, tests/cox_efron_plan_main.cpp,
// tests/cox_post_plan_main.cpp, tests/cox_concordance_plan_main.cpp, tests/cox_score_plan_main.cpp).
// cox_kernels.hpp calls these functions and nothing else decides the sizes.
//
// The tie groups are kept as TWO int32 vectors, not as head flags: first[s] and last[s] are the first and the last sorted
// position of the group that sorted position s belongs to.  The risk-set sum of a row is the suffix scan read at first[s], its
// cumulative hazards the prefix scans read at last[s]: one gather each, and no scan over flags on the device.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <numeric>
#include <vector>

// ---- the kernels' shape ------------------------------------------------------------------------------------------------------
// A lane holds kCoxPer consecutive sorted positions, a workgroup of kCoxBlock lanes a tile of kCoxTile positions.  The positions
// planned are the padded ld of the handle (a multiple of 32, so a lane's positions lie wholly below ld or wholly beyond):
// positions n .. ld - 1 stand for the pad rows n .. ld - 1, in place.  Workgroup b owns the CONTIGUOUS run of tiles
// cox_run_first(b) .. cox_run_first(b + 1) - 1 and carries its running sum from tile to tile (forwards for a prefix scan,
// backwards for a suffix scan); a launch of one workgroup turns the runs' sums into the runs' offsets between two scans.
constexpr int kCoxBlock = 256;
constexpr int kCoxPer = 4;
constexpr int64_t kCoxTile = (int64_t)kCoxBlock * kCoxPer;
constexpr int64_t kCoxMaxGrid = 1024;                     // the runs' sums are scanned by ONE workgroup: kCoxPer a lane
constexpr int kCoxVals = 5;                               // the record: (nll, sum w, clamped, capped, events)
static_assert(kCoxMaxGrid == kCoxTile, "k_cox_offsets scans the runs' sums as one tile");

struct CoxPlan {
    int64_t tiles;     // tiles of kCoxTile positions over ld (the last may be short)
    int64_t grid;      // workgroups: min(tiles, cap), at least 1; every one owns at least one tile
    int64_t records;   // partial records of the apply launch: one per workgroup
    int64_t longest;   // tiles of the longest run
};

// cap: kCoxMaxGrid, or the smaller grid a test asks for (CDH_COX_GRID); values outside 1 .. kCoxMaxGrid mean kCoxMaxGrid
constexpr int64_t cox_grid_cap(int64_t cap) { return (cap < 1 || cap > kCoxMaxGrid) ? kCoxMaxGrid : cap; }

constexpr CoxPlan cox_plan(int64_t ld, int64_t cap = kCoxMaxGrid) {
    const int64_t tiles = (ld + kCoxTile - 1) / kCoxTile;
    const int64_t c = cox_grid_cap(cap);
    int64_t grid = tiles < c ? tiles : c;
    if (grid < 1) grid = 1;
    return CoxPlan{tiles, grid, grid, (tiles + grid - 1) / grid};
}

// the first tile of workgroup b's run (b == grid: one past the last tile): the tiles split as evenly as integers allow,
// tiles <= 2^21 and b <= 2^10, so the product stays far inside int64
constexpr int64_t cox_run_first(int64_t tiles, int64_t grid, int64_t b) { return b * tiles / grid; }

// ---- the scratch -------------------------------------------------------------------------------------------------------------
// One buffer of doubles: e (then T, its suffix scan, in place), h (then A), h2 (then B) and the times, ld each, then the
// runs' sums (then offsets) of the three scans, kCoxMaxGrid each.  One buffer of int32: order, first, last, ld each.
// A handle with strata or observation weights (cdh_glm_set_survival_strata) holds a SECOND pair of buffers, which a plain
// handle never allocates: int32 -- sfirst and slast, the bounds of every position's stratum, the stratum ids in the caller's
// row order (for the getter), ld each, then the head-seen flags of the runs, kCoxMaxGrid for the suffix scan and kCoxMaxGrid
// for the two prefix scans; doubles -- the weights in the caller's row order, ld.
// A handle with start times (cdh_glm_set_survival_interval) holds the second pair AND a THIRD: int32 -- pos2 (the start order,
// as positions of the stop order), lo and enter (cox_order_interval), ld each, then the head-seen flags of the second suffix
// scan's runs, kCoxMaxGrid; doubles -- the start times in the caller's row order, T2 (ev in start order, then its suffix scan
// in place), ld each, then that scan's runs' sums, kCoxMaxGrid.
struct CoxLayout {
    int64_t eT, hA, hB, time, sums;   // offsets in doubles; sums + i kCoxMaxGrid: scan i's runs
    int64_t doubles;
    int64_t order, first, last;       // offsets in int32s
    int64_t ints;
    int64_t sfirst, slast, strata, heads;   // offsets in int32s of the second pair; heads + i kCoxMaxGrid: suffix (0), prefix (1)
    int64_t strata_ints;
    int64_t weight;                   // offset in doubles of the second pair
    int64_t strata_doubles;
    int64_t pos2, lo, enter, heads2;  // offsets in int32s of the third pair
    int64_t interval_ints;
    int64_t start, T2, sums2;         // offsets in doubles of the third pair
    int64_t interval_doubles;
};
constexpr CoxLayout cox_layout(int64_t ld) {
    return CoxLayout{0, ld, 2 * ld, 3 * ld, 4 * ld, 4 * ld + 3 * kCoxMaxGrid, 0, ld, 2 * ld, 3 * ld,
                     0, ld, 2 * ld, 3 * ld, 3 * ld + 2 * kCoxMaxGrid, 0, ld,
                     0, ld, 2 * ld, 3 * ld, 3 * ld + kCoxMaxGrid, 0, ld, 2 * ld, 2 * ld + kCoxMaxGrid};
}

// A handle set to Efron ties (cdh_glm_set_cox_ties) holds the second pair AND a pair of its own, which no other handle
// allocates.  Doubles, ld each: cnt and Dv (the event indicator and ev at the events, then their prefix scans inside the tie
// group: an event's rank l + 1, and d_g and D_g at the group's last position), Sdv (dv, then its SUFFIX scan inside the tie
// group: sum dv of the group at its first position), hc and hc2 (the event's own-group terms m c / den and m c^2 / den^2, then
// their prefix scans inside the tie group), lg and mm (log den and m at an event that counts, else 0: the nll's terms); then
// the runs' sums of the five scans, kCoxMaxGrid each, in the order cnt, Dv, Sdv, hc, hc2.  cnt and Dv, and hc and hc2, are ld
// apart and their sums kCoxMaxGrid apart: each pair is ONE launch of k_cox_scan<2, false, true>.  int32: the head-seen flags
// of the runs for the scans whose heads are the tie groups' first positions (heads_p) and last positions (heads_s),
// kCoxMaxGrid each.
struct CoxEfronLayout {
    int64_t cnt, Dv, Sdv, hc, hc2, lg, mm, sums;   // offsets in doubles; sums + i kCoxMaxGrid: cnt, Dv, Sdv, hc, hc2
    int64_t doubles;
    int64_t heads_p, heads_s;                      // offsets in int32s
    int64_t ints;
};
constexpr CoxEfronLayout cox_efron_layout(int64_t ld) {
    return CoxEfronLayout{0, ld, 2 * ld, 3 * ld, 4 * ld, 5 * ld, 6 * ld, 7 * ld, 7 * ld + 5 * kCoxMaxGrid,
                          0, kCoxMaxGrid, 2 * kCoxMaxGrid};
}

// A handle that was asked for a post-estimation export (cdh_glm_cox_residuals, cdh_glm_cox_baseline; cox_post.hip) holds a pair
// of its own, allocated by the first such call and by no other.  Doubles, ld each: dv (v delta in sorted order, then its prefix
// scan inside the tie group: the group's n_event at its last position), flag (1 at the last position of a tie group that holds
// an event, then its plain prefix scan: the group's slot in the table, plus one), and kCoxPostCols = 5 output vectors -- the
// table's columns time, n_event, risk_sum, cumhaz, cumvar (a table has at most n rows), or the rows' export cumhaz, martingale,
// deviance in the first three; then the runs' sums of the two scans, kCoxMaxGrid each, and ONE double: the table's length.
// int32: the table's stratum column and slotpos (the last sorted position of every table row's tie group: where the rows'
// export reads hA), ld each, and the head-seen flags of the runs for the scan of dv, kCoxMaxGrid.
constexpr int kCoxPostCols = 5;
struct CoxPostLayout {
    int64_t dv, flag, out, sums, total;   // offsets in doubles; out + c ld: column c; sums + i kCoxMaxGrid: dv (0), flag (1)
    int64_t doubles;
    int64_t stratum, slotpos, heads;      // offsets in int32s
    int64_t ints;
};
constexpr CoxPostLayout cox_post_layout(int64_t ld) {
    return CoxPostLayout{0, ld, 2 * ld, (2 + kCoxPostCols) * ld, (2 + kCoxPostCols) * ld + 2 * kCoxMaxGrid,
                         (2 + kCoxPostCols) * ld + 2 * kCoxMaxGrid + 1, 0, ld, 2 * ld, 2 * ld + kCoxMaxGrid};
}

// A handle that was asked for score or Schoenfeld residuals or the information matrix (cdh_glm_cox_score; cox_score.hip) holds a
// SIXTH pair, allocated whole by the first such call for the m columns it asks for and regrown whole, never shrunk, when a later
// call asks for more (cox_score_grow); no other call allocates it and no setter needs to drop it: every call fills it again.
// Doubles: e, ev, h, dvk and wA by sorted position (exp(eta); v e; the hazard term dv / S at an event that counts, else 0; dv at
// such an event, else 0; ev A), ld each; then per column, ld apart: xt (the centred column in sorted order), N (ev xt, then
// its suffix scan inside the stratum) and Q (h xbar, then its prefix scan inside the stratum); the runs' sums of the two scans,
// kCoxMaxGrid per column each; the kCoxScoreMaxCols centres; the two residual outputs, ld m each (stored n apart); the
// information matrix's partials, kCoxMaxGrid runs x pair tiles x 2 sums x kCoxScorePair^2 entries; and the m x m matrix.
// int32: the head-seen flags of the runs for the suffix scan and the prefix scan, kCoxMaxGrid each, and the kCoxScoreMaxCols
// column indices (0-based).
constexpr int kCoxScoreMaxCols = 64;                      // cdh_vc_gram's cap
constexpr int kCoxScorePair = 4;                          // the information matrix is computed in pair tiles of 4 x 4 columns
constexpr int kCoxScoreCentreRuns = 256;                  // workgroups that share a column's rows for its mean; their partials,
                                                          // kCoxScoreCentreRuns a column, lie at the head of the matrix's partials
constexpr int64_t cox_score_col_tiles(int64_t m) { return (m + kCoxScorePair - 1) / kCoxScorePair; }
constexpr int64_t cox_score_pair_tiles(int64_t m) { return cox_score_col_tiles(m) * (cox_score_col_tiles(m) + 1) / 2; }
// pair tile t of ct column tiles -> its column tiles (ci <= di), row by row of the upper triangle; and back
struct CoxScorePair { int64_t ci, di; };
constexpr CoxScorePair cox_score_pair(int64_t ct, int64_t t) {
    int64_t ci = 0;
    while (t >= ct - ci) { t -= ct - ci; ++ci; }
    return CoxScorePair{ci, ci + t};
}
constexpr int64_t cox_score_pair_index(int64_t ct, int64_t ci, int64_t di) { return ci * ct - ci * (ci - 1) / 2 + (di - ci); }
// the columns the group holds room for after a call that asks for m: never fewer than before
constexpr int64_t cox_score_grow(int64_t have, int64_t m) { return m > have ? m : have; }
struct CoxScoreLayout {
    int64_t e, ev, h, dvk, wA, xt, N, Q, sums, mu, out, part, info;   // offsets in doubles; sums + (a m + c) kCoxMaxGrid: scan a
    int64_t doubles;
    int64_t heads, idx;                                                // offsets in int32s; heads + a kCoxMaxGrid
    int64_t ints;
};
constexpr CoxScoreLayout cox_score_layout(int64_t ld, int64_t m) {
    static_assert(kCoxMaxGrid * 2 * kCoxScorePair * kCoxScorePair >= (int64_t)kCoxScoreCentreRuns * kCoxScorePair * 2,
                  "the partials of the matrix hold the centres' partials: pair tiles >= column tiles / 2, 4 columns a tile");
    const int64_t xt = 5 * ld, sums = xt + 3 * m * ld, mu = sums + 2 * m * kCoxMaxGrid, out = mu + kCoxScoreMaxCols,
                  part = out + 2 * m * ld,
                  info = part + kCoxMaxGrid * cox_score_pair_tiles(m) * 2 * kCoxScorePair * kCoxScorePair;
    return CoxScoreLayout{0, ld, 2 * ld, 3 * ld, 4 * ld, xt, xt + m * ld, xt + 2 * m * ld, sums, mu, out, part, info,
                          info + m * m, 0, 2 * kCoxMaxGrid, 2 * kCoxMaxGrid + kCoxScoreMaxCols};
}

// ---- the time order and its tie groups ---------------------------------------------------------------------------------------
// What cdh_glm_set_survival refuses of its data, the row named in msg (at least 128 chars): a time or an offset that is not
// finite, a status other than 0 or 1, a weight (cdh_glm_set_survival_strata; NULL: none) that is not finite or not > 0, no
// event at all.  -> true when the data pass.
inline bool cox_check(int64_t n, const double* time, const double* status, const double* offset, char* msg, size_t len,
                      const double* weights = nullptr) {
    int64_t events = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (!(fabs(time[i]) <= 1.7976931348623157e308)) {          // (a NaN fails the comparison)
            snprintf(msg, len, "time[%lld] = %g is not finite", (long long)i, time[i]);
            return false;
        }
        if (status[i] != 0.0 && status[i] != 1.0) {
            snprintf(msg, len, "status[%lld] = %g is neither 0 (censored) nor 1 (event)", (long long)i, status[i]);
            return false;
        }
        if (offset && !(fabs(offset[i]) <= 1.7976931348623157e308)) {
            snprintf(msg, len, "offset[%lld] = %g is not finite", (long long)i, offset[i]);
            return false;
        }
        if (weights && !(weights[i] > 0.0 && weights[i] <= 1.7976931348623157e308)) {
            snprintf(msg, len, "weights[%lld] = %g is not finite and > 0", (long long)i, weights[i]);
            return false;
        }
        events += status[i] == 1.0;
    }
    if (events == 0) {
        snprintf(msg, len, "no row is an event: the partial likelihood is constant");
        return false;
    }
    return true;
}

// order[s]: the row at sorted position s, by a stable ascending sort of the times (rows of equal time keep the caller's order);
// first[s], last[s]: the bounds of s's tie group.  Positions n .. ld - 1 are the pad rows in place, each a group of its own.
inline void cox_order(int64_t n, int64_t ld, const double* time, std::vector<int32_t>& order, std::vector<int32_t>& first,
                      std::vector<int32_t>& last) {
    order.resize((size_t)ld);
    first.resize((size_t)ld);
    last.resize((size_t)ld);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.begin() + n, [&](int32_t a, int32_t b) { return time[a] < time[b]; });
    for (int64_t s = 0; s < n;) {
        int64_t e = s + 1;
        while (e < n && time[order[e]] == time[order[s]]) ++e;
        for (int64_t q = s; q < e; ++q) { first[q] = (int32_t)s; last[q] = (int32_t)(e - 1); }
        s = e;
    }
    for (int64_t s = n; s < ld; ++s) { first[s] = (int32_t)s; last[s] = (int32_t)s; }
}

// The same order with strata: a stable ascending sort by (stratum id, time) -- the strata in ascending id order, the rows of a
// stratum in time order, rows equal in both in the caller's order -- so that a stratum is a SEGMENT of sorted positions.
// first[s], last[s]: the bounds of s's tie group (same stratum AND same time); sfirst[s], slast[s]: the bounds of s's stratum.
// Positions n .. ld - 1 are the pad rows in place: each a tie group of its own, together ONE stratum (n .. ld - 1).
// strata == nullptr: one stratum; order, first and last are then cox_order's, element for element.
inline void cox_order_strata(int64_t n, int64_t ld, const double* time, const int32_t* strata, std::vector<int32_t>& order,
                             std::vector<int32_t>& first, std::vector<int32_t>& last, std::vector<int32_t>& sfirst,
                             std::vector<int32_t>& slast) {
    order.resize((size_t)ld);
    first.resize((size_t)ld);
    last.resize((size_t)ld);
    sfirst.resize((size_t)ld);
    slast.resize((size_t)ld);
    std::iota(order.begin(), order.end(), 0);
    auto stratum = [&](int32_t row) { return strata ? strata[row] : 0; };
    std::stable_sort(order.begin(), order.begin() + n, [&](int32_t a, int32_t b) {
        return stratum(a) != stratum(b) ? stratum(a) < stratum(b) : time[a] < time[b];
    });
    for (int64_t s = 0; s < n;) {
        int64_t se = s + 1;
        while (se < n && stratum(order[se]) == stratum(order[s])) ++se;
        for (int64_t g = s; g < se;) {
            int64_t e = g + 1;
            while (e < se && time[order[e]] == time[order[g]]) ++e;
            for (int64_t q = g; q < e; ++q) { first[q] = (int32_t)g; last[q] = (int32_t)(e - 1); }
            g = e;
        }
        for (int64_t q = s; q < se; ++q) { sfirst[q] = (int32_t)s; slast[q] = (int32_t)(se - 1); }
        s = se;
    }
    for (int64_t s = n; s < ld; ++s) {
        first[s] = (int32_t)s; last[s] = (int32_t)s;
        sfirst[s] = (int32_t)n; slast[s] = (int32_t)(ld - 1);
    }
}

// The strata's bounds of a handle WITHOUT strata, as cox_order_strata(.., strata = nullptr, ..) gives them -- the rows one
// stratum, the pads another -- without sorting again: what cdh_glm_set_cox_ties stores when a plain handle turns to Efron, whose
// chain is segmented (order, first and last are then cox_order's and stay).
inline void cox_one_stratum(int64_t n, int64_t ld, std::vector<int32_t>& sfirst, std::vector<int32_t>& slast) {
    sfirst.assign((size_t)ld, 0);
    slast.assign((size_t)ld, (int32_t)(n - 1));
    for (int64_t s = n; s < ld; ++s) { sfirst[(size_t)s] = (int32_t)n; slast[(size_t)s] = (int32_t)(ld - 1); }
}

// ---- start-stop times: the second order and the two lookups --------------------------------------------------------------------
// What cdh_glm_set_survival_interval refuses of its start times, after cox_check has passed the stop times: a start that is not
// finite, and an interval (start, stop] that is empty, start >= stop; the row named in msg.  -> true when they pass.
inline bool cox_check_interval(int64_t n, const double* start, const double* stop, char* msg, size_t len) {
    for (int64_t i = 0; i < n; ++i) {
        if (!(fabs(start[i]) <= 1.7976931348623157e308)) {
            snprintf(msg, len, "start[%lld] = %g is not finite", (long long)i, start[i]);
            return false;
        }
        if (!(start[i] < stop[i])) {
            snprintf(msg, len, "start[%lld] = %g is not below stop[%lld] = %g", (long long)i, start[i], (long long)i, stop[i]);
            return false;
        }
    }
    return true;
}

// Row i is at risk at t iff start_i < t <= stop_i.  order, first, last, sfirst and slast are cox_order_strata's on the stop
// times, element for element.  order2[s]: the row at position s of the SECOND order, a stable ascending sort by (stratum,
// start); a stratum occupies the same positions in both orders, so sfirst and slast bound it in either.  pos2[s]: the position
// of that row in the stop order (order[pos2[s]] == order2[s]): what the device gathers ev through, so that ev is the same bits
// in both orders.  Two lookups, both inside the stratum of stop-order position s:
//   lo[s]     the first start-order position whose start is >= the stop time of position s; -1 if none.  The suffix scan of ev in
//             start order read there is the sum over the rows that have NOT YET entered at that time: a row whose start equals
//             an event time is not at risk at it.
//   enter[s]  the last stop-order position whose stop time is <= the start of row order[s]; -1 if none.  The prefix scans of
//             the hazard read there are the sums over the event times the row was not yet at risk at.
// Pad positions n .. ld - 1 stay in place in both orders, with lo = enter = -1.
inline void cox_order_interval(int64_t n, int64_t ld, const double* start, const double* stop, const int32_t* strata,
                               std::vector<int32_t>& order, std::vector<int32_t>& first, std::vector<int32_t>& last,
                               std::vector<int32_t>& sfirst, std::vector<int32_t>& slast, std::vector<int32_t>& order2,
                               std::vector<int32_t>& pos2, std::vector<int32_t>& lo, std::vector<int32_t>& enter) {
    cox_order_strata(n, ld, stop, strata, order, first, last, sfirst, slast);
    order2.resize((size_t)ld);
    pos2.resize((size_t)ld);
    lo.assign((size_t)ld, -1);
    enter.assign((size_t)ld, -1);
    std::iota(order2.begin(), order2.end(), 0);
    auto stratum = [&](int32_t row) { return strata ? strata[row] : 0; };
    std::stable_sort(order2.begin(), order2.begin() + n, [&](int32_t a, int32_t b) {
        return stratum(a) != stratum(b) ? stratum(a) < stratum(b) : start[a] < start[b];
    });
    std::vector<int32_t> where((size_t)ld);                       // row -> its position in the stop order
    for (int64_t s = 0; s < ld; ++s) where[(size_t)order[s]] = (int32_t)s;
    for (int64_t s = 0; s < ld; ++s) pos2[s] = where[(size_t)order2[s]];
    for (int64_t s = 0; s < n; ++s) {
        const int64_t a = sfirst[s], b = slast[s];
        const double t = stop[order[s]], u = start[order[s]];
        int64_t l = a, r = b + 1;                                 // the first position of a .. b in start order with start >= t
        while (l < r) {
            const int64_t m = l + (r - l) / 2;
            if (start[order2[m]] >= t) r = m; else l = m + 1;
        }
        lo[s] = l <= b ? (int32_t)l : -1;
        l = a, r = b + 1;                                         // the first position of a .. b in stop order with stop > u
        while (l < r) {
            const int64_t m = l + (r - l) / 2;
            if (stop[order[m]] > u) r = m; else l = m + 1;
        }
        enter[s] = l > a ? (int32_t)(l - 1) : -1;
    }
}

// ---- the concordance index (cdh_glm_cox_concordance; cox_concordance.hip) ------------------------------------------------------
// The concordance order: the Cox order with every tie group stably partitioned, its events before its censored rows -- a stable
// sort by (stratum, time, events before censored).  For a position s that holds an event the rows it is comparable with (a
// later time in its stratum, or the same time and censored) are then ONE range of positions [qa[s], qb[s]): qa is the first
// censored position of s's tie group (the group's end when it has none), qb the end of s's stratum.  Every other position, the
// pads included, has qa = qb = 0.  order, last, slast: the handle's (slast == nullptr: one stratum, 0 .. n - 1);
// status: by row.  corder, qa, qb get N entries, N >= ld the positions the kernels plan (cox_conc_layout); the pads stay in
// place and the positions beyond ld hold row -1, which no kernel reads.
inline void cox_conc_order(int64_t n, int64_t ld, int64_t N, const int32_t* order, const int32_t* last, const int32_t* slast, const double* status, std::vector<int32_t>& corder, std::vector<int32_t>& qa,
                           std::vector<int32_t>& qb) {
    corder.assign((size_t)N, -1);
    qa.assign((size_t)N, 0);
    qb.assign((size_t)N, 0);
    for (int64_t s = n; s < ld; ++s) corder[(size_t)s] = (int32_t)s;
    for (int64_t g = 0; g < n;) {
        const int64_t e = (int64_t)last[g] + 1;
        int64_t at = g;
        for (int64_t s = g; s < e; ++s)
            if (status[order[s]] == 1.0) corder[(size_t)at++] = order[s];
        const int64_t censored = at;
        for (int64_t s = g; s < e; ++s)
            if (status[order[s]] != 1.0) corder[(size_t)at++] = order[s];
        const int64_t end = slast ? (int64_t)slast[g] + 1 : n;
        for (int64_t s = g; s < censored; ++s) { qa[(size_t)s] = (int32_t)censored; qb[(size_t)s] = (int32_t)end; }
        g = e;
    }
}

// The level arithmetic.  At level lev the positions are cut into the runs [m 2^lev, (m + 1) 2^lev), each sorted by eta.  A range
// [a, b) is the disjoint union of at most two WHOLE runs per level, the iterative segment-tree walk: with l = ceil(a / 2^lev)
// and r = floor(b / 2^lev), while l < r, run l is taken if l is odd and run r - 1 if r is odd (l odd and r odd never name the
// same run: then r - 1 is even).  Both are closed forms of lev, so a kernel that holds level lev alone can answer its part.
struct CoxConcTake { int64_t run[2]; int count; };
constexpr CoxConcTake cox_conc_take(int64_t a, int64_t b, int lev) {
    const int64_t l = (a + ((int64_t)1 << lev) - 1) >> lev, r = b >> lev;
    CoxConcTake t{{0, 0}, 0};
    if (l < r) {
        if (l & 1) t.run[t.count++] = l;
        if (r & 1) t.run[t.count++] = r - 1;
    }
    return t;
}

// The levels below the tile are not kept: what the walk takes of them is exactly the two FRINGES of the range, [a, a1) and
// [b0, b) with a1 = a rounded up and b0 = b rounded down to a multiple of the tile (both clipped so that a <= a1 <= b0 <= b: a
// range inside two neighbouring tiles is all fringe), and a fringe is counted position by position.  The levels from the tile's
// up then tile [a1, b0).
constexpr int kCoxTileLog = 10;
static_assert(((int64_t)1 << kCoxTileLog) == kCoxTile, "the first level the level kernel reads is the tile's");
struct CoxConcFringe { int64_t a1, b0; };
constexpr CoxConcFringe cox_conc_fringe(int64_t a, int64_t b) {
    int64_t a1 = (a + kCoxTile - 1) / kCoxTile * kCoxTile;
    if (a1 > b) a1 = b;
    int64_t b0 = b / kCoxTile * kCoxTile;
    if (b0 < a1) b0 = a1;
    return CoxConcFringe{a1, b0};
}
// the last level: the first whose one run holds all N positions (N a multiple of the tile, so top >= kCoxTileLog)
constexpr int cox_conc_top(int64_t N) {
    int lev = kCoxTileLog;
    while (((int64_t)1 << lev) < N) ++lev;
    return lev;
}

// A handle that was asked for the concordance index holds a FIFTH pair, allocated whole by the first cdh_glm_cox_concordance
// after a setter of survival data and dropped by that setter (the order is the data's).  N: ld rounded up to whole tiles.
// Doubles, N each: key0 and v0 (eta and the weight by position; +inf and 0 outside the subset and on the pads), two ping-pong
// pairs (ka, pa) and (kb, pb) -- a level's keys and the inclusive prefix sums of the weights inside its runs -- and the rows'
// three sums L (smaller eta), E (smaller or equal) and G (all) over their ranges; then 4 doubles per tile (the tiles' partial
// concordant, discordant, tied and NaN counts) and the 4 of the result.  int32, N each: corder, qa, qb.
struct CoxConcLayout {
    int64_t N, tiles;
    int64_t key0, v0, ka, pa, kb, pb, L, E, G, part, out;   // offsets in doubles
    int64_t doubles;
    int64_t order, qa, qb;                                   // offsets in int32s
    int64_t ints;
};
constexpr CoxConcLayout cox_conc_layout(int64_t ld) {
    const int64_t tiles = ld > 0 ? (ld + kCoxTile - 1) / kCoxTile : 1, N = tiles * kCoxTile;
    return CoxConcLayout{N, tiles, 0, N, 2 * N, 3 * N, 4 * N, 5 * N, 6 * N, 7 * N, 8 * N, 9 * N, 9 * N + 4 * tiles,
                         9 * N + 4 * tiles + 4, 0, N, 2 * N, 3 * N};
}
