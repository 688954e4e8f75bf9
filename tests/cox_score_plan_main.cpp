// Stand-alone check of what csrc/cox_plan.hpp adds for cdh_glm_cox_score (tests/test_cox_score_plan_host.py builds and runs it
// under the host sanitizers).
//   no arguments     cox_score_layout at many (ld, m): the spans in order, back to back, nothing overlaps and nothing is unused;
//                    the group walked the way the kernels walk it over exactly-sized heap blocks (a lane that leaves its block is
//                    an ASan report): every position of every per-column vector once, a record per run and column, the
//                    partials of every (run, pair tile), every entry of the matrix; the pair tiles: every pair (c, d) with
//                    c <= d < m in exactly one tile for m = 1 .. 64, cox_score_pair and cox_score_pair_index inverse to each
//                    other; the regrowth never shrinks and the regrown layout holds the smaller one's spans.
//   layout ld m ...  the layout's fields, one line per (ld, m) pair
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../coordinatedescent.jl_amd/csrc/cox_plan.hpp"

static int fails = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); ++fails; } \
    } while (0)

static int64_t padded(int64_t n) { return (n + 31) / 32 * 32; }
constexpr int64_t kPair2 = (int64_t)kCoxScorePair * kCoxScorePair;

static void layout_case(int64_t ld, int64_t m) {
    const CoxScoreLayout s = cox_score_layout(ld, m);
    const int64_t part = kCoxMaxGrid * cox_score_pair_tiles(m) * 2 * kPair2;
    const std::pair<int64_t, int64_t> spans[] = {{s.e, ld}, {s.ev, ld}, {s.h, ld}, {s.dvk, ld}, {s.wA, ld}, {s.xt, m * ld}, {s.N, m * ld},
                                                 {s.Q, m * ld}, {s.sums, 2 * m * kCoxMaxGrid}, {s.mu, kCoxScoreMaxCols},
                                                 {s.out, 2 * m * ld}, {s.part, part}, {s.info, m * m}};
    int64_t at = 0;
    for (const auto& sp : spans) { EXPECT(sp.first == at); at += sp.second; }
    EXPECT(at == s.doubles);
    EXPECT(m * kCoxScoreCentreRuns <= part);      // the centres' partials, kCoxScoreCentreRuns a column, borrow the head of part
    EXPECT(s.heads == 0 && s.idx == 2 * kCoxMaxGrid && s.ints == 2 * kCoxMaxGrid + kCoxScoreMaxCols);
}

// every pair of columns in exactly one tile, the two maps inverse to each other
static void pair_tiles(int64_t m) {
    const int64_t ct = cox_score_col_tiles(m), npt = cox_score_pair_tiles(m);
    EXPECT(ct * kCoxScorePair >= m && (ct - 1) * kCoxScorePair < m && npt == ct * (ct + 1) / 2);
    std::vector<int> seen((size_t)(m * m), 0);
    for (int64_t t = 0; t < npt; ++t) {
        const CoxScorePair p = cox_score_pair(ct, t);
        EXPECT(0 <= p.ci && p.ci <= p.di && p.di < ct);
        EXPECT(cox_score_pair_index(ct, p.ci, p.di) == t);
        for (int64_t i = 0; i < kCoxScorePair; ++i)
            for (int64_t j = 0; j < kCoxScorePair; ++j) {
                const int64_t c = p.ci * kCoxScorePair + i, d = p.di * kCoxScorePair + j;
                if (c < m && d < m && c <= d) ++seen[(size_t)(c * m + d)];          // k_score_info_sum's condition
            }
    }
    for (int64_t c = 0; c < m; ++c)
        for (int64_t d = 0; d < m; ++d) EXPECT(seen[(size_t)(c * m + d)] == (c <= d ? 1 : 0));
}

// the kernels' writes into the score group, for a call of m columns on a group that holds room for `have`
static void walk(int64_t n, int64_t cap, int64_t m, int64_t have) {
    const int64_t ld = padded(n), cols = cox_score_grow(have, m);
    const CoxPlan pl = cox_plan(ld, cap);
    const CoxScoreLayout s = cox_score_layout(ld, cols);
    std::vector<double> qd((size_t)s.doubles, 0.0);
    std::vector<int32_t> qi((size_t)s.ints, 0);
    double* sums_N = qd.data() + s.sums;
    double* sums_Q = sums_N + cols * kCoxMaxGrid;                       // cox_score_host.hpp's pointers
    double* sch = qd.data() + s.out;
    double* score = sch + cols * ld;
    const int64_t npt = cox_score_pair_tiles(m);
    for (int64_t c = 0; c < m; ++c) { qi[(size_t)(s.idx + c)] += 1; qd[(size_t)(s.mu + c)] += 1.0; }
    for (int64_t b = 0; b < pl.grid; ++b) {
        const int64_t t0 = cox_run_first(pl.tiles, pl.grid, b), t1 = cox_run_first(pl.tiles, pl.grid, b + 1);
        qi[(size_t)(s.heads + b)] += 1;
        qi[(size_t)(s.heads + kCoxMaxGrid + b)] += 1;
        for (int64_t c = 0; c < m; ++c) { sums_N[c * kCoxMaxGrid + b] += 1.0; sums_Q[c * kCoxMaxGrid + b] += 1.0; }
        for (int64_t t = 0; t < npt; ++t)
            for (int64_t i = 0; i < 2 * kPair2; ++i) qd[(size_t)(s.part + (b * npt + t) * 2 * kPair2 + i)] += 1.0;
        for (int64_t t = t0; t < t1; ++t)
            for (int64_t lane = 0; lane < kCoxBlock; ++lane) {
                const int64_t s0 = t * kCoxTile + lane * kCoxPer;
                if (s0 >= ld) continue;
                for (int k = 0; k < kCoxPer; ++k) {
                    const int64_t p = s0 + k;
                    for (int64_t off : {s.e, s.ev, s.h, s.dvk, s.wA}) qd[(size_t)(off + p)] += 1.0;
                    for (int64_t c = 0; c < m; ++c) {
                        for (int64_t off : {s.xt, s.N, s.Q}) qd[(size_t)(off + c * ld + p)] += 1.0;
                        if (p < n) { sch[c * n + p] += 1.0; score[c * n + p] += 1.0; }      // the outputs are n apart
                    }
                }
            }
    }
    for (int64_t c = 0; c < m; ++c)
        for (int64_t d = 0; d < m; ++d) qd[(size_t)(s.info + c * m + d)] += 1.0;
    for (int64_t i = 0; i < 5 * ld; ++i) EXPECT(qd[(size_t)i] == 1.0);
    for (int64_t off : {s.xt, s.N, s.Q})
        for (int64_t i = 0; i < cols * ld; ++i) EXPECT(qd[(size_t)(off + i)] == (i < m * ld ? 1.0 : 0.0));
    for (int64_t a = 0; a < 2; ++a)
        for (int64_t i = 0; i < cols * kCoxMaxGrid; ++i)
            EXPECT(qd[(size_t)(s.sums + a * cols * kCoxMaxGrid + i)] == ((i < m * kCoxMaxGrid && i % kCoxMaxGrid < pl.grid) ? 1.0 : 0.0));
    for (int64_t a = 0; a < 2; ++a)
        for (int64_t i = 0; i < cols * ld; ++i) EXPECT(qd[(size_t)(s.out + a * cols * ld + i)] == (i < m * n ? 1.0 : 0.0));
    for (int64_t i = 0; i < s.info - s.part; ++i) EXPECT(qd[(size_t)(s.part + i)] == (i < pl.grid * npt * 2 * kPair2 ? 1.0 : 0.0));
    for (int64_t i = 0; i < cols * cols; ++i) EXPECT(qd[(size_t)(s.info + i)] == (i < m * m ? 1.0 : 0.0));
    for (int64_t i = 0; i < 2 * kCoxMaxGrid; ++i) EXPECT(qi[(size_t)i] == (i % kCoxMaxGrid < pl.grid ? 1 : 0));
    for (int64_t i = 0; i < kCoxScoreMaxCols; ++i) EXPECT(qi[(size_t)(s.idx + i)] == (i < m ? 1 : 0));
}

int main(int argc, char** argv) {
    if (argc > 3 && !std::strcmp(argv[1], "layout")) {
        for (int i = 2; i + 1 < argc; i += 2) {
            const CoxScoreLayout s = cox_score_layout(std::atoll(argv[i]), std::atoll(argv[i + 1]));
            const int64_t f[] = {s.e, s.ev, s.h, s.dvk, s.wA, s.xt, s.N, s.Q, s.sums, s.mu, s.out, s.part, s.info, s.doubles, s.heads,
                                 s.idx, s.ints};
            static_assert(sizeof f == sizeof(CoxScoreLayout), "every field of CoxScoreLayout is listed");
            for (int64_t v : f) std::printf("%lld ", (long long)v);
            std::printf("\n");
        }
        return 0;
    }
    for (int64_t ld : {(int64_t)32, (int64_t)64, kCoxTile, kCoxTile + 32, 5 * kCoxTile + 32, (int64_t)2000000})
        for (int64_t m = 1; m <= kCoxScoreMaxCols; ++m) layout_case(ld, m);
    for (int64_t m = 1; m <= kCoxScoreMaxCols; ++m) pair_tiles(m);
    for (int64_t have = 0; have <= kCoxScoreMaxCols; ++have)
        for (int64_t m = 1; m <= kCoxScoreMaxCols; ++m) {
            const int64_t g = cox_score_grow(have, m);
            EXPECT(g >= have && g >= m && (g == have || g == m));
            EXPECT(cox_score_layout(4096, g).doubles >= cox_score_layout(4096, have).doubles);
        }
    for (int64_t n : {(int64_t)1, (int64_t)65, kCoxTile + 1, 5 * kCoxTile + 3})
        for (int64_t cap : {(int64_t)2, kCoxMaxGrid})
            for (int64_t m : {(int64_t)1, (int64_t)3, (int64_t)5, (int64_t)64})
                for (int64_t have : {(int64_t)0, (int64_t)9, (int64_t)64}) {
                    // (a group of 64 columns holds 35 MB of partials: walked at two sizes only)
                    if (cox_score_grow(have, m) == 64 && !(n == 65 || (n == 5 * kCoxTile + 3 && cap == 2 && have == 0))) continue;
                    walk(n, cap, m, have);
                }
    if (fails) { std::printf("cox_score_plan_main: %d FAILED\n", fails); return 1; }
    std::printf("cox_score_plan_main OK pair=%d cols=%d\n", kCoxScorePair, kCoxScoreMaxCols);
    return 0;
}
