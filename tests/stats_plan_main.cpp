// Stand-alone check of csrc/stats_plan.hpp, built with -fsanitize=address,undefined by tests/test_stats_plan_host.py: the
// launches of a Gram block hold 1 .. 64 distinct columns of the call's list for every m, the scatter stays inside a record, an
// m x m matrix and m dots that are exactly that long (the sanitizer watches their ends) and writes every entry, and the batches
// of a varying-coefficient point tile the expanded columns with partials that fit what cdh_create allocates.
#include <stdio.h>
#include <stdlib.h>

#include <cmath>
#include <vector>

#include "../coordinatedescent.jl_amd/csrc/stats_plan.hpp"

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { if (++g_bad < 20) fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

// compile time: the plan is constexpr, and these are the numbers the comments quote
static_assert(gram_launches(64) == 1 && gram_launches(65) == 3 && gram_launches(4096) == 128 * 127 / 2, "");
static_assert(gram_launch_at(65, 2).a0 == 32 && gram_launch_at(65, 2).b0 == 64 && gram_launch_at(65, 2).nb == 1, "");
static_assert(gs_g(0, 0) == 0 && gs_g(15, 15) == 255 && gs_g(0, 16) == 256 && gs_g(63, 63) == kGsOffC - 1 && kGsRec == 2625, "");
static_assert(vc_batches(4096) == 1 && vc_batches(4098) == 2 && vc_batch(4098, 2, 2502, 256, false, 0).jb1 == 1366 &&
              vc_batch(4098, 2, 2502, 256, false, 1).jb0 == 1365, "the last group of p = 4098 at degree 2 is in both batches");
static_assert(vc_point_launches(4098, 0) == 1 && vc_point_launches(4098, 2) == 3, "");

int main() {
    long launches = 0;
    for (int64_t m = 1; m <= kGramMaxCols; ++m) {
        const int64_t nl = gram_launches(m), ng = (m + 31) / 32;
        EXPECT(nl == (m <= 64 ? 1 : ng * (ng - 1) / 2));
        const bool replay = m <= 200 || m == 4065 || m == 4095 || m == 4096;
        std::vector<double> rec, G, c;
        if (replay) { rec.assign((size_t)kGsRec, 1.0); G.assign((size_t)(m * m), NAN); c.assign((size_t)m, NAN); }
        for (int64_t t = 0; t < nl; ++t, ++launches) {
            const GramLaunch L = gram_launch_at(m, t);
            EXPECT(L.cols() >= 1 && L.cols() <= kGramLaunchCols && L.na >= 1 && L.nb >= 0);
            EXPECT(L.col_of(0) >= 0 && L.col_of(L.cols() - 1) < m && L.a0 + L.na <= L.b0);     // ascending and inside the list: distinct
            if (!replay) continue;
            double q = NAN;
            gram_scatter(L, m, rec.data(), G.data(), c.data(), &q);
            gram_scatter(L, m, rec.data(), G.data(), nullptr, nullptr);
            EXPECT(q == 1.0);
        }
        if (!replay) continue;
        bool all = true;
        for (double v : G) all = all && v == 1.0;
        for (double v : c) all = all && v == 1.0;
        EXPECT(all);
    }
    long batches = 0;
    for (int cus : {1, 8, 64, 256, 304, 1024}) for (int f64 = 0; f64 < 2; ++f64) for (int64_t n : {1, 33, 513, 5003, 300000, 10000019})
        for (int degree = 1; degree <= 3; ++degree) for (int64_t k = 1; k <= 3; ++k) for (int64_t d = -8; d <= 8; ++d) {
            const int64_t Q1 = degree + 1, p = (4096 * k + d) / Q1 * Q1;
            const SweepSizes s = sweep_sizes(f64, n, p, cus);
            int64_t next = 0;
            for (int64_t t = 0; t < vc_batches(p); ++t, ++batches) {
                const VcBatch B = vc_batch(p, degree, s.nvec, cus, true, t);
                EXPECT(B.b0 == next && B.b1 > B.b0 && B.b1 - B.b0 <= kSpColBatch);
                EXPECT(B.jb0 * Q1 <= B.b0 && B.b0 < (B.jb0 + 1) * Q1 && (B.jb1 - 1) * Q1 < B.b1 && B.b1 <= B.jb1 * Q1);
                EXPECT(B.chunks >= 1 && B.chunks <= kSpColChunks && B.partials == 2 * B.table && B.partials <= s.partials_doubles);
                EXPECT(vc_batch(p, degree, s.nvec, cus, false, t).partials == B.table);
                next = B.b1;
            }
            EXPECT(next == p && vc_point_launches(p, degree) == 1 + vc_batches(p));
        }
    if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    printf("stats_plan_main OK (%ld Gram launches, %ld batches)\n", launches, batches);
    return 0;
}
