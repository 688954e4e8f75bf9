// Stand-alone check of csrc/solve_plan.hpp, built with -fsanitize=address,undefined by tests/test_solve_plan_host.py: the grid
// writes exactly numSteps + 1 doubles and its last one is exp(log(target)), the lambda_max reduction reads exactly p strided
// values (the sanitizer watches the arrays' ends), the walk tiles [0, m) with steps inside their bounds whatever the hits, the
// limit form of the rows-per-non-zero rule is its product form, and the pass loop's rule is the four lines it replaced.
#include <stdio.h>
#include <stdlib.h>

#include <cmath>
#include <limits>
#include <vector>

#include "../coordinatedescent.jl_amd/csrc/solve_plan.hpp"

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { if (++g_bad < 20) fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static_assert(kScreen == 64 && kScreenMax == 1024 && kScreenMinPass == 16, "");
static_assert(screen_gate(1, false, false, 16, 4, 16) && !screen_gate(1, false, false, 15, 0, 15) && !screen_gate(1, false, false, 16, 5, 16), "");
static_assert(!screen_gate(0, false, false, 700, 0, 700) && !screen_gate(1, true, false, 700, 0, 700) && screen_gate(2, true, true, 700, 175, 700), "");
static_assert(rows_support_limit(3000, 32, false) == 93 && rows_support_limit(3000, 32, true) == kNoSupportLimit, "");

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33); }

// one walk with a mover every so often (per_mille of the visits); returns the screens' lengths
static std::vector<int> walk_once(int64_t m, int B, int64_t cap, int64_t p, unsigned per_mille, long* steps) {
    std::vector<unsigned char> mover((size_t)m);            // exactly m long: a step past the pass reads past it
    for (auto& v : mover) v = rnd() % 1000 < per_mille;
    std::vector<int> screens;
    ScreenWalk walk(m, B, cap, p);
    int64_t next = 0;
    while (!walk.done()) {
        const ScreenStep s = walk.next();
        ++*steps;
        EXPECT(s.pos == next && s.len >= 1 && s.pos + s.len <= m);
        if (!s.screen) { EXPECT(s.len <= cap); next += s.len; continue; }
        EXPECT(s.len <= std::min<int64_t>(kScreenMax, p) && s.len <= cap);
        int hit = s.len;
        for (int i = 0; i < s.len; ++i) if (mover[(size_t)(s.pos + i)]) { hit = i; break; }
        walk.hit(hit);
        screens.push_back(s.len);
        next += hit;
        if (hit < s.len) EXPECT(!walk.done());              // the visit that can move is still to come
    }
    EXPECT(next == m);
    return screens;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    // ---- the grid ----
    long grids = 0;
    for (int64_t numSteps : {1, 2, 50}) for (double lmax : {0.0, 1e-300, 0.37, 1.0, 12.5, 1e300, inf, (double)NAN})
        for (double target : {0.0, 1e-3, 0.37, 0.37000000000000005, 1.0, 12.5, 40.0, inf, (double)NAN}) {
            std::vector<double> g((size_t)numSteps + 1, -1.0);
            const double step = (std::log(target) - std::log(lmax)) / (double)numSteps;
            const bool ok = cold_start_grid(lmax, target, numSteps, g.data());
            EXPECT(ok == !(step == 0.0 || step != step));
            if (!ok) continue;
            ++grids;
            const double last = std::exp(std::log(target));
            EXPECT(g[(size_t)numSteps] == last || (last != last && g[(size_t)numSteps] != g[(size_t)numSteps]));
            if (lmax > 0.0 && lmax < inf && target > 0.0 && target < inf) {
                EXPECT(g[0] == std::exp(std::log(lmax)));
                for (int64_t j = 0; j < numSteps; ++j) EXPECT(target < lmax ? g[(size_t)j] >= g[(size_t)j + 1] : g[(size_t)j] <= g[(size_t)j + 1]);
            }
        }
    // ---- lambda_max ----
    for (int64_t stride : {1, 2}) for (int64_t p : {1, 7, 64}) {
        std::vector<double> v((size_t)((p - 1) * stride + 1)), om((size_t)p);      // no entry behind the last dot
        for (auto& x : v) x = (double)rnd() / 65536.0 - 16000.0;
        for (auto& x : om) x = 0.5 + (double)(rnd() % 1000) / 1000.0;
        double want = 0.0, want_om = 0.0;
        for (int64_t k = 0; k < p; ++k) {
            want = std::max(want, std::fabs(v[(size_t)(k * stride)] / 3.0));
            want_om = std::max(want_om, std::fabs(v[(size_t)(k * stride)] / 3.0) / om[(size_t)k]);
        }
        EXPECT(lambda_max_of(v.data(), stride, p, 3.0, nullptr) == want && lambda_max_of(v.data(), stride, p, 3.0, om.data()) == want_om);
        v[0] = NAN;                                           // a NaN never wins
        const double rest = lambda_max_of(v.data(), stride, p, 3.0, nullptr);
        EXPECT(rest == rest && rest <= want);
        om[(size_t)(p - 1)] = 0.0;                            // a zero omega does: inf (0 / 0 apart)
        if (p > 1) EXPECT(lambda_max_of(v.data(), stride, p, 3.0, om.data()) == inf);
    }
    // ---- the walk ----
    long walks = 0, steps = 0;
    for (int64_t p : {16, 17, 63, 64, 65, 191, 192, 193, 1024, 1025, 2500, 5000}) for (int B : {1, 8, 16, 32, 64})
        for (int64_t m : {p, p + 1, 2 * p + 3, 3 * p}) for (unsigned per_mille : {0u, 10u, 100u, 500u, 1000u}) {
            const int64_t cap = std::max<int64_t>(p, 4096);
            const std::vector<int> screens = walk_once(m, B, cap, p, per_mille, &steps);
            ++walks;
            if (per_mille == 0 && m == p && p == 5000) EXPECT((screens == std::vector<int>{64, 128, 256, 512, 1024, 1024, 1024, 968}));
            if (per_mille == 1000) EXPECT(screens.size() <= 2 + (size_t)std::log2((double)m));     // a handful of screens, each a miss
        }
    // a cap below the longest screen bounds the screens too (the handle's is max(p, 4096); the visit after a hit streams
    // max(B, 1) whatever the cap, so B <= cap here as there)
    for (int64_t cap : {16, 40, 64, 100}) walk_once(700, 16, cap, 700, 30, &steps);
    // ---- the rows-per-non-zero rule: nnz > n / r  <=>  nnz * r > n ----
    for (int64_t r : {1, 2, 32, 400}) for (int64_t n : {1, 31, 32, 33, 399, 400, 401, 3000, 10000019})
        for (int64_t d = -3; d <= 3; ++d) {
            const int64_t nnz = n / r + d;
            if (nnz < 0) continue;
            EXPECT((nnz > rows_support_limit(n, r, false)) == (nnz * r > n));
            EXPECT(!(nnz > rows_support_limit(n, r, true)));
        }
    // ---- the pass loop's rule ----
    for (int len = 1; len <= 6; ++len) for (int bits = 0; bits < (1 << len); ++bits) {
        SolveProgress at;
        bool prev = false, conv = true;
        int64_t iter = 0;
        for (int k = 0; k < len; ++k) {
            const double maxH = (bits >> k & 1) ? 1e-13 : 1e-3;
            const bool done = at.pass_done(maxH, 1e-12);
            prev = conv; conv = maxH < 1e-12; ++iter;
            EXPECT(at.prev_converged == prev && at.converged == conv && at.iter == iter && done == (prev && conv));
            if (done) break;
        }
    }
    { SolveProgress at; EXPECT(!at.pass_done(NAN, 1e-12) && !at.converged && at.prev_converged); }      // a NaN is not below optTol
    if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    printf("solve_plan_main OK (%ld grids, %ld walks, %ld steps)\n", grids, walks, steps);
    return 0;
}
