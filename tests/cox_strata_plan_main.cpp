// Stand-alone check of the strata-aware part of csrc/cox_plan.hpp (tests/test_cox_strata_plan_host.py builds and runs it under
// the host sanitizers).
//   no arguments        for n in 1 .. 2100 and around the tile multiples, under every strata pattern (one stratum, two, sizes
//                       1..7 cycling, every row its own, ids that are negative or INT32_MAX) and times with and without ties:
//                       cox_order_strata's five vectors are held to their definition -- a permutation sorted by (stratum,
//                       time), stable, every bound the true one, the pads one stratum in place -- without strata the first three
//                       are cox_order's; then the second pair of buffers is walked the way the kernels walk it, over
//                       exactly-sized heap blocks (a lane that leaves its block is an ASan report).
//   order t g t g ...   (pairs "time stratum") order, first, last, sfirst, slast, one line each
//   check t s o w ...   (quadruples "time status offset weight") cox_check's verdict: "ok" or its message
//   layout ld ...       the layout's fields of the second pair, one line per ld
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../coordinatedescent.jl_amd/csrc/cox_plan.hpp"

static int fails = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); ++fails; } \
    } while (0)

static int64_t padded(int64_t n) { return (n + 31) / 32 * 32; }

// a small generator of its own: the cases must not depend on the C library's rand
static uint64_t lcg(uint64_t& s) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return s >> 33; }

static std::vector<int32_t> pattern(int which, int64_t n) {
    std::vector<int32_t> g((size_t)n, 0);
    uint64_t seed = 77 + (uint64_t)n;
    for (int64_t i = 0, size = 1, left = 1, id = 0; i < n; ++i) {
        switch (which) {
            case 0: g[(size_t)i] = 0; break;                                        // one stratum
            case 1: g[(size_t)i] = (int32_t)(lcg(seed) & 1); break;                 // two, interleaved in the caller's order
            case 2:                                                                 // sizes 1..7 cycling, ids descending
                g[(size_t)i] = (int32_t)(1000 - id);
                if (--left == 0) { size = size % 7 + 1; left = size; ++id; }
                break;
            case 3: g[(size_t)i] = (int32_t)((i * 7919) % n); break;                // every row its own (7919 is prime)
            default: {                                                              // negative ids and INT32_MAX
                const int32_t ids[] = {INT32_MIN, -5, 0, INT32_MAX};
                g[(size_t)i] = ids[lcg(seed) % 4];
            }
        }
    }
    return g;
}

static void order_case(int64_t n, int which, bool ties) {
    const int64_t ld = padded(n);
    uint64_t seed = 1234 + (uint64_t)n * 5 + (uint64_t)which;
    std::vector<double> t((size_t)n);
    for (auto& v : t) v = ties ? (double)(lcg(seed) % 9) * 0.5 : (double)lcg(seed) / 1024.0;
    const std::vector<int32_t> g = pattern(which, n);
    std::vector<int32_t> order, first, last, sfirst, slast;
    cox_order_strata(n, ld, t.data(), g.data(), order, first, last, sfirst, slast);
    for (const auto* v : {&order, &first, &last, &sfirst, &slast}) EXPECT((int64_t)v->size() == ld);
    std::vector<unsigned char> seen((size_t)ld, 0);
    for (int64_t s = 0; s < ld; ++s) {
        EXPECT(order[s] >= 0 && order[s] < ld);
        ++seen[(size_t)order[s]];
    }
    for (int64_t s = 0; s < ld; ++s) EXPECT(seen[(size_t)s] == 1);
    for (int64_t s = 1; s < n; ++s) {
        const int32_t a = order[s - 1], b = order[s];
        EXPECT(g[a] < g[b] || (g[a] == g[b] && (t[a] < t[b] || (t[a] == t[b] && a < b))));      // sorted, and stable
    }
    for (int64_t s = 0; s < n; ++s) {
        const int32_t f = first[s], l = last[s], sf = sfirst[s], sl = slast[s];
        EXPECT(0 <= sf && sf <= f && f <= s && s <= l && l <= sl && sl < n);
        if (!(0 <= sf && sf <= f && f <= s && s <= l && l <= sl && sl < n)) continue;
        EXPECT(g[order[sf]] == g[order[s]] && g[order[sl]] == g[order[s]]);
        EXPECT(sf == 0 || g[order[sf - 1]] != g[order[s]]);
        EXPECT(sl == n - 1 || g[order[sl + 1]] != g[order[s]]);
        EXPECT(t[order[f]] == t[order[s]] && t[order[l]] == t[order[s]]);
        EXPECT(f == sf || t[order[f - 1]] != t[order[s]]);
        EXPECT(l == sl || t[order[l + 1]] != t[order[s]]);
    }
    for (int64_t s = n; s < ld; ++s)
        EXPECT(order[s] == s && first[s] == s && last[s] == s && sfirst[s] == n && slast[s] == ld - 1);
    if (which == 0) {
        // one stratum, and no strata at all: the first three vectors are cox_order's, element for element
        std::vector<int32_t> o2, f2, l2, o3, f3, l3, sf3, sl3;
        cox_order(n, ld, t.data(), o2, f2, l2);
        cox_order_strata(n, ld, t.data(), nullptr, o3, f3, l3, sf3, sl3);
        EXPECT(o2 == order && f2 == first && l2 == last && o3 == order && f3 == first && l3 == last && sf3 == sfirst && sl3 == slast);
        for (int64_t s = 0; s < n; ++s) EXPECT(sfirst[s] == 0 && slast[s] == n - 1);
    }
}

// the kernels' reads and writes of the second pair: per run the bound of its first / last position and a flag in each of
// the two flag arrays; per position sfirst, slast and the weight of its row
static void walk(int64_t n, int64_t cap) {
    const int64_t ld = padded(n);
    const CoxPlan pl = cox_plan(ld, cap);
    const CoxLayout lay = cox_layout(ld);
    EXPECT(lay.sfirst == 0 && lay.slast == ld && lay.strata == 2 * ld && lay.heads == 3 * ld);
    EXPECT(lay.strata_ints == 3 * ld + 2 * kCoxMaxGrid && lay.weight == 0 && lay.strata_doubles == ld);
    std::vector<int32_t> si((size_t)lay.strata_ints, 0);
    std::vector<double> sd((size_t)lay.strata_doubles, 0.0);
    for (int64_t b = 0; b < pl.grid; ++b) {
        const int64_t t0 = cox_run_first(pl.tiles, pl.grid, b), t1 = cox_run_first(pl.tiles, pl.grid, b + 1);
        const int64_t lo = t0 * kCoxTile, hi = (t1 * kCoxTile < ld ? t1 * kCoxTile : ld) - 1;
        EXPECT(lo >= 0 && lo <= hi && hi < ld);
        si[(size_t)(lay.slast + lo)] += 0;                       // k_cox_exp reads the run's first position's stratum end
        si[(size_t)(lay.sfirst + hi)] += 0;                      // k_cox_hazard the run's last position's stratum start
        si[(size_t)(lay.heads + b)] += 1;
        si[(size_t)(lay.heads + kCoxMaxGrid + b)] += 1;
        for (int64_t t = t0; t < t1; ++t)
            for (int64_t lane = 0; lane < kCoxBlock; ++lane) {
                const int64_t s0 = t * kCoxTile + lane * kCoxPer;
                if (s0 >= ld) continue;
                for (int c = 0; c < kCoxPer; ++c) {
                    si[(size_t)(lay.sfirst + s0 + c)] += 1;
                    si[(size_t)(lay.slast + s0 + c)] += 1;
                    si[(size_t)(lay.strata + s0 + c)] += 1;
                    sd[(size_t)(lay.weight + s0 + c)] += 1.0;
                }
            }
    }
    for (int64_t i = 0; i < 3 * ld; ++i) EXPECT(si[(size_t)i] == 1);
    for (int64_t i = 0; i < ld; ++i) EXPECT(sd[(size_t)i] == 1.0);
    for (int64_t b = 0; b < 2 * kCoxMaxGrid; ++b) EXPECT(si[(size_t)(lay.heads + b)] == ((b % kCoxMaxGrid) < pl.grid ? 1 : 0));
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "order")) {
        std::vector<double> t;
        std::vector<int32_t> g;
        for (int a = 2; a + 1 < argc; a += 2) {
            t.push_back(std::strtod(argv[a], nullptr));
            g.push_back((int32_t)std::strtoll(argv[a + 1], nullptr, 10));
        }
        const int64_t n = (int64_t)t.size();
        std::vector<int32_t> order, first, last, sfirst, slast;
        cox_order_strata(n, padded(n), t.data(), g.data(), order, first, last, sfirst, slast);
        for (const auto* v : {&order, &first, &last, &sfirst, &slast}) {
            for (int64_t s = 0; s < padded(n); ++s) std::printf("%d ", (int)(*v)[(size_t)s]);
            std::printf("\n");
        }
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "check")) {
        std::vector<double> t, s, o, w;
        for (int a = 2; a + 3 < argc; a += 4) {
            t.push_back(std::strtod(argv[a], nullptr));
            s.push_back(std::strtod(argv[a + 1], nullptr));
            o.push_back(std::strtod(argv[a + 2], nullptr));
            w.push_back(std::strtod(argv[a + 3], nullptr));
        }
        char msg[128];
        const bool ok = cox_check((int64_t)t.size(), t.data(), s.data(), o.data(), msg, sizeof msg, w.data());
        std::printf("%s\n", ok ? "ok" : msg);
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "layout")) {
        for (int a = 2; a < argc; ++a) {
            const CoxLayout lay = cox_layout(std::atoll(argv[a]));
            std::printf("%lld %lld %lld %lld %lld %lld %lld\n", (long long)lay.sfirst, (long long)lay.slast, (long long)lay.strata,
                        (long long)lay.heads, (long long)lay.strata_ints, (long long)lay.weight, (long long)lay.strata_doubles);
        }
        return 0;
    }
    for (int which = 0; which < 5; ++which)
        for (int ties = 0; ties < 2; ++ties) {
            for (int64_t n = 1; n <= 2100; n += (n < 130 ? 1 : 31)) order_case(n, which, ties != 0);
            const int64_t around[] = {kCoxTile, 2 * kCoxTile};
            for (int64_t m : around)
                for (int64_t dd = -33; dd <= 33; dd += 11) order_case(m + dd, which, ties != 0);
        }
    const int64_t caps[] = {kCoxMaxGrid, 1, 2, 3};
    for (int64_t cap : caps) {
        for (int64_t n = 1; n <= 2100; n += (n < 130 ? 1 : 31)) walk(n, cap);
        for (int64_t m : {kCoxTile, 2 * kCoxTile, 5 * kCoxTile})
            for (int64_t dd = -33; dd <= 33; dd += 11) walk(m + dd, cap);
    }
    // hand-made: strata in ascending id order whatever the caller's order, ties inside a stratum only
    {
        const double t[] = {2.0, 1.0, 2.0, 1.0, 2.0, 3.0};
        const int32_t g[] = {5, -1, 5, 5, -1, 5};
        std::vector<int32_t> order, first, last, sfirst, slast;
        cox_order_strata(6, 32, t, g, order, first, last, sfirst, slast);
        const int32_t o[] = {1, 4, 3, 0, 2, 5}, f[] = {0, 1, 2, 3, 3, 5}, l[] = {0, 1, 2, 4, 4, 5}, sf[] = {0, 0, 2, 2, 2, 2},
                      sl[] = {1, 1, 5, 5, 5, 5};
        for (int s = 0; s < 6; ++s)
            EXPECT(order[s] == o[s] && first[s] == f[s] && last[s] == l[s] && sfirst[s] == sf[s] && slast[s] == sl[s]);
        EXPECT(sfirst[6] == 6 && slast[6] == 31 && sfirst[31] == 6 && slast[31] == 31 && first[31] == 31);
    }
    std::printf(fails ? "cox_strata_plan_main: %d FAILED\n" : "cox_strata_plan_main OK tile=%d\n", fails ? fails : (int)kCoxTile);
    return fails ? 1 : 0;
}
