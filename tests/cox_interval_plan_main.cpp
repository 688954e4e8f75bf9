// Stand-alone check of the start-stop part of csrc/cox_plan.hpp (tests/test_cox_interval_plan_host.py builds and runs it under
// the host sanitizers).
//   no arguments          for n = 1, 2, 65, 1025 and more, under strata patterns and starts with and without ties (among them
//                         starts equal to other rows' stops): cox_order_interval's first five vectors are cox_order_strata's on
//                         the stop times, order2 is a stable sort by (stratum, start), pos2 its positions in the stop order, lo
//                         and enter equal a brute-force search inside the stratum, the pads stay in place with lo = enter = -1;
//                         then the third pair of buffers is walked the way the kernels walk it, over exactly-sized heap blocks.
//   order a b g a b g ... (triples "start stop stratum") order, first, last, sfirst, slast, order2, pos2, lo, enter, one line each
//   check a b a b ...     (pairs "start stop") cox_check_interval's verdict: "ok" or its message
//   layout ld ...         the layout's fields of the third pair, one line per ld
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
static uint64_t lcg(uint64_t& s) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return s >> 33; }

struct Vectors { std::vector<int32_t> order, first, last, sfirst, slast, order2, pos2, lo, enter; };

static Vectors run(int64_t n, const double* a, const double* b, const int32_t* g) {
    Vectors v;
    cox_order_interval(n, padded(n), a, b, g, v.order, v.first, v.last, v.sfirst, v.slast, v.order2, v.pos2, v.lo, v.enter);
    return v;
}

// which: 0 one stratum, 1 two interleaved, 2 sizes 1..7 cycling with descending ids, 3 one stratum WITHOUT strata (nullptr);
// ties: times on a grid of halves, so that starts coincide with stops of other rows and with each other
static void order_case(int64_t n, int which, bool ties) {
    const int64_t ld = padded(n);
    uint64_t seed = 4321 + (uint64_t)n * 7 + (uint64_t)which;
    std::vector<double> a((size_t)n), b((size_t)n);
    std::vector<int32_t> g((size_t)n, 0);
    for (int64_t i = 0, size = 1, left = 1, id = 0; i < n; ++i) {
        if (ties) {
            b[(size_t)i] = 0.5 * (double)(1 + lcg(seed) % 9);
            a[(size_t)i] = 0.5 * (double)(lcg(seed) % (uint64_t)(2.0 * b[(size_t)i]));
        } else {
            b[(size_t)i] = 1.0 + (double)lcg(seed) / 1024.0;
            a[(size_t)i] = b[(size_t)i] * (double)(lcg(seed) % 1000) / 1000.0;
        }
        if (which == 1) g[(size_t)i] = (int32_t)(lcg(seed) & 1);
        if (which == 2) {
            g[(size_t)i] = (int32_t)(1000 - id);
            if (--left == 0) { size = size % 7 + 1; left = size; ++id; }
        }
    }
    const int32_t* gp = which == 3 ? nullptr : g.data();
    const Vectors v = run(n, a.data(), b.data(), gp);
    std::vector<int32_t> order, first, last, sfirst, slast;
    cox_order_strata(n, ld, b.data(), gp, order, first, last, sfirst, slast);
    EXPECT(order == v.order && first == v.first && last == v.last && sfirst == v.sfirst && slast == v.slast);
    for (const auto* x : {&v.order2, &v.pos2, &v.lo, &v.enter}) EXPECT((int64_t)x->size() == ld);
    std::vector<unsigned char> seen((size_t)ld, 0);
    for (int64_t s = 0; s < ld; ++s) {
        EXPECT(v.order2[s] >= 0 && v.order2[s] < ld);
        ++seen[(size_t)v.order2[s]];
        EXPECT(v.pos2[s] >= 0 && v.pos2[s] < ld && v.order[v.pos2[s]] == v.order2[s]);
    }
    for (int64_t s = 0; s < ld; ++s) EXPECT(seen[(size_t)s] == 1);
    for (int64_t s = 1; s < n; ++s) {
        const int32_t p = v.order2[s - 1], q = v.order2[s];
        EXPECT(g[p] < g[q] || (g[p] == g[q] && (a[p] < a[q] || (a[p] == a[q] && p < q))));          // sorted, and stable
    }
    for (int64_t s = 0; s < n; ++s) {
        EXPECT(g[v.order2[s]] == g[v.order[s]]);                 // a stratum holds the same positions in both orders
        const int64_t sa = v.sfirst[s], sb = v.slast[s];
        const double t = b[v.order[s]], u = a[v.order[s]];
        int64_t lo = -1, enter = -1;                             // brute force, inside the stratum only
        for (int64_t q = sb; q >= sa; --q) if (a[v.order2[q]] >= t) lo = q;
        for (int64_t q = sa; q <= sb; ++q) if (b[v.order[q]] <= u) enter = q;
        EXPECT(v.lo[s] == lo);
        EXPECT(v.enter[s] == enter);
        EXPECT(v.enter[s] < v.first[s]);                         // start < stop: the row enters before its own tie group
        EXPECT(v.enter[s] < 0 || v.last[v.enter[s]] == v.enter[s]);      // and at a tie group's end
    }
    for (int64_t s = n; s < ld; ++s) EXPECT(v.order2[s] == s && v.pos2[s] == s && v.lo[s] == -1 && v.enter[s] == -1);
}

// the kernels' reads and writes of the third pair: per run a record of the second scan; per position pos2, lo, enter, T2 and
// the start; every lookup that is not -1 lies inside 0 .. ld - 1
static void walk(int64_t n, int64_t cap) {
    const int64_t ld = padded(n);
    const CoxPlan pl = cox_plan(ld, cap);
    const CoxLayout lay = cox_layout(ld);
    EXPECT(lay.pos2 == 0 && lay.lo == ld && lay.enter == 2 * ld && lay.heads2 == 3 * ld && lay.interval_ints == 3 * ld + kCoxMaxGrid);
    EXPECT(lay.start == 0 && lay.T2 == ld && lay.sums2 == 2 * ld && lay.interval_doubles == 2 * ld + kCoxMaxGrid);
    std::vector<int32_t> vi((size_t)lay.interval_ints, 0);
    std::vector<double> vd((size_t)lay.interval_doubles, 0.0);
    for (int64_t b = 0; b < pl.grid; ++b) {
        const int64_t t0 = cox_run_first(pl.tiles, pl.grid, b), t1 = cox_run_first(pl.tiles, pl.grid, b + 1);
        vi[(size_t)(lay.heads2 + b)] += 1;
        vd[(size_t)(lay.sums2 + b)] += 1.0;
        for (int64_t t = t0; t < t1; ++t)
            for (int64_t lane = 0; lane < kCoxBlock; ++lane) {
                const int64_t s0 = t * kCoxTile + lane * kCoxPer;
                if (s0 >= ld) continue;
                for (int c = 0; c < kCoxPer; ++c) {
                    vi[(size_t)(lay.pos2 + s0 + c)] += 1;
                    vi[(size_t)(lay.lo + s0 + c)] += 1;
                    vi[(size_t)(lay.enter + s0 + c)] += 1;
                    vd[(size_t)(lay.T2 + s0 + c)] += 1.0;
                    vd[(size_t)(lay.start + s0 + c)] += 1.0;
                }
            }
    }
    for (int64_t i = 0; i < 3 * ld; ++i) EXPECT(vi[(size_t)i] == 1);
    for (int64_t i = 0; i < 2 * ld; ++i) EXPECT(vd[(size_t)i] == 1.0);
    for (int64_t b = 0; b < kCoxMaxGrid; ++b) {
        EXPECT(vi[(size_t)(lay.heads2 + b)] == (b < pl.grid ? 1 : 0));
        EXPECT(vd[(size_t)(lay.sums2 + b)] == (b < pl.grid ? 1.0 : 0.0));
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "order")) {
        std::vector<double> a, b;
        std::vector<int32_t> g;
        for (int i = 2; i + 2 < argc; i += 3) {
            a.push_back(std::strtod(argv[i], nullptr));
            b.push_back(std::strtod(argv[i + 1], nullptr));
            g.push_back((int32_t)std::strtoll(argv[i + 2], nullptr, 10));
        }
        const int64_t n = (int64_t)a.size();
        const Vectors v = run(n, a.data(), b.data(), g.data());
        for (const auto* x : {&v.order, &v.first, &v.last, &v.sfirst, &v.slast, &v.order2, &v.pos2, &v.lo, &v.enter}) {
            for (int64_t s = 0; s < padded(n); ++s) std::printf("%d ", (int)(*x)[(size_t)s]);
            std::printf("\n");
        }
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "check")) {
        std::vector<double> a, b;
        for (int i = 2; i + 1 < argc; i += 2) {
            a.push_back(std::strtod(argv[i], nullptr));
            b.push_back(std::strtod(argv[i + 1], nullptr));
        }
        char msg[160];
        const bool ok = cox_check_interval((int64_t)a.size(), a.data(), b.data(), msg, sizeof msg);
        std::printf("%s\n", ok ? "ok" : msg);
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "layout")) {
        for (int i = 2; i < argc; ++i) {
            const CoxLayout lay = cox_layout(std::atoll(argv[i]));
            std::printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)lay.pos2, (long long)lay.lo, (long long)lay.enter,
                        (long long)lay.heads2, (long long)lay.interval_ints, (long long)lay.start, (long long)lay.T2,
                        (long long)lay.sums2, (long long)lay.interval_doubles);
        }
        return 0;
    }
    for (int which = 0; which < 4; ++which)
        for (int ties = 0; ties < 2; ++ties) {
            for (int64_t n = 1; n <= 130; ++n) order_case(n, which, ties != 0);
            for (int64_t n : {kCoxTile - 1, kCoxTile, kCoxTile + 1, 2 * kCoxTile + 1, (int64_t)2100}) order_case(n, which, ties != 0);
        }
    const int64_t caps[] = {kCoxMaxGrid, 1, 2, 3};
    for (int64_t cap : caps)
        for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)65, kCoxTile - 1, kCoxTile + 1, 2 * kCoxTile + 1, 5 * kCoxTile + 3}) walk(n, cap);
    // hand-made.  Stratum -1 (rows 1, 4) holds the SMALLER stops; row 0 of stratum 5 starts below every stop of its own stratum
    // but above those of stratum -1: a lookup that leaks across the boundary would give it enter = 1.  Row 2 starts at 2.0, the
    // stop (an event time) of row 3: it is not at risk there -- enter points at that stop, and lo of that stop at row 2's start.
    // Rows 2 and 5 tie in start.
    {
        const double a[] = {1.5, 0.0, 2.0, 0.5, 0.25, 2.0};
        const double b[] = {3.0, 1.0, 4.0, 2.0, 1.25, 2.5};
        const int32_t g[] = {5, -1, 5, 5, -1, 5};
        const Vectors v = run(6, a, b, g);
        const int32_t o[] = {1, 4, 3, 5, 0, 2}, o2[] = {1, 4, 3, 0, 2, 5}, p2[] = {0, 1, 2, 4, 5, 3};
        const int32_t lo[] = {-1, -1, 4, -1, -1, -1}, en[] = {-1, -1, -1, 2, -1, 2};
        for (int s = 0; s < 6; ++s) {
            EXPECT(v.order[s] == o[s]);
            EXPECT(v.order2[s] == o2[s]);
            EXPECT(v.pos2[s] == p2[s]);
            EXPECT(v.lo[s] == lo[s]);
            EXPECT(v.enter[s] == en[s]);
        }
        EXPECT(v.lo[6] == -1 && v.enter[31] == -1 && v.order2[31] == 31 && v.pos2[6] == 6);
    }
    std::printf(fails ? "cox_interval_plan_main: %d FAILED\n" : "cox_interval_plan_main OK tile=%d\n", fails ? fails : (int)kCoxTile);
    return fails ? 1 : 0;
}
