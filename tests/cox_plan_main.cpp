// Stand-alone check of csrc/cox_plan.hpp (tests/test_cox_plan_host.py builds and runs it under the host sanitizers).
//   no arguments      for n in 1 .. 2100 and around every constant of the plan, at the full grid cap and at small ones, the
//                     workgroups' runs are walked the way the Cox kernels walk them over exactly-sized heap blocks -- a lane that
//                     leaves its block is an ASan report -- and must cover every position of [0, ld) exactly once, every tile in
//                     exactly one run; then the time order and the tie groups of small hand-made cases.
//   plan ld cap ...   the plan, the runs' first tiles at b = 0, 1, grid - 1, grid, and the layout of each pair, one line each,
//                     for tests/_cox_plan.py to be held to (no memory is touched: ld may be 2^31 - 32)
//   runs ld cap ...   per pair one line: tiles, grid, then the first tile of every run b = 0 .. grid (grid + 1 figures)
//   order t0 t1 ...   order, first and last of the given times, one line each
//   check t s [o] ... (triples "time status offset") cox_check's verdict: "ok" or its message
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

static void walk(int64_t n, int64_t cap) {
    const int64_t ld = padded(n);
    const CoxPlan pl = cox_plan(ld, cap);
    const int64_t c = cox_grid_cap(cap);
    EXPECT(pl.tiles == (ld + kCoxTile - 1) / kCoxTile && pl.tiles >= 1);
    EXPECT(pl.grid >= 1 && pl.grid <= c && pl.grid <= kCoxMaxGrid && (pl.grid == pl.tiles || pl.grid == c));
    EXPECT(pl.records == pl.grid && pl.longest == (pl.tiles + pl.grid - 1) / pl.grid);
    const CoxLayout lay = cox_layout(ld);
    std::vector<unsigned char> seen((size_t)ld, 0), tile_seen((size_t)pl.tiles, 0);
    std::vector<double> d((size_t)lay.doubles, 0.0);
    std::vector<int32_t> ii((size_t)lay.ints, 0);
    EXPECT(cox_run_first(pl.tiles, pl.grid, 0) == 0 && cox_run_first(pl.tiles, pl.grid, pl.grid) == pl.tiles);
    int64_t longest = 0;
    for (int64_t b = 0; b < pl.grid; ++b) {
        const int64_t t0 = cox_run_first(pl.tiles, pl.grid, b), t1 = cox_run_first(pl.tiles, pl.grid, b + 1);
        EXPECT(t1 > t0);                                        // every workgroup owns at least one tile
        if (t1 - t0 > longest) longest = t1 - t0;
        for (int64_t t = t0; t < t1; ++t) {
            ++tile_seen[(size_t)t];
            for (int64_t lane = 0; lane < kCoxBlock; ++lane) {
                const int64_t s0 = t * kCoxTile + lane * kCoxPer;
                if (s0 >= ld) continue;                         // the kernels' own guard: a lane's positions lie wholly below ld
                for (int c2 = 0; c2 < kCoxPer; ++c2) {
                    ++seen[(size_t)(s0 + c2)];
                    d[(size_t)(lay.eT + s0 + c2)] += 1.0; d[(size_t)(lay.hA + s0 + c2)] += 1.0; d[(size_t)(lay.hB + s0 + c2)] += 1.0;
                    d[(size_t)(lay.time + s0 + c2)] += 1.0;
                    ii[(size_t)(lay.order + s0 + c2)] += 1; ii[(size_t)(lay.first + s0 + c2)] += 1; ii[(size_t)(lay.last + s0 + c2)] += 1;
                }
            }
        }
        for (int a = 0; a < 3; ++a) d[(size_t)(lay.sums + a * kCoxMaxGrid + b)] += 1.0;
    }
    EXPECT(longest == pl.longest);
    for (int64_t i = 0; i < ld; ++i) EXPECT(seen[(size_t)i] == 1);
    for (int64_t t = 0; t < pl.tiles; ++t) EXPECT(tile_seen[(size_t)t] == 1);
    // the layout: the seven ld-long segments and the three runs of sums tile their buffers without overlap
    for (int64_t i = 0; i < 4 * ld; ++i) EXPECT(d[(size_t)i] == 1.0);
    for (int64_t i = 0; i < lay.ints; ++i) EXPECT(ii[(size_t)i] == 1);
    EXPECT(lay.doubles == 4 * ld + 3 * kCoxMaxGrid && lay.ints == 3 * ld && lay.sums == 4 * ld);
}

static void order_case(const std::vector<double>& t, const std::vector<int32_t>& o, const std::vector<int32_t>& f,
                       const std::vector<int32_t>& l) {
    const int64_t n = (int64_t)t.size(), ld = padded(n);
    std::vector<int32_t> order, first, last;
    cox_order(n, ld, t.data(), order, first, last);
    EXPECT((int64_t)order.size() == ld && (int64_t)first.size() == ld && (int64_t)last.size() == ld);
    for (int64_t s = 0; s < n; ++s) EXPECT(order[s] == o[s] && first[s] == f[s] && last[s] == l[s]);
    for (int64_t s = n; s < ld; ++s) EXPECT(order[s] == s && first[s] == s && last[s] == s);
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "plan")) {
        for (int a = 2; a + 1 < argc; a += 2) {
            const int64_t ld = std::atoll(argv[a]), cap = std::atoll(argv[a + 1]);
            const CoxPlan pl = cox_plan(ld, cap);
            const CoxLayout lay = cox_layout(ld);
            std::printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)pl.tiles,
                        (long long)pl.grid, (long long)pl.records, (long long)pl.longest,
                        (long long)cox_run_first(pl.tiles, pl.grid, 0), (long long)cox_run_first(pl.tiles, pl.grid, 1),
                        (long long)cox_run_first(pl.tiles, pl.grid, pl.grid - 1), (long long)cox_run_first(pl.tiles, pl.grid, pl.grid),
                        (long long)lay.eT, (long long)lay.hA, (long long)lay.hB, (long long)lay.time, (long long)lay.sums,
                        (long long)lay.doubles, (long long)lay.order, (long long)lay.first, (long long)lay.last, (long long)lay.ints);
        }
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "runs")) {
        for (int a = 2; a + 1 < argc; a += 2) {
            const CoxPlan pl = cox_plan(std::atoll(argv[a]), std::atoll(argv[a + 1]));
            std::printf("%lld %lld", (long long)pl.tiles, (long long)pl.grid);
            for (int64_t b = 0; b <= pl.grid; ++b) std::printf(" %lld", (long long)cox_run_first(pl.tiles, pl.grid, b));
            std::printf("\n");
        }
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "order")) {
        std::vector<double> t;
        for (int a = 2; a < argc; ++a) t.push_back(std::atof(argv[a]));
        const int64_t n = (int64_t)t.size();
        std::vector<int32_t> order, first, last;
        cox_order(n, padded(n), t.data(), order, first, last);
        for (const auto* v : {&order, &first, &last}) {
            for (int64_t s = 0; s < padded(n); ++s) std::printf("%d ", (int)(*v)[(size_t)s]);
            std::printf("\n");
        }
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "check")) {
        std::vector<double> t, s, o;
        for (int a = 2; a + 2 < argc; a += 3) {
            t.push_back(std::strtod(argv[a], nullptr));
            s.push_back(std::strtod(argv[a + 1], nullptr));
            o.push_back(std::strtod(argv[a + 2], nullptr));
        }
        char msg[128];
        const bool ok = cox_check((int64_t)t.size(), t.data(), s.data(), o.data(), msg, sizeof msg);
        std::printf("%s\n", ok ? "ok" : msg);
        return 0;
    }
    const int64_t caps[] = {kCoxMaxGrid, 1, 2, 3, 7};
    for (int64_t cap : caps) {
        for (int64_t n = 1; n <= 2100; n += (n < 130 ? 1 : 31)) walk(n, cap);
        const int64_t around[] = {kCoxTile, 2 * kCoxTile, 3 * kCoxTile, 5 * kCoxTile, 7 * kCoxTile, 8 * kCoxTile};
        for (int64_t m : around)
            for (int64_t dd = -33; dd <= 33; dd += 11) walk(m + dd, cap);
    }
    walk(kCoxMaxGrid * kCoxTile, kCoxMaxGrid);                  // the grid cap itself, and the first ld beyond it
    walk(kCoxMaxGrid * kCoxTile + 32, kCoxMaxGrid);
    EXPECT(kCoxBlock == 256 && kCoxPer == 4 && kCoxTile == 1024 && kCoxMaxGrid == 1024 && kCoxVals == 5);
    EXPECT(cox_grid_cap(0) == kCoxMaxGrid && cox_grid_cap(-5) == kCoxMaxGrid && cox_grid_cap(kCoxMaxGrid + 1) == kCoxMaxGrid);
    EXPECT(cox_grid_cap(1) == 1 && cox_grid_cap(kCoxMaxGrid) == kCoxMaxGrid);
    EXPECT(cox_plan(kCoxTile).grid == 1 && cox_plan(kCoxTile + 32).grid == 2);
    EXPECT(cox_plan(kCoxMaxGrid * kCoxTile).longest == 1 && cox_plan(kCoxMaxGrid * kCoxTile + 32).longest == 2);
    EXPECT(cox_plan(5 * kCoxTile + 32, 2).grid == 2 && cox_plan(5 * kCoxTile + 32, 2).longest == 3);
    // the time order: distinct, all equal, ties, sorted, reversed, n = 1 (stable: rows of equal time keep their order)
    order_case({3.0, 1.0, 2.0}, {1, 2, 0}, {0, 1, 2}, {0, 1, 2});
    order_case({5.0, 5.0, 5.0, 5.0}, {0, 1, 2, 3}, {0, 0, 0, 0}, {3, 3, 3, 3});
    order_case({2.0, 1.0, 2.0, 1.0, 3.0, 2.0}, {1, 3, 0, 2, 5, 4}, {0, 0, 2, 2, 2, 5}, {1, 1, 4, 4, 4, 5});
    order_case({1.0, 2.0, 2.0, 4.0}, {0, 1, 2, 3}, {0, 1, 1, 3}, {0, 2, 2, 3});
    order_case({4.0, 2.0, 2.0, 1.0}, {3, 1, 2, 0}, {0, 1, 1, 3}, {0, 2, 2, 3});
    order_case({7.0}, {0}, {0}, {0});
    order_case({0.0, -0.0, -1.0}, {2, 0, 1}, {0, 1, 1}, {0, 2, 2});
    std::printf(fails ? "cox_plan_main: %d FAILED\n" : "cox_plan_main OK tile=%d\n", fails ? fails : (int)kCoxTile);
    return fails ? 1 : 0;
}
