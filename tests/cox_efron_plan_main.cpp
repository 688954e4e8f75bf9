// Stand-alone check of what csrc/cox_plan.hpp adds for Efron ties (tests/test_cox_efron_plan_host.py builds and runs it under the
// host sanitizers).
//   no arguments     the Efron pair's layout at many ld: the offsets in order, the stated sizes, no overlap; the pair walked the
//                    way the kernels walk it over exactly-sized heap blocks (a lane that leaves its block is an ASan report);
//                    cox_one_stratum against cox_order_strata without ids; and the runs' records of the TIE-GROUP scans, as
//                    k_efron_mark and k_efron_hazard form them (the sum from the first position of the group the run's last
//                    position lies in, head seen when it lies inside the run; for the suffix scan the mirror image), pushed
//                    through a sequential restatement of k_cox_offsets and k_cox_scan on small integers and held to the
//                    group sums computed directly: an event's rank, d at the group's last position, the group's total at its
//                    first.
//   layout ld ...    the layout's fields, one line per ld
//   stratum n        cox_one_stratum's two vectors, one line each
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

static void layout_case(int64_t ld) {
    const CoxEfronLayout el = cox_efron_layout(ld);
    const int64_t offs[] = {el.cnt, el.Dv, el.Sdv, el.hc, el.hc2, el.lg, el.mm, el.sums, el.doubles};
    EXPECT(el.cnt == 0);
    for (int i = 0; i < 7; ++i) EXPECT(offs[i + 1] - offs[i] == ld);                  // seven vectors of ld, back to back
    EXPECT(el.doubles - el.sums == 5 * kCoxMaxGrid);                                 // the five scans' runs
    EXPECT(el.Dv - el.cnt == ld && el.hc2 - el.hc == ld);                            // each pair is one k_cox_scan<2, ., .>
    EXPECT(el.heads_p == 0 && el.heads_s == kCoxMaxGrid && el.ints == 2 * kCoxMaxGrid);
}

// the kernels' reads and writes of the Efron pair: every position of the seven vectors once per pass, a record per run
static void walk(int64_t n, int64_t cap) {
    const int64_t ld = padded(n);
    const CoxPlan pl = cox_plan(ld, cap);
    const CoxEfronLayout el = cox_efron_layout(ld);
    std::vector<double> ed((size_t)el.doubles, 0.0);
    std::vector<int32_t> ei((size_t)el.ints, 0);
    for (int64_t b = 0; b < pl.grid; ++b) {
        const int64_t t0 = cox_run_first(pl.tiles, pl.grid, b), t1 = cox_run_first(pl.tiles, pl.grid, b + 1);
        for (int i = 0; i < 5; ++i) ed[(size_t)(el.sums + i * kCoxMaxGrid + b)] += 1.0;
        ei[(size_t)(el.heads_p + b)] += 1;
        ei[(size_t)(el.heads_s + b)] += 1;
        for (int64_t t = t0; t < t1; ++t)
            for (int64_t lane = 0; lane < kCoxBlock; ++lane) {
                const int64_t s0 = t * kCoxTile + lane * kCoxPer;
                if (s0 >= ld) continue;
                for (int c = 0; c < kCoxPer; ++c)
                    for (int64_t v : {el.cnt, el.Dv, el.Sdv, el.hc, el.hc2, el.lg, el.mm}) ed[(size_t)(v + s0 + c)] += 1.0;
            }
    }
    for (int64_t i = 0; i < 7 * ld; ++i) EXPECT(ed[(size_t)i] == 1.0);
    for (int64_t i = 0; i < 5 * kCoxMaxGrid; ++i) EXPECT(ed[(size_t)(el.sums + i)] == ((i % kCoxMaxGrid) < pl.grid ? 1.0 : 0.0));
    for (int64_t i = 0; i < 2 * kCoxMaxGrid; ++i) EXPECT(ei[(size_t)i] == ((i % kCoxMaxGrid) < pl.grid ? 1 : 0));
}

// k_cox_offsets and k_cox_scan<., SUFFIX, true>, restated sequentially: rec, head -- the runs' records; bound[s] == s marks a head
static std::vector<int64_t> scan(const std::vector<int64_t>& x, const std::vector<int32_t>& bound, bool suffix, const CoxPlan& pl,
                                 int64_t ld, const std::vector<int64_t>& rec, const std::vector<int>& head) {
    std::vector<int64_t> off((size_t)pl.grid, 0), out((size_t)ld, 0);
    int64_t carry = 0;
    for (int64_t i = 0; i < pl.grid; ++i) {
        const int64_t b = suffix ? pl.grid - 1 - i : i;
        off[(size_t)b] = carry;
        carry = head[(size_t)b] ? rec[(size_t)b] : carry + rec[(size_t)b];
    }
    for (int64_t b = 0; b < pl.grid; ++b) {
        const int64_t lo = cox_run_first(pl.tiles, pl.grid, b) * kCoxTile;
        const int64_t hi = std::min(cox_run_first(pl.tiles, pl.grid, b + 1) * kCoxTile, ld);
        int64_t c = off[(size_t)b];
        for (int64_t i = 0; i < hi - lo; ++i) {
            const int64_t s = suffix ? hi - 1 - i : lo + i;
            c = bound[(size_t)s] == s ? x[(size_t)s] : c + x[(size_t)s];
            out[(size_t)s] = c;
        }
    }
    return out;
}

static void records_case(int64_t n, int64_t cap, int maxgroup) {
    const int64_t ld = padded(n);
    const CoxPlan pl = cox_plan(ld, cap);
    uint64_t seed = 99 + (uint64_t)n * 3 + (uint64_t)maxgroup;
    std::vector<double> t((size_t)n);
    double now = 0.0;
    for (int64_t i = 0, left = 0; i < n; ++i) {
        if (left == 0) { now += 1.0; left = 1 + (int64_t)(lcg(seed) % (uint64_t)maxgroup); }
        t[(size_t)i] = now;
        --left;
    }
    std::vector<int32_t> order, first, last, sfirst, slast;
    cox_order_strata(n, ld, t.data(), nullptr, order, first, last, sfirst, slast);
    std::vector<int64_t> x((size_t)ld, 0);
    for (int64_t s = 0; s < n; ++s) x[(size_t)s] = (int64_t)(lcg(seed) % 3);          // 0: not an event
    std::vector<int64_t> rp((size_t)pl.grid), rs((size_t)pl.grid);
    std::vector<int> hp((size_t)pl.grid), hs((size_t)pl.grid);
    for (int64_t b = 0; b < pl.grid; ++b) {
        const int64_t t0 = cox_run_first(pl.tiles, pl.grid, b), t1 = cox_run_first(pl.tiles, pl.grid, b + 1);
        const int64_t end = std::min(t1 * kCoxTile, ld);
        const int64_t gb = first[(size_t)(end - 1)], ge = last[(size_t)(t0 * kCoxTile)];
        int64_t p = 0, q = 0;
        for (int64_t s = t0 * kCoxTile; s < end; ++s) { p += s >= gb ? x[(size_t)s] : 0; q += s <= ge ? x[(size_t)s] : 0; }
        rp[(size_t)b] = p; hp[(size_t)b] = gb >= t0 * kCoxTile;
        rs[(size_t)b] = q; hs[(size_t)b] = ge < end;
    }
    const std::vector<int64_t> pre = scan(x, first, false, pl, ld, rp, hp), suf = scan(x, last, true, pl, ld, rs, hs);
    for (int64_t s = 0; s < ld; ++s) {
        int64_t a = 0, z = 0;
        for (int64_t q = first[(size_t)s]; q <= s; ++q) a += x[(size_t)q];
        for (int64_t q = s; q <= last[(size_t)s]; ++q) z += x[(size_t)q];
        EXPECT(pre[(size_t)s] == a && suf[(size_t)s] == z);
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "layout")) {
        for (int a = 2; a < argc; ++a) {
            const CoxEfronLayout el = cox_efron_layout(std::atoll(argv[a]));
            std::printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)el.cnt, (long long)el.Dv,
                        (long long)el.Sdv, (long long)el.hc, (long long)el.hc2, (long long)el.lg, (long long)el.mm, (long long)el.sums,
                        (long long)el.doubles, (long long)el.heads_p, (long long)el.heads_s, (long long)el.ints);
        }
        return 0;
    }
    if (argc > 2 && !std::strcmp(argv[1], "stratum")) {
        const int64_t n = std::atoll(argv[2]);
        std::vector<int32_t> sfirst, slast;
        cox_one_stratum(n, padded(n), sfirst, slast);
        for (const auto* v : {&sfirst, &slast}) {
            for (int32_t q : *v) std::printf("%d ", (int)q);
            std::printf("\n");
        }
        return 0;
    }
    for (int64_t ld : {(int64_t)32, kCoxTile - 32, kCoxTile, kCoxTile + 32, 5 * kCoxTile + 32, ((int64_t)1 << 31) - 32}) layout_case(ld);
    for (int64_t n = 1; n <= 2100; n += (n < 130 ? 1 : 31)) {
        std::vector<int32_t> o, f, l, sf, sl, sf2, sl2;
        std::vector<double> t((size_t)n, 1.0);
        cox_order_strata(n, padded(n), t.data(), nullptr, o, f, l, sf, sl);
        cox_one_stratum(n, padded(n), sf2, sl2);
        EXPECT(sf == sf2 && sl == sl2);
    }
    const int64_t caps[] = {kCoxMaxGrid, 1, 2, 3};
    for (int64_t cap : caps)
        for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)31, (int64_t)32, (int64_t)65, kCoxTile - 1, kCoxTile + 1, 2 * kCoxTile + 1,
                          5 * kCoxTile + 3}) {
            walk(n, cap);
            for (int maxgroup : {1, 2, 7, 300, 100000}) records_case(n, cap, maxgroup);
        }
    std::printf(fails ? "cox_efron_plan_main: %d FAILED\n" : "cox_efron_plan_main OK tile=%d\n", fails ? fails : (int)kCoxTile);
    return fails ? 1 : 0;
}
