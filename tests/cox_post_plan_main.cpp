// Stand-alone check of what csrc/cox_plan.hpp adds for the post-estimation exports (tests/test_cox_post_plan_host.py builds and
// runs it under the host sanitizers).
//   no arguments     cox_post_layout at many ld: the offsets in order, the stated sizes, no overlap; cox_layout and
//                    cox_efron_layout value for value what they were, at ld = 32 and 4096; the post group walked the way the
//                    kernels walk it over exactly-sized heap blocks (a lane that leaves its block is an ASan report); and the
//                    table's compaction -- the runs' records of the scan of dv by TIE GROUP as k_post_mark forms them, the
//                    flags, the runs' counts and the slots -- pushed through a sequential restatement of k_post_offsets and
//                    k_post_scan on small integers and held to the groups' sums and ranks computed directly, for groups of 1 to
//                    n rows and grids of 1, 2, 3 and full.
//   layout ld ...    the layout's fields, one line per ld
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
    const CoxPostLayout pl = cox_post_layout(ld);
    EXPECT(pl.dv == 0 && pl.flag == ld && pl.out == 2 * ld);                         // two scanned vectors, then the columns
    EXPECT(pl.sums - pl.out == kCoxPostCols * ld && kCoxPostCols == 5);
    EXPECT(pl.total - pl.sums == 2 * kCoxMaxGrid && pl.doubles == pl.total + 1);     // the two scans' runs, then the count
    EXPECT(pl.stratum == 0 && pl.slotpos == ld && pl.heads == 2 * ld && pl.ints == 2 * ld + kCoxMaxGrid);
}

// the earlier layouts keep every value
static void earlier_layouts() {
    const int64_t G = kCoxMaxGrid;
    for (int64_t ld : {(int64_t)32, (int64_t)4096}) {
        const CoxLayout a = cox_layout(ld);
        const int64_t got[] = {a.eT, a.hA, a.hB, a.time, a.sums, a.doubles, a.order, a.first, a.last, a.ints, a.sfirst, a.slast,
                               a.strata, a.heads, a.strata_ints, a.weight, a.strata_doubles, a.pos2, a.lo, a.enter, a.heads2,
                               a.interval_ints, a.start, a.T2, a.sums2, a.interval_doubles};
        const int64_t want[] = {0, ld, 2 * ld, 3 * ld, 4 * ld, 4 * ld + 3 * G, 0, ld, 2 * ld, 3 * ld, 0, ld,
                                2 * ld, 3 * ld, 3 * ld + 2 * G, 0, ld, 0, ld, 2 * ld, 3 * ld,
                                3 * ld + G, 0, ld, 2 * ld, 2 * ld + G};
        static_assert(sizeof got == sizeof want && sizeof got == sizeof(CoxLayout), "every field of CoxLayout is listed");
        for (size_t i = 0; i < sizeof got / sizeof got[0]; ++i) EXPECT(got[i] == want[i]);
        const CoxEfronLayout e = cox_efron_layout(ld);
        const int64_t egot[] = {e.cnt, e.Dv, e.Sdv, e.hc, e.hc2, e.lg, e.mm, e.sums, e.doubles, e.heads_p, e.heads_s, e.ints};
        const int64_t ewant[] = {0, ld, 2 * ld, 3 * ld, 4 * ld, 5 * ld, 6 * ld, 7 * ld, 7 * ld + 5 * G, 0, G, 2 * G};
        static_assert(sizeof egot == sizeof ewant && sizeof egot == sizeof(CoxEfronLayout), "every field of CoxEfronLayout is listed");
        for (size_t i = 0; i < sizeof egot / sizeof egot[0]; ++i) EXPECT(egot[i] == ewant[i]);
    }
    EXPECT(cox_layout(32).doubles == 128 + 3072 && cox_layout(4096).doubles == 16384 + 3072);      // and as plain numbers
    EXPECT(cox_efron_layout(32).doubles == 224 + 5120 && cox_efron_layout(4096).doubles == 28672 + 5120);
}

// the kernels' reads and writes of the post group: every position of dv and flag once per pass, a record per run; the columns
// and the stratum only at slots below the count
static void walk(int64_t n, int64_t cap) {
    const int64_t ld = padded(n);
    const CoxPlan pl = cox_plan(ld, cap);
    const CoxPostLayout po = cox_post_layout(ld);
    std::vector<double> pd((size_t)po.doubles, 0.0);
    std::vector<int32_t> pi((size_t)po.ints, 0);
    for (int64_t b = 0; b < pl.grid; ++b) {
        const int64_t t0 = cox_run_first(pl.tiles, pl.grid, b), t1 = cox_run_first(pl.tiles, pl.grid, b + 1);
        for (int i = 0; i < 2; ++i) pd[(size_t)(po.sums + i * kCoxMaxGrid + b)] += 1.0;
        pi[(size_t)(po.heads + b)] += 1;
        for (int64_t t = t0; t < t1; ++t)
            for (int64_t lane = 0; lane < kCoxBlock; ++lane) {
                const int64_t s0 = t * kCoxTile + lane * kCoxPer;
                if (s0 >= ld) continue;
                for (int c = 0; c < kCoxPer; ++c) {
                    pd[(size_t)(po.dv + s0 + c)] += 1.0;
                    pd[(size_t)(po.flag + s0 + c)] += 1.0;
                    if (s0 + c < n) {                            // the worst case: every row a table row, slot = position
                        for (int k = 0; k < kCoxPostCols; ++k) pd[(size_t)(po.out + k * ld + s0 + c)] += 1.0;
                        pi[(size_t)(po.stratum + s0 + c)] += 1;
                        pi[(size_t)(po.slotpos + s0 + c)] += 1;
                    }
                }
            }
    }
    pd[(size_t)po.total] += 1.0;
    for (int64_t i = 0; i < 2 * ld; ++i) EXPECT(pd[(size_t)i] == 1.0);
    for (int64_t i = 0; i < kCoxPostCols * ld; ++i) EXPECT(pd[(size_t)(po.out + i)] == ((i % ld) < n ? 1.0 : 0.0));
    for (int64_t i = 0; i < 2 * kCoxMaxGrid; ++i) EXPECT(pd[(size_t)(po.sums + i)] == ((i % kCoxMaxGrid) < pl.grid ? 1.0 : 0.0));
    for (int64_t i = 0; i < 2 * ld; ++i) EXPECT(pi[(size_t)i] == ((i % ld) < n ? 1 : 0));
    for (int64_t i = 0; i < kCoxMaxGrid; ++i) EXPECT(pi[(size_t)(po.heads + i)] == (i < pl.grid ? 1 : 0));
}

// k_post_offsets, sequentially: the runs' (sum since the last head, head seen) into exclusive offsets; -> the total
static double offsets(std::vector<double>& sums, const std::vector<int32_t>* heads, int64_t runs) {
    double carry = 0.0;
    for (int64_t b = 0; b < runs; ++b) {
        const double mine = sums[(size_t)b];
        sums[(size_t)b] = carry;
        carry = (heads && (*heads)[(size_t)b]) ? mine : carry + mine;
    }
    return carry;
}

// k_post_scan, sequentially: run b walks its tiles forwards from its offset, restarting at bound[s] == s
static void scan(std::vector<double>& v, const std::vector<double>& offs, const CoxPlan& pl, int64_t ld, const std::vector<int32_t>* bound) {
    for (int64_t b = 0; b < pl.grid; ++b) {
        const int64_t s0 = cox_run_first(pl.tiles, pl.grid, b) * kCoxTile;
        const int64_t s1 = std::min(cox_run_first(pl.tiles, pl.grid, b + 1) * kCoxTile, ld);
        double carry = offs[(size_t)b];
        for (int64_t s = s0; s < s1; ++s) {
            carry = (bound && (*bound)[(size_t)s] == s) ? v[(size_t)s] : carry + v[(size_t)s];
            v[(size_t)s] = carry;
        }
    }
}

// the table's compaction over n rows in tie groups of random sizes up to `longest`, events at random
static void compaction(int64_t n, int64_t cap, int64_t longest, uint64_t seed) {
    const int64_t ld = padded(n);
    const CoxPlan pl = cox_plan(ld, cap);
    std::vector<int32_t> first((size_t)ld), last((size_t)ld);
    std::vector<double> dv((size_t)ld, 0.0);
    for (int64_t s = 0; s < n;) {
        const int64_t e = std::min<int64_t>(n, s + 1 + (int64_t)(lcg(seed) % (uint64_t)longest));
        const bool none = lcg(seed) % 4 == 0;                    // a quarter of the groups hold no event
        for (int64_t q = s; q < e; ++q) {
            first[(size_t)q] = (int32_t)s; last[(size_t)q] = (int32_t)(e - 1);
            dv[(size_t)q] = none ? 0.0 : (double)(lcg(seed) % 3);      // small integers: every sum is exact in any order
        }
        s = e;
    }
    for (int64_t s = n; s < ld; ++s) { first[(size_t)s] = last[(size_t)s] = (int32_t)s; }
    // what the table should hold, directly
    std::vector<double> want_event;
    std::vector<int64_t> want_at;
    for (int64_t s = 0; s < n; s = last[(size_t)s] + 1) {
        double sum = 0.0;
        for (int64_t q = s; q <= last[(size_t)s]; ++q) sum += dv[(size_t)q];
        if (sum > 0.0) { want_event.push_back(sum); want_at.push_back(last[(size_t)s]); }
    }
    // k_post_mark's records, the offsets and the scan by tie group
    std::vector<double> sums((size_t)kCoxMaxGrid, 0.0), v = dv;
    std::vector<int32_t> heads((size_t)kCoxMaxGrid, 0);
    for (int64_t b = 0; b < pl.grid; ++b) {
        const int64_t t0 = cox_run_first(pl.tiles, pl.grid, b), t1 = cox_run_first(pl.tiles, pl.grid, b + 1);
        const int64_t end = std::min(t1 * kCoxTile, ld), gb = first[(size_t)(end - 1)];
        for (int64_t s = t0 * kCoxTile; s < end; ++s) sums[(size_t)b] += s >= gb ? dv[(size_t)s] : 0.0;
        heads[(size_t)b] = gb >= t0 * kCoxTile ? 1 : 0;
    }
    offsets(sums, &heads, pl.grid);
    scan(v, sums, pl, ld, &first);
    // k_post_flag, the counts' offsets, the plain scan, the slots
    std::vector<double> flag((size_t)ld, 0.0), fsums((size_t)kCoxMaxGrid, 0.0);
    for (int64_t b = 0; b < pl.grid; ++b) {
        const int64_t s0 = cox_run_first(pl.tiles, pl.grid, b) * kCoxTile;
        const int64_t s1 = std::min(cox_run_first(pl.tiles, pl.grid, b + 1) * kCoxTile, ld);
        for (int64_t s = s0; s < s1; ++s) {
            flag[(size_t)s] = (s < n && last[(size_t)s] == s && v[(size_t)s] > 0.0) ? 1.0 : 0.0;
            fsums[(size_t)b] += flag[(size_t)s];
        }
    }
    const std::vector<double> is_flag = flag;
    const double total = offsets(fsums, nullptr, pl.grid);
    scan(flag, fsums, pl, ld, nullptr);
    EXPECT((int64_t)total == (int64_t)want_event.size());
    int64_t seen = 0;
    for (int64_t s = 0; s < ld; ++s) {
        if (is_flag[(size_t)s] == 0.0) continue;
        const int64_t slot = (int64_t)flag[(size_t)s] - 1;
        EXPECT(slot == seen && slot < n);
        if (slot == seen && seen < (int64_t)want_event.size()) {
            EXPECT(want_at[(size_t)slot] == s && want_event[(size_t)slot] == v[(size_t)s]);
        }
        ++seen;
    }
    EXPECT(seen == (int64_t)want_event.size());
}

int main(int argc, char** argv) {
    if (argc > 2 && !std::strcmp(argv[1], "layout")) {
        for (int i = 2; i < argc; ++i) {
            const CoxPostLayout p = cox_post_layout(std::atoll(argv[i]));
            std::printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)p.dv, (long long)p.flag, (long long)p.out,
                        (long long)p.sums, (long long)p.total, (long long)p.doubles, (long long)p.stratum, (long long)p.slotpos,
                        (long long)p.heads, (long long)p.ints);
        }
        return 0;
    }
    for (int64_t ld = 32; ld <= 8 * kCoxTile; ld += 32) layout_case(ld);
    layout_case(2000000 + 0);
    earlier_layouts();
    for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)65, kCoxTile - 1, kCoxTile + 1, 2 * kCoxTile + 1, 5 * kCoxTile + 3})
        for (int64_t cap : {(int64_t)1, (int64_t)2, (int64_t)3, kCoxMaxGrid}) {
            walk(n, cap);
            uint64_t seed = (uint64_t)(n * 7 + cap);
            for (int64_t longest : {(int64_t)1, (int64_t)3, (int64_t)9, (int64_t)300, 2 * kCoxTile + 5, n}) compaction(n, cap, longest, ++seed);
        }
    if (fails) { std::printf("cox_post_plan_main: %d FAILED\n", fails); return 1; }
    std::printf("cox_post_plan_main OK tile=%lld\n", (long long)kCoxTile);
    return 0;
}
