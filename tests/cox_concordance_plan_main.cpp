// Stand-alone check of what csrc/cox_plan.hpp adds for the concordance index (tests/test_cox_concordance_plan_host.py builds and
// runs it under the host sanitizers).
//   no arguments     cox_conc_take: for every 0 <= a <= b <= 70 the runs taken over all levels tile [a, b) exactly once, at most
//                    two a level, all of them whole; cox_conc_fringe with the levels from the tile's up does the same for
//                    ranges up to 5 T + 3; cox_conc_layout tiles its two buffers; and the whole count the way the kernels walk
//                    it -- the tile sort in two ping-pong blocks, the fringes, a level's queries and its merge-path ranks with
//                    a short last run and a run without a sibling -- as a sequential restatement over exactly-sized heap blocks
//                    (an index that leaves its block is an ASan report), held to the pairs counted directly with ==.
//   layout ld ...    the layout's fields, one line per ld
//   order ld N strata(0/1) time status stratum ...
//                    the handle's order (cox_order_strata, or cox_order without strata) and then cox_conc_order: corder, qa and
//                    qb, one line each
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "../coordinatedescent.jl_amd/csrc/cox_plan.hpp"

static int fails = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); ++fails; } \
    } while (0)

static int64_t padded(int64_t n) { return (n + 31) / 32 * 32; }
static uint64_t lcg(uint64_t& s) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return s >> 33; }

static void take_tiles() {
    for (int64_t b = 0; b <= 70; ++b)
        for (int64_t a = 0; a <= b; ++a) {
            std::vector<int> hit(71, 0);
            for (int lev = 0; lev <= 7; ++lev) {
                const CoxConcTake t = cox_conc_take(a, b, lev);
                EXPECT(t.count >= 0 && t.count <= 2);
                for (int i = 0; i < t.count; ++i) {
                    const int64_t lo = t.run[i] << lev, hi = (t.run[i] + 1) << lev;
                    EXPECT(lo >= a && hi <= b);                         // a whole run inside the range
                    for (int64_t s = lo; s < hi && s <= 70; ++s) ++hit[(size_t)s];
                }
            }
            for (int64_t s = 0; s <= 70; ++s) EXPECT(hit[(size_t)s] == (s >= a && s < b ? 1 : 0));
        }
}

static void fringe_tiles() {
    const int64_t top = 5 * kCoxTile + 3;
    uint64_t seed = 11;
    for (int trial = 0; trial < 4000; ++trial) {
        int64_t a = (int64_t)(lcg(seed) % (uint64_t)(top + 1)), b = (int64_t)(lcg(seed) % (uint64_t)(top + 1));
        if (trial < 64) { a = (trial % 8) * kCoxTile / 2 + (trial % 3) - 1; b = a + (trial / 8) * kCoxTile / 2 + (trial % 2); }
        if (a < 0) a = 0;
        if (a > b) std::swap(a, b);
        if (b > top) b = top;
        if (a > b) a = b;
        const CoxConcFringe f = cox_conc_fringe(a, b);
        EXPECT(a <= f.a1 && f.a1 <= f.b0 && f.b0 <= b);
        EXPECT(f.a1 - a < kCoxTile && b - f.b0 < 2 * kCoxTile);
        EXPECT(f.a1 == f.b0 || (f.a1 % kCoxTile == 0 && f.b0 % kCoxTile == 0));
        int64_t covered = 0, at = f.a1;                                 // the levels from the tile's up tile [a1, b0)
        std::vector<std::pair<int64_t, int64_t>> runs;
        for (int lev = kCoxTileLog; lev <= 14; ++lev) {
            const CoxConcTake t = cox_conc_take(a, b, lev);
            for (int i = 0; i < t.count; ++i) runs.push_back({t.run[i] << lev, (t.run[i] + 1) << lev});
        }
        std::sort(runs.begin(), runs.end());
        for (auto& r : runs) { EXPECT(r.first == at); at = r.second; covered += r.second - r.first; }
        EXPECT(covered == f.b0 - f.a1 && (runs.empty() || at == f.b0));
    }
}

static void layout_case(int64_t ld) {
    const CoxConcLayout c = cox_conc_layout(ld);
    EXPECT(c.N % kCoxTile == 0 && c.N >= ld && c.N - ld < kCoxTile && c.tiles * kCoxTile == c.N && c.tiles >= 1);
    const int64_t d[] = {c.key0, c.v0, c.ka, c.pa, c.kb, c.pb, c.L, c.E, c.G, c.part};
    for (int i = 0; i < 10; ++i) EXPECT(d[i] == (int64_t)i * c.N);
    EXPECT(c.out == c.part + 4 * c.tiles && c.doubles == c.out + 4);
    EXPECT(c.order == 0 && c.qa == c.N && c.qb == 2 * c.N && c.ints == 3 * c.N);
    EXPECT(((int64_t)1 << cox_conc_top(c.N)) >= c.N && (cox_conc_top(c.N) == kCoxTileLog || ((int64_t)1 << (cox_conc_top(c.N) - 1)) < c.N));
}

static int64_t lower(const double* k, int64_t len, double x) {
    int64_t lo = 0, hi = len;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (k[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}
static int64_t upper(const double* k, int64_t len, double x) {
    int64_t lo = 0, hi = len;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (k[mid] <= x) lo = mid + 1; else hi = mid; }
    return lo;
}

// The kernels' walk, sequentially (cox_concordance.hip: k_conc_tile, k_conc_fringe, k_conc_level, k_conc_rows, k_conc_total), on
// small integers: times in 0 .. tmax - 1, eta in 0 .. emax - 1, G strata, weights 1 or 2, a subset of the rows.
static void walk(int64_t n, int tmax, int emax, int G, bool weights, bool subset, uint64_t seed) {
    const int64_t ld = padded(n);
    const CoxConcLayout cl = cox_conc_layout(ld);
    const int64_t N = cl.N;
    std::vector<double> time((size_t)n), status((size_t)n), eta((size_t)n), v((size_t)n);
    std::vector<int32_t> g((size_t)n);
    std::vector<char> in((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        time[(size_t)i] = (double)(lcg(seed) % (uint64_t)tmax);
        status[(size_t)i] = lcg(seed) % 10 < 7 ? 1.0 : 0.0;
        eta[(size_t)i] = (double)(lcg(seed) % (uint64_t)emax);
        g[(size_t)i] = (int32_t)(lcg(seed) % (uint64_t)G);
        v[(size_t)i] = weights ? (double)(1 + lcg(seed) % 2) : 1.0;
        in[(size_t)i] = subset ? (lcg(seed) % 3 != 0) : 1;
    }
    std::vector<int32_t> order, first, last, sfirst, slast, corder, qa, qb;
    cox_order_strata(n, ld, time.data(), g.data(), order, first, last, sfirst, slast);
    cox_conc_order(n, ld, N, order.data(), last.data(), slast.data(), status.data(), corder, qa, qb);
    // exactly-sized blocks, as the layout cuts them
    std::vector<double> key0((size_t)N), v0((size_t)N), ka((size_t)N), pa((size_t)N), kb((size_t)N), pb((size_t)N), L((size_t)N),
        E((size_t)N), Gs((size_t)N);
    const double inf = std::numeric_limits<double>::infinity();
    for (int64_t t = 0; t < cl.tiles; ++t) {                           // k_conc_tile
        std::vector<double> sk[2] = {std::vector<double>((size_t)kCoxTile), std::vector<double>((size_t)kCoxTile)};
        std::vector<double> sp[2] = {std::vector<double>((size_t)kCoxTile), std::vector<double>((size_t)kCoxTile)};
        for (int e = 0; e < kCoxTile; ++e) {
            const int64_t p = t * kCoxTile + e;
            double key = inf, w = 0.0;
            if (p < n) {
                const int32_t row = corder[(size_t)p];
                EXPECT(row >= 0 && row < n);
                if (in[(size_t)row]) { key = eta[(size_t)row]; w = v[(size_t)row]; }
            }
            key0[(size_t)p] = key; v0[(size_t)p] = w; sk[0][(size_t)e] = key; sp[0][(size_t)e] = w;
        }
        int src = 0;
        for (int lev = 0; lev < kCoxTileLog; ++lev) {
            const int len = 1 << lev;
            for (int e = 0; e < kCoxTile; ++e) {
                const int m = e >> lev, own = m << lev, sib = (m ^ 1) << lev;
                const double key = sk[src][(size_t)e];
                const int j = (int)((m & 1) ? upper(sk[src].data() + sib, len, key) : lower(sk[src].data() + sib, len, key));
                const int pos = ((m & ~1) << lev) + (e - own) + j;
                sk[src ^ 1].at((size_t)pos) = key;
                sp[src ^ 1].at((size_t)pos) = j > 0 ? sp[src][(size_t)e] + sp[src].at((size_t)(sib + j - 1)) : sp[src][(size_t)e];
            }
            src ^= 1;
        }
        for (int e = 0; e < kCoxTile; ++e) { ka[(size_t)(t * kCoxTile + e)] = sk[src][(size_t)e]; pa[(size_t)(t * kCoxTile + e)] = sp[src][(size_t)e]; }
    }
    auto asks = [&](int64_t p) { return v0[(size_t)p] > 0.0 && qa[(size_t)p] < qb[(size_t)p]; };
    for (int64_t p = 0; p < N; ++p) {                                   // k_conc_fringe
        double l = 0, e = 0, gg = 0;
        if (asks(p)) {
            const double x = key0[(size_t)p];
            const int64_t a = qa[(size_t)p], b = qb[(size_t)p];
            EXPECT(a > p && b <= n);
            const CoxConcFringe f = cox_conc_fringe(a, b);
            for (int64_t j = a; j < b; ++j) {
                if (j >= f.a1 && j < f.b0) continue;
                l += key0.at((size_t)j) < x ? v0[(size_t)j] : 0.0;
                e += key0[(size_t)j] <= x ? v0[(size_t)j] : 0.0;
                gg += v0[(size_t)j];
            }
        }
        L[(size_t)p] = l; E[(size_t)p] = e; Gs[(size_t)p] = gg;
    }
    const int top = cox_conc_top(N);
    double *kin = ka.data(), *pin = pa.data(), *kout = kb.data(), *pout = pb.data();
    for (int lev = kCoxTileLog; lev < top; ++lev) {                     // k_conc_level: the run of level top is never taken
        const int64_t len = (int64_t)1 << lev;
        std::vector<char> written((size_t)N, 0);
        for (int64_t p = 0; p < N; ++p) {
            if (asks(p)) {
                const CoxConcTake t = cox_conc_take(qa[(size_t)p], qb[(size_t)p], lev);
                for (int i = 0; i < t.count; ++i) {
                    const int64_t rb = t.run[i] << lev;
                    EXPECT(rb >= 0 && rb + len <= N);
                    const int64_t lo = lower(kin + rb, len, key0[(size_t)p]), up = upper(kin + rb, len, key0[(size_t)p]);
                    L[(size_t)p] += lo > 0 ? pin[rb + lo - 1] : 0.0;
                    E[(size_t)p] += up > 0 ? pin[rb + up - 1] : 0.0;
                    Gs[(size_t)p] += pin[rb + len - 1];
                }
            }
            if (lev < top - 1) {
                const int64_t m = p >> lev, own = m << lev, sib = (m ^ 1) << lev;
                int64_t pos = p;
                double pre = pin[p];
                if (sib < N) {
                    const int64_t sl = N - sib < len ? N - sib : len;
                    EXPECT(sl > 0);
                    const int64_t j = (m & 1) ? upper(kin + sib, sl, kin[p]) : lower(kin + sib, sl, kin[p]);
                    pos = ((m & ~(int64_t)1) << lev) + (p - own) + j;
                    if (j > 0) pre += pin[sib + j - 1];
                }
                EXPECT(pos >= 0 && pos < N && !written[(size_t)pos]);
                if (pos >= 0 && pos < N) { kout[pos] = kin[p]; pout[pos] = pre; written[(size_t)pos] = 1; }
            }
        }
        if (lev < top - 1) {
            for (int64_t p = 0; p + 1 < N; ++p)                         // the new runs are sorted and their prefix sums ascend
                if (((p + 1) >> (lev + 1)) == (p >> (lev + 1))) EXPECT(kout[p] <= kout[p + 1] && pout[p] <= pout[p + 1]);
            std::swap(kin, kout);
            std::swap(pin, pout);
        }
    }
    double got[3] = {0, 0, 0}, want[3] = {0, 0, 0};
    for (int64_t p = 0; p < N; ++p)
        if (asks(p)) {
            got[0] += v0[(size_t)p] * L[(size_t)p];
            got[1] += v0[(size_t)p] * (Gs[(size_t)p] - E[(size_t)p]);
            got[2] += v0[(size_t)p] * (E[(size_t)p] - L[(size_t)p]);
        }
    for (int64_t i = 0; i < n; ++i) {                                   // the definition
        if (!in[(size_t)i] || status[(size_t)i] != 1.0) continue;
        for (int64_t j = 0; j < n; ++j) {
            if (j == i || !in[(size_t)j] || g[(size_t)j] != g[(size_t)i]) continue;
            if (!(time[(size_t)j] > time[(size_t)i] || (time[(size_t)j] == time[(size_t)i] && status[(size_t)j] == 0.0))) continue;
            const double w = v[(size_t)i] * v[(size_t)j];
            want[eta[(size_t)i] > eta[(size_t)j] ? 0 : eta[(size_t)i] < eta[(size_t)j] ? 1 : 2] += w;
        }
    }
    for (int i = 0; i < 3; ++i) EXPECT(got[i] == want[i]);
    if (got[0] != want[0] || got[1] != want[1] || got[2] != want[2])
        std::printf("walk n=%lld: got %g %g %g want %g %g %g\n", (long long)n, got[0], got[1], got[2], want[0], want[1], want[2]);
}

int main(int argc, char** argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "layout")) {
        for (int i = 2; i < argc; ++i) {
            const CoxConcLayout c = cox_conc_layout(std::atoll(argv[i]));
            std::printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)c.N,
                        (long long)c.tiles, (long long)c.key0, (long long)c.v0, (long long)c.ka, (long long)c.pa, (long long)c.kb,
                        (long long)c.pb, (long long)c.L, (long long)c.E, (long long)c.G, (long long)c.part, (long long)c.out,
                        (long long)c.doubles, (long long)c.order, (long long)c.qa, (long long)c.qb, (long long)c.ints);
        }
        return 0;
    }
    if (argc >= 5 && !std::strcmp(argv[1], "order")) {
        const int64_t ld = std::atoll(argv[2]), N = std::atoll(argv[3]);
        const bool strata = std::atoi(argv[4]) != 0;
        const int64_t n = (argc - 5) / 3;
        std::vector<double> time((size_t)n), status((size_t)n);
        std::vector<int32_t> g((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            time[(size_t)i] = std::atof(argv[5 + 3 * i]);
            status[(size_t)i] = std::atof(argv[6 + 3 * i]);
            g[(size_t)i] = (int32_t)std::atoi(argv[7 + 3 * i]);
        }
        std::vector<int32_t> order, first, last, sfirst, slast, corder, qa, qb;
        if (strata) cox_order_strata(n, ld, time.data(), g.data(), order, first, last, sfirst, slast);
        else cox_order(n, ld, time.data(), order, first, last);
        cox_conc_order(n, ld, N, order.data(), last.data(), strata ? slast.data() : nullptr, status.data(), corder, qa, qb);
        for (const std::vector<int32_t>* vec : {&corder, &qa, &qb}) {
            for (int32_t x : *vec) std::printf("%d ", x);
            std::printf("\n");
        }
        return 0;
    }
    take_tiles();
    fringe_tiles();
    for (int64_t ld : {(int64_t)32, (int64_t)64, kCoxTile, kCoxTile + 32, 2 * kCoxTile, 5 * kCoxTile + 32, (int64_t)2000032}) layout_case(ld);
    EXPECT(cox_conc_top(kCoxTile) == 10 && cox_conc_top(2 * kCoxTile) == 11 && cox_conc_top(3 * kCoxTile) == 12 &&
           cox_conc_top(6 * kCoxTile) == 13);
    uint64_t seed = 5;                                           // (n = 2 T = N = 2^top: the one size at which level top - 1 is taken)
    for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)65, kCoxTile, kCoxTile + 1, 2 * kCoxTile, 2 * kCoxTile + 1, 3 * kCoxTile - 5, 5 * kCoxTile + 3}) {
        walk(n, 1 << 20, 1 << 20, 1, false, false, ++seed);      // (nearly) no ties at all
        walk(n, 7, 5, 3, true, true, ++seed);                       // heavy ties, strata, weights, a subset
        walk(n, 1, 3, 1, false, true, ++seed);                      // one time for all
        walk(n, 40, 1, 2, true, false, ++seed);                     // one eta for all
    }
    if (fails) { std::printf("%d FAILED\n", fails); return 1; }
    std::printf("cox_concordance_plan_main OK tile=%lld\n", (long long)kCoxTile);
    return 0;
}
