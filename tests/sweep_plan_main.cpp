// Stand-alone check of csrc/sweep_plan.hpp, built with -fsanitize=address,undefined by tests/test_sweep_plan_host.py: over
// every width, knob, element size and a sweep of CU counts and lengths, no launch the plan asks for can be refused for its
// partials, the chunk loop of k_gramstep hands every chunk out exactly once, and the profile's model stays inside its list of moves.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../coordinatedescent.jl_amd/csrc/sweep_plan.hpp"

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { if (++g_bad < 20) fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

// compile time: the plan is constexpr, and these are the numbers the comments quote
static_assert(sweep_sizes(true, 3000, 5000, 256).blockB == 64 && sweep_sizes(true, 262144, 50, 256).blockB == 32, "");
static_assert(sweep_sizes(false, 3000, 50, 256).blockB == 32 && kWide64Rows == 262144, "");
static_assert(gram_plan(1500, 3000, 256, 4, 8, 2, 0).variant == kGramLtShort && gram_plan(1500, 3000, 256, 4, 8, 2, 0).nchunks == 94, "");
static_assert(sp_gram_rec(4) == 2625 && sp_gram_rec(2) == 801 && sp_gram_rec(1) == 273 && sp_block_rec(8) == 45, "");

int main() {
    const int cuss[] = {1, 2, 7, 8, 64, 104, 256, 304, 1024};
    const int64_t ns[] = {1, 2, 31, 32, 33, 127, 128, 129, 511, 512, 513, 3000, 4099, 65535, 65536, 65537, 262143, 262144, 262145,
                          999999, 1999999, 2000000, 2000001, 10000000, 10000019, (int64_t)1 << 31, ((int64_t)1 << 33) + 5};
    long plans = 0;
    for (int cus : cuss) for (int f64 = 0; f64 < 2; ++f64) for (int64_t n : ns) {
        const int esz = f64 ? 8 : 4;
        const SweepSizes s = sweep_sizes(f64, n, 70, cus);
        EXPECT(s.ld >= n && s.ld % 32 == 0 && s.ld - n < 32 && s.nvec * (16 / esz) >= n && (s.nvec - 1) * (16 / esz) < n);
        EXPECT(s.step_grid >= 1 && (size_t)s.step_grid * kSpNSum <= s.partials_doubles);
        EXPECT(s.block_grid >= 1 && (size_t)s.block_grid * sp_block_rec(kMaxBlockB) <= s.partials_doubles);
        EXPECT((size_t)elementwise_grid(s.nvec, kMomentsGridCap) * kSpNSum <= s.partials_doubles);
        EXPECT((size_t)gram_read_grid(s.nvec, cus) * sp_gram_rec(4) <= s.partials_doubles);
        for (int64_t bc : {(int64_t)1, (int64_t)7, (int64_t)8, (int64_t)9, (int64_t)4095, kSpColBatch}) for (int width = 1; width <= 2; ++width) {
            const ColDotsPlan c = col_dots_plan(bc, s.nvec, cus, width);
            EXPECT(c.chunks >= 1 && c.chunks <= kSpColChunks && c.groups * kSpColGroup >= bc && c.doubles <= s.partials_doubles);
        }
        for (int NG : {1, 2, 4}) for (int lt = 0; lt < 3; ++lt) for (int ks = 0; ks < 3; ++ks) {
            const GramPlan g = gram_plan(s.nvec, n, cus, NG, esz, lt, ks);
            ++plans;
            EXPECT((size_t)g.grid * sp_gram_rec(NG) <= s.partials_doubles);
            EXPECT(g.cvn * g.nchunks >= s.nvec && s.nvec > g.cvn * (g.nchunks - 1));
            EXPECT(!(NG == 4 && esz == 4) || g.variant == kGramFrag);
            EXPECT(NG >= 2 || g.variant != kGramLtShort);
            EXPECT(g.grid >= 1 && g.grid <= cus * gram_blocks_per_cu(NG, g.variant != kGramFrag));
            if (g.nchunks > 40000) continue;   // (up to 1e6 rows at every chunk length; the Python test replays the longer ones it lists)
            // the kernel's loop: wave w of block b takes chunks w * G + b, + kGramWaves * G, ...
            std::vector<unsigned char> taken((size_t)g.nchunks, 0);
            int64_t most = 0;
            for (int b = 0; b < g.grid; ++b) for (int w = 0; w < kSpGramWaves; ++w) {
                int64_t trips = 0;
                for (int64_t ch = (int64_t)w * g.grid + b; ch < g.nchunks; ch += (int64_t)g.grid * kSpGramWaves) { ++taken[(size_t)ch]; ++trips; }
                if (trips > most) most = trips;
            }
            bool once = true;
            for (unsigned char t : taken) once = once && t == 1;
            EXPECT(once);
            EXPECT(most == g.rounds);
        }
    }
    // the profile's model reads hs[0 .. m) and nothing else (the vector is exactly m long: the sanitizer watches its ends)
    for (int B : {1, 2, 4, 8, 16, 32, 64}) for (int m : {1, B - 1, B, B + 1, 2 * B + 6}) {
        if (m < 1) continue;
        std::vector<double> hs((size_t)m, 1.0);
        const ChunkTraffic t = chunk_traffic(B > 1, B, m, false, hs.data(), 1000, 8);
        EXPECT(t.launches == (B > 1 ? (m + B - 1) / B : m) && t.bytes > 0.0);
        const ChunkRoute r = chunk_route(B > 1, B, false, m, 0, false);
        EXPECT(r.rewrites == t.launches + 1 && (r.key >> 20) == (uint64_t)m);
    }
    if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    printf("sweep_plan_main OK (%ld wide-block plans)\n", plans);
    return 0;
}
