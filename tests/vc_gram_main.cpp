// Stand-alone check of csrc/vc_gram_types.hpp under the host sanitizers (tests/test_vc_gram_host.py builds and runs it): the
// scatter of every (Q, mb) from records whose entries encode where they belong, into exactly-sized heap blocks, so that an
// index out of range is an ASan report and a wrong one a wrong number; the record layout without gaps or overlaps; every
// refusal of the argument check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../coordinatedescent.jl_amd/csrc/vc_gram_types.hpp"

static int fails = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); ++fails; } \
    } while (0)

static double code_M(int s, int64_t j, int64_t k) { return 1e6 * (s + 1) + 1e3 * (j + 1) + (k + 1); }   // j <= k
static double code_m(int a, int64_t j) { return -(1e3 * (a + 1) + (j + 1)); }

int main() {
    const int64_t mbs[] = {1, 2, 3, 64};
    for (int Q = 0; Q <= kVgMaxDegree; ++Q)
        for (int64_t mb : mbs) {
            const VcGramRec R = vc_gram_rec(Q, mb);
            std::vector<double> rec((size_t)R.n, 0.0);
            std::vector<int> hits((size_t)R.n, 0);
            for (int s = 0; s <= 2 * Q; ++s)
                for (int64_t j = 0; j < mb; ++j)
                    for (int64_t k = j; k < mb; ++k) {
                        const int64_t at = s * R.tri + vc_gram_tri(mb, j, k);
                        EXPECT(at >= 0 && at < R.off_m);
                        rec[(size_t)at] = code_M(s, j, k);
                        ++hits[(size_t)at];
                    }
            for (int a = 0; a <= Q; ++a)
                for (int64_t j = 0; j < mb; ++j) { rec[(size_t)(R.off_m + a * mb + j)] = code_m(a, j); ++hits[(size_t)(R.off_m + a * mb + j)]; }
            ++hits[(size_t)R.off_w];
            for (int v : hits) EXPECT(v == 1);                       // every entry of the record has exactly one owner
            const int64_t Q1 = Q + 1, ep = mb * Q1;
            double* G = (double*)std::malloc(sizeof(double) * (size_t)(ep * ep));
            double* c = (double*)std::malloc(sizeof(double) * (size_t)ep);
            vc_gram_scatter(Q, mb, rec.data(), G, c);
            for (int64_t j = 0; j < mb; ++j)
                for (int64_t a = 0; a < Q1; ++a) {
                    EXPECT(c[j * Q1 + a] == code_m((int)a, j));
                    for (int64_t k = 0; k < mb; ++k)
                        for (int64_t b = 0; b < Q1; ++b) {
                            const double want = code_M((int)(a + b), j < k ? j : k, j < k ? k : j);
                            EXPECT(G[(k * Q1 + b) * ep + j * Q1 + a] == want);
                            EXPECT(G[(j * Q1 + a) * ep + k * Q1 + b] == want);
                        }
                }
            vc_gram_scatter(Q, mb, rec.data(), G, nullptr);          // c may be NULL
            std::free(G);
            std::free(c);
            EXPECT((int64_t)vc_gram_grid(1 << 20, Q, mb) * R.n <= kVgPartialDoubles);
            EXPECT(vc_gram_pairs(mb) * vc_gram_slices(mb) <= kVgThreads && vc_gram_slices(mb) >= 1);
        }
    // the refusals, one argument wrong at a time
    int64_t* idx = (int64_t*)std::malloc(sizeof(int64_t) * 3);
    idx[0] = 3; idx[1] = 1; idx[2] = 3;
    auto chk = [&](int deg, bool yset, bool wantc, int kind, double h, double z0, int64_t lo, int wpow, int64_t mb) {
        return vc_gram_check(deg, yset, wantc, 3, 10, kind, h, z0, lo, wpow, mb, idx);
    };
    EXPECT(chk(1, true, true, 0, 0.5, 0.1, -1, 1, 3) == nullptr);
    EXPECT(chk(1, false, false, 1, 0.5, 0.1, 9, 2, 3) == nullptr);
    EXPECT(chk(-1, true, true, 0, 0.5, 0.1, -1, 1, 3) != nullptr);
    EXPECT(chk(1, false, true, 0, 0.5, 0.1, -1, 1, 3) != nullptr);
    EXPECT(chk(1, true, true, 2, 0.5, 0.1, -1, 1, 3) != nullptr);
    EXPECT(chk(1, true, true, -1, 0.5, 0.1, -1, 1, 3) != nullptr);
    EXPECT(chk(1, true, true, 0, 0.0, 0.1, -1, 1, 3) != nullptr);
    EXPECT(chk(1, true, true, 0, -1.0, 0.1, -1, 1, 3) != nullptr);
    EXPECT(chk(1, true, true, 0, 0.5, 0.1, -1, 0, 3) != nullptr);
    EXPECT(chk(1, true, true, 0, 0.5, 0.1, -1, 3, 3) != nullptr);
    EXPECT(chk(1, true, true, 0, 0.5, 0.1, 10, 1, 3) != nullptr);
    EXPECT(chk(1, true, true, 0, 0.5, 0.1, -2, 1, 3) != nullptr);
    EXPECT(chk(1, true, true, 0, 0.5, 0.1, -1, 1, 0) != nullptr);
    EXPECT(chk(1, true, true, 0, 0.5, 0.1, -1, 1, 65) != nullptr);
    idx[1] = 0;
    EXPECT(chk(1, true, true, 0, 0.5, 0.1, -1, 1, 3) != nullptr);
    idx[1] = 4;
    EXPECT(chk(1, true, true, 0, 0.5, 0.1, -1, 1, 3) != nullptr);
    EXPECT(chk(1, true, true, 0, 0.5, 0.1, -1, 1, 1) == nullptr);   // ... and only the listed mb entries are read
    std::free(idx);
    std::printf(fails ? "vc_gram_main: %d FAILED\n" : "vc_gram_main OK\n", fails);
    return fails ? 1 : 0;
}
