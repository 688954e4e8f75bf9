// Stand-alone check of csrc/cv_plan.hpp under the host sanitizers (tests/test_cv_host.py builds and runs it): for every
// (s, m) at the edges of the grouping, the packed image of B, the partial records and the kernel's LDS tile are laid out in
// exactly-sized heap blocks and written the way cv_path.hpp writes them -- a plan that is too small is an ASan report -- the
// groups are checked to cover 0 .. m exactly once, and the limits' messages to name the numbers the header defines.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../coordinatedescent.jl_amd/csrc/cv_plan.hpp"

static int fails = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); ++fails; } \
    } while (0)

static void walk(int64_t n, int64_t s, int64_t m, bool image) {
    const CvPlan pl = cv_plan(n, s, m);
    EXPECT(pl.refused == nullptr);
    if (pl.refused) return;
    const int64_t G = kCvGroup;
    // the groups cover 0 .. m exactly once
    std::vector<int> seen((size_t)m, 0);
    EXPECT(pl.groups == (m + G - 1) / G && pl.mpad == pl.groups * G && pl.nvals == 2 * pl.mpad);
    for (int64_t g = 0; g < pl.groups; ++g) {
        const int64_t w = cv_group_width(m, g);
        EXPECT(w >= 1 && w <= G);
        for (int64_t j = cv_group_first(g); j < cv_group_first(g) + w; ++j) ++seen[(size_t)j];
    }
    EXPECT(cv_group_width(m, pl.groups) == 0);
    for (int64_t j = 0; j < m; ++j) EXPECT(seen[(size_t)j] == 1);
    // the packed image of B: every (t, j) has a slot of its own, rows s .. srows - 1 are padding
    EXPECT(pl.srows >= s && pl.srows < s + kCvUnroll && pl.srows % kCvUnroll == 0);
    EXPECT(pl.b_doubles == pl.groups * pl.srows * G);
    double* Bp = (double*)std::calloc((size_t)pl.b_doubles, sizeof(double));
    for (int64_t j = 0; image && j < m; ++j)      // (a function of s and m alone: walked once per pair)
        for (int64_t t = 0; t < s; ++t) {
            const int64_t at = cv_b_index(pl.srows, t, j);
            EXPECT(at >= 0 && at < pl.b_doubles && Bp[at] == 0.0);
            Bp[at] = 1.0;
            EXPECT(at == ((j / G) * pl.srows + t) * G + j % G);      // what the kernel reads: Bg + t G + jj of group j / G
        }
    std::free(Bp);
    // the partial records: workgroup b writes [held][train] at col0 + column for each of its groups
    EXPECT(pl.tiles == (n + kCvRows - 1) / kCvRows);
    EXPECT(pl.grid >= 1 && pl.grid <= kCvMaxGrid && pl.grid <= pl.tiles);
    EXPECT(pl.partial_doubles == pl.grid * pl.nvals && pl.partial_doubles <= kCvPartialDoubles);
    EXPECT(pl.grid == pl.tiles || pl.grid == kCvMaxGrid || (pl.grid + 1) * pl.nvals > kCvPartialDoubles);
    double* part = (double*)std::malloc(sizeof(double) * (size_t)pl.partial_doubles);
    for (int64_t b = 0; b < pl.grid; b += (pl.grid > 8 ? pl.grid - 1 : 1))
        for (int64_t g = 0; g < pl.groups; ++g)
            for (int64_t c = 0; c < G; ++c) {
                double* rec = part + b * pl.nvals + cv_group_first(g) + c;
                rec[0] = 1.0;
                rec[pl.mpad] = 2.0;
            }
    std::free(part);
    EXPECT(pl.nvals <= kCvMaxVals);
    // the LDS tile: [kCvChunk][kCvStride], lane tid writes column jj at jj kCvStride + tid; lane (c, q) reads c kCvStride + q + 16 u
    EXPECT(pl.lds_bytes == kCvLdsBytes && pl.lds_bytes <= kCvLdsBudget);
    double* lds = (double*)std::malloc(pl.lds_bytes);
    for (int jj = 0; jj < kCvChunk; ++jj)
        for (int tid = 0; tid < kCvRows; ++tid) lds[jj * kCvStride + tid] = (double)tid;
    for (int tid = 0; tid < kCvRows; ++tid)
        for (int u = 0; u < 16; ++u) EXPECT(lds[(tid >> 4) * kCvStride + (tid & 15) + 16 * u] == (double)((tid & 15) + 16 * u));
    std::free(lds);
}

int main() {
    const int64_t G = kCvGroup;
    const int64_t ss[] = {1, 2, 63, 64, 65, kCvMaxS};
    const int64_t ms[] = {1, G - 1, G, G + 1, 2 * G + 1, kCvMaxM};
    const int64_t ns[] = {1, kCvRows - 1, kCvRows, kCvRows + 1, kCvRows * kCvMaxGrid - 1, kCvRows * kCvMaxGrid, kCvRows * kCvMaxGrid + 1,
                          2000000};
    for (int64_t s : ss)
        for (int64_t m : ms)
            for (int64_t n : ns) walk(n, s, m, n == ns[0]);
    // the grid wraps where the tiles outnumber it, and the widest call is held back by the buffer
    EXPECT(cv_plan(kCvRows * kCvMaxGrid, 1, 1).grid == kCvMaxGrid && cv_plan(kCvRows * kCvMaxGrid + 1, 1, 1).tiles == kCvMaxGrid + 1);
    EXPECT(cv_plan(2000000, 64, kCvMaxM).grid == kCvPartialDoubles / kCvMaxVals);
    // the limits, and the messages that name them
    auto names = [](const char* msg, long long v) { return msg && std::string(msg).find(std::to_string(v)) != std::string::npos; };
    EXPECT(names(cv_plan(10, 0, 1).refused, kCvMaxS) && names(cv_plan(10, kCvMaxS + 1, 1).refused, kCvMaxS));
    EXPECT(names(cv_plan(10, 1, 0).refused, kCvMaxM) && names(cv_plan(10, 1, kCvMaxM + 1).refused, kCvMaxM));
    EXPECT(cv_plan(0, 1, 1).refused != nullptr);
    EXPECT(cv_plan(10, kCvMaxS, kCvMaxM).refused == nullptr);
    EXPECT(names(cv_check_K(1000, 1), kCvMinK) && names(cv_check_K(1000, kCvMaxK + 1), kCvMaxK) && cv_check_K(3, 4) != nullptr);
    EXPECT(cv_check_K(1000, kCvMinK) == nullptr && cv_check_K(1000, kCvMaxK) == nullptr && cv_check_K(2, 2) == nullptr);
    EXPECT(kCvMaxS == 4096 && kCvMaxM == 1024 && kCvMaxK == 255);
    std::printf(fails ? "cv_plan_main: %d FAILED\n" : "cv_plan_main OK G=%d\n", fails ? fails : kCvGroup);
    return fails ? 1 : 0;
}
