// Stand-alone check of csrc/glm_plan.hpp (tests/test_glm_host.py builds and runs it under the host sanitizers): for every n in
// 1 .. 600 and a few around each constant of the plan, at the full grid cap and at small ones, the workgroups' row ranges are
// walked the way k_glm_step walks them over an exactly-sized heap block of ld rows -- a range that leaves the block is an ASan
// report -- and must cover [0, n), and [n, ld), exactly once; the record count must be the grid.  With arguments
// "ld cap ld cap ..." it prints the plan of each pair instead, one line each, for tests/_glm_plan.py to be held to.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../coordinatedescent.jl_amd/csrc/glm_plan.hpp"

static int fails = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); ++fails; } \
    } while (0)

static int64_t padded(int64_t n) { return (n + 31) / 32 * 32; }      // the handle's ld: columns start 256-byte aligned

static void walk(int64_t n, int64_t cap) {
    const int64_t ld = padded(n);
    const GlmPlan pl = glm_plan(ld, cap);
    const int64_t c = glm_grid_cap(cap);
    EXPECT(pl.vecs * kGlmVec == ld);
    EXPECT(pl.tiles == (ld + kGlmRows - 1) / kGlmRows && pl.tiles >= 1);
    EXPECT(pl.grid >= 1 && pl.grid <= c && pl.grid <= pl.tiles && (pl.grid == pl.tiles || pl.grid == c));
    EXPECT(pl.records == pl.grid);
    EXPECT(pl.strides == (pl.tiles + pl.grid - 1) / pl.grid && pl.strides >= 1);
    unsigned char* seen = (unsigned char*)std::calloc((size_t)ld, 1);
    double* partials = (double*)std::malloc(sizeof(double) * (size_t)(pl.records * kGlmVals));
    for (int64_t b = 0; b < pl.grid; ++b) {
        // the kernel's own loop: lane t of workgroup b takes vectors b kGlmBlock + t + s grid kGlmBlock while below vecs
        int64_t trips = 0;
        for (int64_t t = 0;; ++t) {
            const int64_t first = glm_rows_first(pl, ld, b, t), end = glm_rows_end(pl, ld, b, t);
            if (first >= end) break;
            ++trips;
            EXPECT(first == (b + t * pl.grid) * kGlmRows && end - first <= kGlmRows);
            for (int64_t lane = 0; lane < kGlmBlock; ++lane) {
                const int64_t j = (b + t * pl.grid) * kGlmBlock + lane;
                if (j >= pl.vecs) break;
                for (int e = 0; e < kGlmVec; ++e) {
                    EXPECT(j * kGlmVec + e >= first && j * kGlmVec + e < end);
                    ++seen[j * kGlmVec + e];
                }
            }
        }
        EXPECT(trips <= pl.strides && (b != 0 || trips == pl.strides));
        for (int i = 0; i < kGlmVals; ++i) partials[b * kGlmVals + i] = (double)trips;
    }
    for (int64_t i = 0; i < ld; ++i) EXPECT(seen[i] == 1);      // [0, n) and the pad rows [n, ld), each exactly once
    std::free(seen);
    std::free(partials);
}

int main(int argc, char** argv) {
    if (argc > 1) {
        for (int a = 1; a + 1 < argc; a += 2) {
            const int64_t ld = std::atoll(argv[a]), cap = std::atoll(argv[a + 1]);
            const GlmPlan pl = glm_plan(ld, cap);
            std::printf("%lld %lld %lld %lld %lld %lld %lld\n", (long long)ld, (long long)cap, (long long)pl.vecs, (long long)pl.tiles,
                        (long long)pl.grid, (long long)pl.records, (long long)pl.strides);
        }
        return 0;
    }
    const int64_t caps[] = {kGlmMaxGrid, 1, 2, 3};
    for (int64_t cap : caps) {
        for (int64_t n = 1; n <= 600; ++n) walk(n, cap);
        const int64_t around[] = {kGlmRows, 2 * kGlmRows, 3 * kGlmRows, 4 * kGlmRows};
        for (int64_t m : around)
            for (int64_t d = -33; d <= 33; ++d) walk(m + d, cap);
    }
    const int64_t near[] = {-33, -32, -31, -1, 0, 1, 31, 32, 33};
    for (int64_t d : near) walk(kGlmMaxGrid * kGlmRows + d, kGlmMaxGrid);                   // the grid cap itself
    walk(2 * kGlmMaxGrid * kGlmRows + 1, kGlmMaxGrid);
    // the constants the documents quote, the cap's domain, and where the second stride begins
    EXPECT(kGlmBlock == 256 && kGlmVec == 2 && kGlmRows == 512 && kGlmMaxGrid == 1024 && kGlmVals == 3);
    EXPECT(glm_grid_cap(0) == kGlmMaxGrid && glm_grid_cap(-5) == kGlmMaxGrid && glm_grid_cap(kGlmMaxGrid + 1) == kGlmMaxGrid);
    EXPECT(glm_grid_cap(1) == 1 && glm_grid_cap(kGlmMaxGrid) == kGlmMaxGrid);
    EXPECT(glm_plan(kGlmRows).grid == 1 && glm_plan(kGlmRows + 32).grid == 2);
    EXPECT(glm_plan(kGlmMaxGrid * kGlmRows).strides == 1 && glm_plan(kGlmMaxGrid * kGlmRows + 32).strides == 2);
    EXPECT(glm_plan(kGlmMaxGrid * kGlmRows + 32).grid == kGlmMaxGrid);
    EXPECT(glm_plan(2 * kGlmRows, 2).strides == 1 && glm_plan(2 * kGlmRows + 32, 2).strides == 2);
    std::printf(fails ? "glm_plan_main: %d FAILED\n" : "glm_plan_main OK rows=%d\n", fails ? fails : (int)kGlmRows);
    return fails ? 1 : 0;
}
