// glm_plan.hpp -- the host-only arithmetic of the IRLS step exports (glm_kernels.hpp: k_glm_step): how the rows of the handle's vectors
// are dealt to the workgroups, how many workgroups run and how many partial records they leave.  No HIP in here:
// tests/test_glm_host.py compiles it with g++ (tests/glm_plan_main.cpp).  glm_kernels.hpp calls these functions and nothing
// else decides the sizes.
#pragma once
#include <float.h>
#include <stdint.h>

// ---- the kernel's shape ------------------------------------------------------------------------------------------------------
// A lane takes one 16-byte vector of two doubles per trip, a workgroup of kGlmBlock lanes a tile of kGlmRows consecutive rows.
// The rows planned are the padded ld of the handle (a multiple of 32, so whole vectors): rows n .. ld - 1 are written as zeros
// by the lanes that hold them.  Workgroup b takes tiles b, b + grid, b + 2 grid, ... -- its strides -- and leaves ONE record
// of kGlmVals doubles (sum nll, sum w, clamped rows) at partials + b kGlmVals; k_gram_reduce sums the records in block order.
constexpr int kGlmBlock = 256;
constexpr int kGlmVec = 2;                                // doubles per 16-byte vector
constexpr int64_t kGlmRows = (int64_t)kGlmBlock * kGlmVec; // a workgroup's share of rows per stride
constexpr int64_t kGlmMaxGrid = 1024;                     // four workgroups per CU of 256
constexpr int kGlmVals = 3;
// the record of the fold-aware binomial step (GlmBinomialFold): (nll of the training rows, sum w, clamped rows, nll of the held-out
// rows, misclassified held-out rows); same grid, same tiles, one record per workgroup
constexpr int kGlmFoldVals = 5;
// the record of the Poisson step (GlmPoisson): (nll of the training rows, sum w, training rows clamped at wmin, live rows
// capped at eta_max, deviance of the held-out rows, deviance of the training rows); same grid, same tiles, one record per
// workgroup
constexpr int kGlmPoisVals = 6;

struct GlmPlan {
    int64_t vecs;      // 16-byte vectors over the ld rows
    int64_t tiles;     // tiles of kGlmRows rows (the last may be short)
    int64_t grid;      // workgroups: min(tiles, cap), at least 1
    int64_t records;   // partial records: one per workgroup
    int64_t strides;   // trips of workgroup 0 (the most any workgroup makes)
};

// cap: kGlmMaxGrid, or the smaller grid a test asks for (CDH_GLM_GRID); values outside 1 .. kGlmMaxGrid mean kGlmMaxGrid
constexpr int64_t glm_grid_cap(int64_t cap) { return (cap < 1 || cap > kGlmMaxGrid) ? kGlmMaxGrid : cap; }

constexpr GlmPlan glm_plan(int64_t ld, int64_t cap = kGlmMaxGrid) {
    const int64_t vecs = (ld + kGlmVec - 1) / kGlmVec;
    const int64_t tiles = (ld + kGlmRows - 1) / kGlmRows;
    const int64_t c = glm_grid_cap(cap);
    int64_t grid = tiles < c ? tiles : c;
    if (grid < 1) grid = 1;
    return GlmPlan{vecs, tiles, grid, grid, (tiles + grid - 1) / grid};
}

// rows [first, end) of workgroup b's t-th stride (empty when the tile lies beyond ld)
constexpr int64_t glm_rows_first(const GlmPlan& pl, int64_t ld, int64_t b, int64_t t) {
    const int64_t r = (b + t * pl.grid) * kGlmRows;
    return r < ld ? r : ld;
}
constexpr int64_t glm_rows_end(const GlmPlan& pl, int64_t ld, int64_t b, int64_t t) {
    const int64_t r = (b + t * pl.grid + 1) * kGlmRows;
    return r < ld ? r : ld;
}

// ---- observation weights -------------------------------------------------------------------------------------------------------
// what cdh_glm_set_weights refuses: the index of the first weight that is not finite or not > 0 (a NaN fails both comparisons;
// a denormal is a weight like any other), or n when there is none
inline int64_t glm_first_bad_weight(const double* v, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!(v[i] > 0.0 && v[i] <= DBL_MAX)) return i;
    return n;
}
