// cv_plan.hpp -- the host-only arithmetic of cdh_set_folds and cdh_path_sse (cv_path.hpp: k_path_sse): the limits and the
// messages that name them, how the m coefficient columns of a call are cut into groups of kCvGroup, the bytes of LDS the
// kernel's row tile takes, the packed image of B the kernel reads, and the grid against the capacity of the partial buffer.
// No HIP in here: tests/test_cv_host.py compiles it with g++ (tests/cv_plan_main.cpp, a stand-alone program under the host
// sanitizers).  cv_path.hpp calls these functions and nothing else decides the sizes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define CV_STR2(x) #x
#define CV_STR(x) CV_STR2(x)
#define CV_MAX_S 4096        /* coordinates of one call: cdh_gram's limit */
#define CV_MAX_M 1024        /* coefficient columns of one call */
#define CV_MIN_K 2
#define CV_MAX_K 255         /* fold ids are a byte per row; 255 marks nothing */

constexpr int64_t kCvMaxS = CV_MAX_S, kCvMaxM = CV_MAX_M;
constexpr int kCvMinK = CV_MIN_K, kCvMaxK = CV_MAX_K;
constexpr const char* kCvMsgS = "need 1 <= s <= " CV_STR(CV_MAX_S) " coordinates";
constexpr const char* kCvMsgM = "need 1 <= m <= " CV_STR(CV_MAX_M) " coefficient columns";
constexpr const char* kCvMsgK = "need " CV_STR(CV_MIN_K) " <= K <= " CV_STR(CV_MAX_K) " folds, and K <= n";

// ---- the kernel's shape ------------------------------------------------------------------------------------------------------
// A lane owns a row and keeps kCvGroup residuals y_i - sum_t X[i, t] B[t, j] as fp64 accumulators: 128 of the 512 registers a
// SIMD has per lane, which with the 8 columns of X in flight, the running sums and the addressing stays under 256 (two waves
// per SIMD) without scratch.  A workgroup of kCvRows lanes takes a tile of kCvRows rows at a time.  The squares leave the lanes
// through LDS kCvChunk columns at a time: [kCvChunk][kCvStride] doubles, kCvStride = kCvRows + 16 so that the transposed reads
// (lane (c, q) sums rows q, q + 16, ... of column c) of the two columns a half-wave covers fall on opposite halves of the banks.
constexpr int kCvGroup = 64;
constexpr int kCvRows = 256;
constexpr int kCvChunk = 16;
constexpr int kCvStride = kCvRows + 16;
constexpr int kCvUnroll = 8;                                   // columns of X a lane has in flight; B's rows are padded to it
constexpr size_t kCvLdsBytes = (size_t)kCvChunk * kCvStride * sizeof(double);
constexpr size_t kCvLdsBudget = (size_t)64 * 1024;             // what a kernel gets without asking
static_assert(kCvLdsBytes <= kCvLdsBudget && kCvGroup % kCvChunk == 0 && kCvRows / 16 == kCvChunk && kCvStride % 32 == 16, "");

// ---- partial records ---------------------------------------------------------------------------------------------------------
// Workgroup b writes one record of nvals = 2 mpad doubles at partials + b nvals: [held: mpad][train: mpad], mpad = m rounded up
// to whole groups; k_gram_reduce sums the records in a fixed order.  The buffer holds kCvPartialDoubles; the grid is the number
// of row tiles, capped by kCvMaxGrid (four workgroups per CU of 256) and by what the buffer holds.
constexpr int64_t kCvPartialDoubles = (int64_t)1 << 20;        // 8 MiB
constexpr int64_t kCvMaxGrid = 1024;
constexpr int64_t kCvMaxVals = 2 * ((kCvMaxM + kCvGroup - 1) / kCvGroup * kCvGroup);
static_assert(kCvMaxVals <= kCvPartialDoubles, "one record always fits");

struct CvPlan {
    const char* refused;     // nullptr, or why the call cannot run (names the limit)
    int64_t groups, mpad, nvals;
    int64_t tiles, grid;
    int64_t srows;           // rows of the packed B: s rounded up to kCvUnroll, the padding zero
    int64_t b_doubles;       // the packed image of B: [group][srows][kCvGroup]
    int64_t partial_doubles; // grid * nvals <= kCvPartialDoubles
    size_t lds_bytes;
};

constexpr int64_t cv_groups(int64_t m) { return (m + kCvGroup - 1) / kCvGroup; }
// group g holds columns first .. first + width - 1 of the call
constexpr int64_t cv_group_first(int64_t g) { return g * kCvGroup; }
constexpr int64_t cv_group_width(int64_t m, int64_t g) {
    const int64_t left = m - cv_group_first(g);
    return left < 0 ? 0 : left < kCvGroup ? left : kCvGroup;
}
constexpr int64_t cv_tiles(int64_t n) { return (n + kCvRows - 1) / kCvRows; }
constexpr int64_t cv_grid(int64_t n, int64_t m) {
    int64_t g = cv_tiles(n);
    const int64_t cap = kCvPartialDoubles / (2 * cv_groups(m) * kCvGroup);
    if (g > kCvMaxGrid) g = kCvMaxGrid;
    if (g > cap) g = cap;
    return g < 1 ? 1 : g;
}
// where B[t, j] of the call sits in the packed image
constexpr int64_t cv_b_index(int64_t srows, int64_t t, int64_t j) {
    return ((j / kCvGroup) * srows + t) * kCvGroup + j % kCvGroup;
}

constexpr CvPlan cv_plan(int64_t n, int64_t s, int64_t m) {
    if (n < 1) return CvPlan{"need n >= 1 rows", 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (s < 1 || s > kCvMaxS) return CvPlan{kCvMsgS, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (m < 1 || m > kCvMaxM) return CvPlan{kCvMsgM, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t groups = cv_groups(m), mpad = groups * kCvGroup, grid = cv_grid(n, m);
    const int64_t srows = (s + kCvUnroll - 1) / kCvUnroll * kCvUnroll;
    return CvPlan{nullptr, groups, mpad, 2 * mpad, cv_tiles(n), grid, srows, groups * srows * kCvGroup, grid * 2 * mpad, kCvLdsBytes};
}

// cdh_set_folds' argument check, before anything is allocated
constexpr const char* cv_check_K(int64_t n, int64_t K) { return (K < kCvMinK || K > kCvMaxK || K > n) ? kCvMsgK : nullptr; }
