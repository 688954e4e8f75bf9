// vc_gram_batch_types.hpp -- the host-only arithmetic of cdh_vc_gram_batch (vc_gram.hpp: k_vc_moments): the argument
// check of a batch of points and the plan of a call -- which regime applies, how the batch is cut into launch groups, how a
// group's points are dealt to the workgroups, and where every partial record sits.  No HIP in here:
// tests/test_vc_gram_batch_host.py compiles it with g++ (a shim for ctypes, and a stand-alone program under the host
// sanitizers).  The export calls these functions and nothing else decides the split.
//
// Point t of a batch is cdh_vc_gram at (bandwidth[t], z0[t], leave_out_row0[t]): the same deal of chunks to workgroups
// (vc_gram_grid), the same slices, the same record (vc_gram_rec) per workgroup, the same sum over the records.  So the plan only
// adds a point index in front of what vc_gram_types.hpp lays out: partial records are [point][workgroup][entry].
#pragma once
#include "vc_gram_types.hpp"

constexpr int64_t kVgbMaxPoints = 65536;                     // points of one call (CDH_VC_GRAM_MAX_POINTS)
constexpr int64_t kVgbPartialDoubles = (int64_t)1 << 24;     // the partial records of one launch group fit 128 MiB
constexpr int64_t kVgbOutDoubles = (int64_t)1 << 22;         // its summed records fit 32 MiB, on the device and pinned
constexpr int64_t kVgbMaxGroupPoints = 32768;                // points of one launch group, at most (grid.y stays below 65536)
// The resident regime deals a group's points to grid.y shares per chunk: shares = ceil(kVgbTargetBlocks / chunks), but no
// more than points / kVgbMinSharePoints.  A workgroup holds 74.5 KiB of LDS, so at most two fit a CU and 512 fill the chip's
// 256 CUs once; the target is twice that (a few workgroups per CU, so that a share that ends early is followed by another).
// A share is not made shorter than kVgbMinSharePoints points: below that, staging the chunk (mb + 2 column reads of 64 rows)
// costs as much as the points walked on it.
constexpr int64_t kVgbTargetBlocks = 1024;
constexpr int64_t kVgbMinSharePoints = 8;
static_assert(kVgPartialDoubles <= kVgbPartialDoubles && vc_gram_rec(kVgMaxDegree, kVgMaxCols).n <= kVgbOutDoubles, "");

// what the kernel reads per point
struct VcGramPoint {
    double z0, h;
    int64_t leave_out;                           // -1: none
};

// ---- the plan: all of it functions of (n, Q, mb, m) ---------------------------------------------------------------------------
// resident: every workgroup of the single-point deal holds one chunk, so a workgroup can stage it once and walk many points.
// This is the batch's question: cdh_vc_gram does not ask it and passes "streamed" at every n.  With one point a workgroup stages
// its chunk once either way, and the streamed instantiation keeps its smaller footprint (38.5 against 74.5 KiB of LDS, fewer
// registers: vc_gram.hpp), so the single point runs as it always has.
constexpr bool vgb_resident(int64_t n, int Q, int64_t mb) { return vc_gram_chunks(n) <= vc_gram_grid(n, Q, mb); }
// points of a full launch group: what the partial buffer, the summed-record buffer and kVgbMaxGroupPoints allow (>= 8: vc_gram_grid
// keeps G records within kVgPartialDoubles = kVgbPartialDoubles / 8)
constexpr int64_t vgb_group_points(int64_t n, int Q, int64_t mb) {
    const int64_t nrec = vc_gram_rec(Q, mb).n;
    int64_t g = kVgbPartialDoubles / (vc_gram_grid(n, Q, mb) * nrec);
    if (g > kVgbOutDoubles / nrec) g = kVgbOutDoubles / nrec;
    if (g > kVgbMaxGroupPoints) g = kVgbMaxGroupPoints;
    return g;
}
constexpr int64_t vgb_groups(int64_t n, int Q, int64_t mb, int64_t m) {
    return (m + vgb_group_points(n, Q, mb) - 1) / vgb_group_points(n, Q, mb);
}
// group g of a call over m points holds points first .. first + size - 1
constexpr int64_t vgb_group_first(int64_t n, int Q, int64_t mb, int64_t g) { return g * vgb_group_points(n, Q, mb); }
constexpr int64_t vgb_group_size(int64_t n, int Q, int64_t mb, int64_t m, int64_t g) {
    const int64_t left = m - vgb_group_first(n, Q, mb, g), full = vgb_group_points(n, Q, mb);
    return left < 0 ? 0 : left < full ? left : full;
}
// points a workgroup walks in a launch over `pts` points: 1 in the streamed regime (grid.y = the points); in the resident one
// ceil(pts / shares) with shares = ceil(kVgbTargetBlocks / chunks), but no more shares than pts / kVgbMinSharePoints
constexpr int64_t vgb_share_points(int64_t n, int Q, int64_t mb, int64_t pts) {
    if (!vgb_resident(n, Q, mb)) return 1;
    const int64_t G = vc_gram_grid(n, Q, mb);
    int64_t shares = (kVgbTargetBlocks + G - 1) / G;
    if (shares > pts / kVgbMinSharePoints) shares = pts / kVgbMinSharePoints;
    if (shares < 1) shares = 1;
    return (pts + shares - 1) / shares;
}
constexpr int64_t vgb_grid_y(int64_t n, int Q, int64_t mb, int64_t pts) {
    const int64_t per = vgb_share_points(n, Q, mb, pts);
    return (pts + per - 1) / per;
}
// share s of that launch walks points begin(s) .. begin(s + 1) - 1 of the group
constexpr int64_t vgb_share_begin(int64_t n, int Q, int64_t mb, int64_t pts, int64_t s) {
    const int64_t b = s * vgb_share_points(n, Q, mb, pts);
    return b < pts ? b : pts;
}
// where workgroup `block` leaves its record of the group's point `point`, in doubles from the start of the partial buffer
constexpr int64_t vgb_rec_offset(int64_t n, int Q, int64_t mb, int64_t point, int64_t block) {
    return (point * vc_gram_grid(n, Q, mb) + block) * vc_gram_rec(Q, mb).n;
}
// the scratch of the export: partial records, summed records (device and pinned), the points (device and pinned)
constexpr int64_t vgb_scratch_device_bytes() {
    return 8 * (kVgbPartialDoubles + kVgbOutDoubles) + (int64_t)sizeof(VcGramPoint) * kVgbMaxGroupPoints;
}
constexpr int64_t vgb_scratch_pinned_bytes() { return 8 * kVgbOutDoubles + (int64_t)sizeof(VcGramPoint) * kVgbMaxGroupPoints; }

// ---- the argument check of a batch: a message for what is refused (and the point it is about in *bad_point, -1 where it
// is about the call), NULL for what is accepted.  Per point it is vc_gram_check.
inline const char* vc_gram_batch_check(int vc_degree, bool y_set, bool want_c, int64_t p_base, int64_t n, int32_t kernel_kind,
                                       int64_t m, const double* bandwidth, const double* z0, const int64_t* leave_out_row0,
                                       int32_t wpow, int64_t mb, const int64_t* base_idx1, int64_t* bad_point) {
    *bad_point = -1;
    if (m < 1 || m > kVgbMaxPoints) return "cdh_vc_gram_batch: need 1 <= m <= 65536 points";
    if (!bandwidth) return "cdh_vc_gram_batch: bandwidth is NULL";
    if (!base_idx1) return "cdh_vc_gram_batch: base_idx1 is NULL";
    for (int64_t t = 0; t < m; ++t) {
        const int64_t lo = leave_out_row0 ? leave_out_row0[t] : -1;
        *bad_point = t;
        if (!z0 && lo == -1) return "cdh_vc_gram_batch: z0 is NULL and this point leaves no row out";
        if (const char* bad = vc_gram_check(vc_degree, y_set, want_c, p_base, n, kernel_kind, bandwidth[t], z0 ? z0[t] : 0.0, lo,
                                            wpow, mb, base_idx1))
            return bad;
    }
    *bad_point = -1;
    return nullptr;
}
