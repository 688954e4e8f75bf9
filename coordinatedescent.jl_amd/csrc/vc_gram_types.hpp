// vc_gram_types.hpp -- the host-only arithmetic of cdh_vc_gram (vc_gram.hpp): the argument checks, how a launch splits its
// rows, the size and layout of the partial records, and the scatter from the moments (M_s, m_a) to the expanded Gram matrix
// and right-hand side.  No HIP in here: tests/test_vc_gram_host.py compiles it with g++ (a shim for ctypes, and a stand-alone
// program under the host sanitizers).
//
// With d_i = z_i - z0 and w_i the weight of row i, the weighted Gram matrix of the expanded design (reference
// varying_coefficient_lasso.jl:572-620, _expand_Xt_w_X!) and its right-hand side (:622-647, _expand_Xt_w_Y!) are
//   G[(j,a),(k,b)] = sum_i w_i x_ij x_ik d_i^(a+b) = M_{a+b}[j,k],      c[(j,a)] = sum_i w_i x_ij y_i d_i^a = m_a[j],
// j, k over the mb listed base columns, a, b = 0 .. Q: 2Q + 1 symmetric mb x mb moment matrices and Q + 1 vectors.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int kVgMaxCols = 64;                   // base columns per call (CDH_VC_GRAM_MAX_COLS)
constexpr int kVgMaxDegree = 3;
constexpr int kVgRows = 64;                      // rows of one chunk: what a workgroup stages in LDS at a time
constexpr int kVgTile = 4;                       // a thread owns a kVgTile x kVgTile tile of every moment matrix
constexpr int kVgThreads = 256;
constexpr int kVgMaxBlocks = 512;                // workgroups of a launch, at most
constexpr int64_t kVgPartialDoubles = (int64_t)1 << 21;    // the partial records of a launch fit 16 MiB

// One record: the upper triangles of M_0 .. M_2Q (row-major: (j, k), j <= k, at j mb - j (j - 1) / 2 + k - j), then m_0 .. m_Q
// (mb each), then sum_i w_i.
struct VcGramRec {
    int64_t tri, off_m, off_w, n;                // entries of one triangle; where m_0 and sum w start; doubles in all
};
constexpr VcGramRec vc_gram_rec(int Q, int64_t mb) {
    VcGramRec r{};
    r.tri = mb * (mb + 1) / 2;
    r.off_m = (2 * Q + 1) * r.tri;
    r.off_w = r.off_m + (Q + 1) * mb;
    r.n = r.off_w + 1;
    return r;
}
constexpr int64_t vc_gram_tri(int64_t mb, int64_t j, int64_t k) { return j * mb - j * (j - 1) / 2 + (k - j); }   // j <= k < mb
static_assert(vc_gram_rec(kVgMaxDegree, kVgMaxCols).n * 8 <= kVgPartialDoubles, "eight records of the largest call fit");

// The columns a workgroup works on: the mb listed ones, y (zeros without it) and a column of ones, so that m_a = M_a[., y]
// and sum w = M_0[1, 1] come out of the same loop.  They are cut into kVgTile-wide groups; a thread owns one pair of groups
// (bj <= bk), and the S slices of threads that share a pair split a chunk's rows between them.
constexpr int vc_gram_groups(int64_t mb) { return (int)((mb + 2 + kVgTile - 1) / kVgTile); }
constexpr int vc_gram_pairs(int64_t mb) { return vc_gram_groups(mb) * (vc_gram_groups(mb) + 1) / 2; }
constexpr int vc_gram_slices(int64_t mb) {
    const int s = kVgThreads / vc_gram_pairs(mb);
    return s < kVgRows ? s : kVgRows;
}
static_assert(vc_gram_pairs(kVgMaxCols) <= kVgThreads && vc_gram_slices(kVgMaxCols) == 1 && vc_gram_slices(1) == kVgRows, "");

// Workgroups of a launch over n rows: one per chunk until kVgMaxBlocks or the partial buffer is reached, chunks dealt round robin.
constexpr int64_t vc_gram_chunks(int64_t n) { return (n + kVgRows - 1) / kVgRows; }
constexpr int vc_gram_grid(int64_t n, int Q, int64_t mb) {
    int64_t g = vc_gram_chunks(n);
    if (g > kVgMaxBlocks) g = kVgMaxBlocks;
    const int64_t fit = kVgPartialDoubles / vc_gram_rec(Q, mb).n;
    if (g > fit) g = fit;
    return (int)(g < 1 ? 1 : g);
}
// L: the longest chain of sequential additions an output entry goes through (vc_gram.hpp states the formula)
constexpr int64_t vc_gram_chain(int64_t n, int Q, int64_t mb) {
    const int64_t G = vc_gram_grid(n, Q, mb), S = vc_gram_slices(mb);
    return (vc_gram_chunks(n) + G - 1) / G * ((kVgRows + S - 1) / S) + S + (G + 3) / 4 + 2;
}

// ---- argument checks: a message for what is refused, NULL for what is accepted ---------------------------------------------
// vc_degree: the handle's (-1 before cdh_vc_set_data); y_set: cdh_set_y has run; want_c: out_c is not NULL
inline const char* vc_gram_check(int vc_degree, bool y_set, bool want_c, int64_t p_base, int64_t n, int32_t kernel_kind,
                                 double bandwidth, double z0, int64_t leave_out_row0, int32_t wpow, int64_t mb,
                                 const int64_t* base_idx1) {
    if (vc_degree < 0) return "cdh_vc_gram needs cdh_vc_set_data first";
    if (vc_degree > kVgMaxDegree) return "cdh_vc_gram: the polynomial degree must be 0 .. 3";
    if (want_c && !y_set) return "cdh_vc_gram: the right-hand side needs y: cdh_set_y first";
    if (kernel_kind != 0 && kernel_kind != 1) return "cdh_vc_gram: unknown smoothing kernel";
    if (!(bandwidth > 0.0) || bandwidth > 1.7976931348623157e308) return "cdh_vc_gram: the bandwidth must be positive";
    if (wpow != 1 && wpow != 2) return "cdh_vc_gram: wpow must be 1 or 2";
    if (leave_out_row0 < -1 || leave_out_row0 >= n) return "cdh_vc_gram: the left-out row is outside 0 .. n - 1";
    if (leave_out_row0 < 0 && !(z0 - z0 == 0.0)) return "cdh_vc_gram: z0 must be finite";
    if (mb < 1 || mb > kVgMaxCols) return "cdh_vc_gram: need 1 <= mb <= 64 base columns";
    for (int64_t i = 0; i < mb; ++i)
        if (base_idx1[i] < 1 || base_idx1[i] > p_base) return "cdh_vc_gram: a base column is outside 1 .. p_base";
    return nullptr;
}

// ---- the scatter: (M_s, m_a) of one record -> G (column-major ep x ep, ep = mb (Q + 1), both triangles) and c, in the
// expanded order (j, a) -> j (Q + 1) + a of the listed columns.  c may be NULL.
inline void vc_gram_scatter(int Q, int64_t mb, const double* rec, double* G, double* c) {
    const VcGramRec R = vc_gram_rec(Q, mb);
    const int64_t Q1 = Q + 1, ep = mb * Q1;
    for (int64_t k = 0; k < mb; ++k)
        for (int64_t b = 0; b < Q1; ++b)
            for (int64_t j = 0; j < mb; ++j) {
                const int64_t t = j <= k ? vc_gram_tri(mb, j, k) : vc_gram_tri(mb, k, j);
                for (int64_t a = 0; a < Q1; ++a) G[(k * Q1 + b) * ep + j * Q1 + a] = rec[(a + b) * R.tri + t];
            }
    if (c)
        for (int64_t j = 0; j < mb; ++j)
            for (int64_t a = 0; a < Q1; ++a) c[j * Q1 + a] = rec[R.off_m + a * mb + j];
}
