// stats_plan.hpp -- the host-only arithmetic of the read-only statistics exports (col_stats.hpp) and of a varying-coefficient
// point (vc_host.hpp: vc_point): which launches a cdh_gram / cdh_gram_weighted call makes, which columns each holds and where
// its record goes in the caller's arrays; the batches of expanded columns a point is set up in, their base columns, row chunks
// and partial tables, and what the point counts towards cdh_profile_end.  No HIP in here: tests/test_stats_plan_host.py compiles
// it with g++ (tests/stats_plan_main.cpp) and holds it to tests/_stats_plan.py.  The launchers walk these plans and nothing
// else decides the numbers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sweep_plan.hpp"   // col_dots_plan, kSpColBatch: a point's batches are the column dots' batches

// ---- the Gram block of m listed columns (gram_block) ----------------------------------------------------------------------------
// Up to 64 columns: one launch of the wide-block kernel.  More (_findInitResiduals! takes any s, src/utils.jl:65-77): groups of
// 32 columns, one launch per PAIR of groups a < b, a outer -- the 64 columns of a pair give the pair's two diagonal blocks and
// the block between them.  A diagonal block comes out of every pair its group is in, each time from the same sums over the same
// rows.
constexpr int64_t kGramMaxCols = 4096;   // columns of a cdh_gram / cdh_gram_weighted / cdh_get_X_row call
constexpr int kGramGroupCols = 32;       // columns of a group
constexpr int kGramLaunchCols = 64;      // columns of a launch: GramRec<4>::B
// GramRec<4> (gram_kernels.hpp) restated: 10 upper-triangular 16 x 16 tiles row-major, the 64 dots, r'r.  cdhip.hip ties each
// to the name it has there.
constexpr int kGsOffC = 10 * 256, kGsOffQ = kGsOffC + kGramLaunchCols, kGsRec = kGsOffQ + 1;
constexpr int gs_g(int s, int l) {       // record offset of G[s][l], s <= l (positions inside the launch)
    const int gs = s >> 4, gl = l >> 4;
    return (gs * 4 - gs * (gs - 1) / 2 + (gl - gs)) * 256 + (s & 15) * 16 + (l & 15);
}

// One launch: positions [0, na) hold columns [a0, a0 + na) of the call's list, positions [na, na + nb) columns [b0, b0 + nb).
// The call of m <= 64 columns is the launch whose second group is empty.
struct GramLaunch {
    int64_t a0, b0;
    int na, nb;
    constexpr int cols() const { return na + nb; }
    constexpr int64_t col_of(int pos) const { return pos < na ? a0 + pos : b0 + (pos - na); }
};
constexpr int64_t gram_launches(int64_t m) {
    const int64_t ng = sp_ceil(m, kGramGroupCols);
    return m <= kGramLaunchCols ? 1 : ng * (ng - 1) / 2;
}
constexpr GramLaunch gram_launch_at(int64_t m, int64_t t) {     // t < gram_launches(m), in launch order
    if (m <= kGramLaunchCols) return GramLaunch{0, m, (int)m, 0};
    const int64_t ng = sp_ceil(m, kGramGroupCols);
    int64_t a = 0;
    while (t >= ng - 1 - a) { t -= ng - 1 - a; ++a; }
    const int64_t a0 = kGramGroupCols * a, b0 = kGramGroupCols * (a + 1 + t);
    return GramLaunch{a0, b0, (int)(sp_min(a0 + kGramGroupCols, m) - a0), (int)(sp_min(b0 + kGramGroupCols, m) - b0)};
}
// column -> position inside the launch; every block and dot the launch's record holds is written (out_c, out_q: or NULL)
constexpr void gram_scatter(const GramLaunch& L, int64_t m, const double* rec, double* out_G, double* out_c, double* out_q) {
    for (int pi = 0; pi < L.cols(); ++pi) {
        const int64_t i = L.col_of(pi);
        for (int pj = 0; pj < L.cols(); ++pj)
            out_G[i * m + L.col_of(pj)] = rec[gs_g(pi < pj ? pi : pj, pi < pj ? pj : pi)];
        if (out_c) out_c[i] = rec[kGsOffC + pi];
    }
    if (out_q) *out_q = rec[kGsOffQ];
}

// ---- one point of the varying-coefficient design (vc_point), degree >= 1 ---------------------------------------------------------
// One k_vc_expand launch per k_col_dots batch of expanded columns [b0, b1), split into that batch's row chunks: the sums then
// are the ones cdh_col_wrms takes.  The launch expands whole base columns [jb0, jb1): a base column whose group of degree + 1
// expanded columns straddles two batches is expanded by both launches (the same values twice), and k_vc_reduce keeps each
// batch's own columns.  table: the sums of w v^2 of the launch, `chunks` per expanded column; with a left-out row those of
// w v y stand behind them, and `partials` is both.
struct VcBatch {
    int64_t b0, b1, jb0, jb1;
    int chunks;
    size_t table, partials;
};
constexpr int64_t vc_batches(int64_t p) { return sp_ceil(p, kSpColBatch); }
constexpr VcBatch vc_batch(int64_t p, int degree, int64_t nvec, int cus, bool loo, int64_t t) {   // t < vc_batches(p)
    const int64_t Q1 = degree + 1, b0 = t * kSpColBatch, b1 = sp_min(b0 + kSpColBatch, p);
    const int chunks = col_dots_plan(b1 - b0, nvec, cus, 1).chunks;
    const int64_t jb0 = b0 / Q1, jb1 = sp_ceil(b1, Q1);
    const size_t table = (size_t)(jb1 - jb0) * Q1 * chunks;
    return VcBatch{b0, b1, jb0, jb1, chunks, table, table * (loo ? 2 : 1)};
}
// what a point counts towards cdh_profile_end: k_vc_weights and one k_vc_expand per batch (degree 0 expands nothing: its scales
// are col_dots'); read p_base columns, write p_base degree, z, w
constexpr int64_t vc_point_launches(int64_t p, int degree) { return 1 + (degree == 0 ? 0 : vc_batches(p)); }
constexpr double vc_point_bytes(int64_t n, size_t esz, int64_t p) { return (double)n * (double)esz * ((double)p + 2.0); }
