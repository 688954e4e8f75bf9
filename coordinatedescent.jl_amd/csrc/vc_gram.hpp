// vc_gram.hpp -- HIP kernels (gfx950 / CDNA4) of cdh_vc_gram: the weighted Gram matrix and right-hand side of the expanded
// varying-coefficient design, taken straight from the base design, z and y -- a read-only query of the handle.
//
// Reference loops these replace (paths relative to the reference's src/):
//   k_vc_moments   _expand_Xt_w_X!(Xt_w_X, w, X, z, z0, degree)     varying_coefficient_lasso.jl:572-620
//                  _expand_Xt_w_Y!(Xt_w_Y, w, X, z, y, z0, degree)  :622-647
//                  with w .= evaluate.(kernel, z, z0) (:272, :303), w .* w (:275), w * w * eps^2 (:306) and the left-out row of
//                  the commented-out lvocv_locpoly (:432-436) formed on the way, never stored
// The (mb (Q + 1))^2 entries of the Gram matrix are the 2Q + 1 moment matrices M_s = sum_i w_i d_i^s x_i x_i' (d_i = z_i - z0),
// its right-hand side the Q + 1 vectors m_a = sum_i w_i d_i^a y_i x_i; the kernel takes those and the host scatters them
// (vc_gram_types.hpp).
//
// How the work is split, and why.  A workgroup takes chunks of kVgRows = 64 rows, round robin.  Per chunk it stages the mb
// listed columns, converted to double, row-major in LDS, with two more columns behind them: y (zeros without it) and ones, so
// that m_a = M_a[., y] and sum w = M_0[1, 1] fall out of the one loop (the moments with the ones column and the orders above Q
// of the y column are computed and dropped: a few percent of the arithmetic for one code path).  The first wave evaluates the
// row's weight and leaves w_i d_i^s, s = 0 .. 2Q, next to it.  A thread then owns a 4 x 4 tile of every M_s in registers
// (16 (2Q + 1) doubles: 224 VGPRs at Q = 3, no scratch) and walks the chunk's rows: two 32-byte LDS reads of x, the row's
// w d^s broadcast, 16 products x_ij x_ik and 16 (2Q + 1) fmas.  Only tile pairs on or above the diagonal are given out (153 of
// them at mb = 64); with fewer columns the idle threads become further slices of the same pairs, each taking every S-th row
// of the chunk, and the slices are summed through LDS in slice order at the end.  Rows whose weight is exactly zero (the
// Epanechnikov kernel outside its support, the left-out row, the rows past n) are skipped: all their terms are zeros.
// The accumulators are plain fp64 FMAs, not fp64 MFMA as in k_gramstep: at mb <= 16 -- the low-dimensional use this is for --
// the pass is bound by the column stream either way, and an MFMA tile would have to carry the 2Q + 1 weightings as 2Q + 1
// scaled copies of an operand.  At mb = 64 the kernel is bound by fp64 arithmetic.
// Staging writes LDS with an 8-way bank conflict (row stride 68 doubles); the tile reads, which dominate, are conflict-free.
//
// Sums.  Everything is taken in double: d_i = z_i - z0 is formed in T, as k_vc_expand forms it, and widened; the kernel value
// is evaluated in double and rounded once to T (vc_kernel_value, as k_vc_weights); w_i = K_i^wpow e_i, its products with the
// powers of d_i, the products x_ij x_ik and all sums are double.  No atomics: every workgroup writes one block-major record
// (vc_gram_types.hpp: VcGramRec) and k_vc_moments_reduce sums the records in block order, four interleaved running sums per
// entry, so results are bit-identical run to run.
// L = ceil(nchunks / G) * ceil(kVgRows / S) + S + ceil(G / 4) + 2
// is the longest chain of sequential additions any output entry goes through (G workgroups, S slices, nchunks chunks of
// kVgRows rows: vc_gram_chain): a thread's rows, the S slices, the reduce kernel's G / 4 records and its last two additions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vc_gram_types.hpp"
#include "vc_kernels.hpp"

namespace cdk {

constexpr int kVgLd = 68;     // LDS row stride in doubles: 64 columns, y, ones, padded to whole tiles of 4 (and to 16 bytes)
constexpr int kVgWs = 8;      // doubles per row of the weight table: w d^s, s = 0 .. 6, padded
static_assert(vc_gram_groups(kVgMaxCols) * kVgTile <= kVgLd && 2 * kVgMaxDegree + 1 <= kVgWs, "");
static_assert(kVgTile * kVgTile * kVgThreads <= kVgRows * kVgLd, "the slices' sums of one order fit the staging area");

template <typename T, int Q>
__global__ __launch_bounds__(kVgThreads) void k_vc_moments(const T* __restrict__ X, int64_t ld, int64_t n,
                                                           const T* __restrict__ z, const T* __restrict__ y,
                                                           const T* __restrict__ e, const int64_t* __restrict__ cols,
                                                           int mb, int kind, double h, double z0, int wpow, int64_t leave_out,
                                                           double* __restrict__ partials) {
    constexpr int NS = 2 * Q + 1, TL = kVgTile;
    __shared__ __attribute__((aligned(16))) double xs[kVgRows * kVgLd];
    __shared__ __attribute__((aligned(16))) double ws[kVgRows * kVgWs];
    __shared__ int64_t scol[kVgMaxCols];
    const int tid = threadIdx.x;
    const int NB = vc_gram_groups(mb), NP = vc_gram_pairs(mb), S = vc_gram_slices(mb);
    const int slice = tid / NP, pair = tid - slice * NP;
    int bj = 0, bk = 0;                         // the pair's column groups, bj <= bk
    for (int t = pair; bj < NB; ++bj) {
        if (t < NB - bj) { bk = bj + t; break; }
        t -= NB - bj;
    }
    const T z0T = leave_out >= 0 ? z[leave_out] : (T)z0;
    const double z0d = leave_out >= 0 ? (double)z0T : z0;
    if (tid < mb) scol[tid] = cols[tid];

    double acc[TL][TL][NS];
#pragma unroll
    for (int u = 0; u < TL; ++u)
#pragma unroll
        for (int v = 0; v < TL; ++v)
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[u][v][s] = 0.0;

    const int64_t nchunks = vc_gram_chunks(n);
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t r0 = chunk * kVgRows;
        __syncthreads();                        // the previous chunk has been read (and scol written)
        if (tid < kVgRows) {
            const int64_t row = r0 + tid;
            double w = 0.0, d = 0.0, yy = 0.0;
            if (row < n) {                      // rows are bounded by n: no pad is trusted
                const T zi = z[row];
                d = (double)(T)(zi - z0T);
                if (row != leave_out) {
                    const double K = (double)(T)vc_kernel_value(kind, h, (double)zi, z0d);
                    w = wpow == 2 ? K * K : K;
                    if (e) w *= (double)e[row];
                }
                if (y) yy = (double)y[row];
            }
            double v = w;
#pragma unroll
            for (int s = 0; s < kVgWs; ++s) {
                ws[tid * kVgWs + s] = s < NS ? v : 0.0;
                v *= d;
            }
            xs[tid * kVgLd + mb] = yy;
            xs[tid * kVgLd + mb + 1] = 1.0;
            for (int c = mb + 2; c < NB * TL; ++c) xs[tid * kVgLd + c] = 0.0;
        }
        {
            const int i = tid & 63;
            const int64_t row = r0 + i;
            for (int c = tid >> 6; c < mb; c += kVgThreads / 64)
                xs[i * kVgLd + c] = row < n ? (double)X[scol[c] * ld + row] : 0.0;
        }
        __syncthreads();
        if (slice < S) {
            for (int i = slice; i < kVgRows; i += S) {
                double wv[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) wv[s] = ws[i * kVgWs + s];
                if (wv[0] == 0.0) continue;
                double xj[TL], xk[TL];
#pragma unroll
                for (int u = 0; u < TL; ++u) {
                    xj[u] = xs[i * kVgLd + bj * TL + u];
                    xk[u] = xs[i * kVgLd + bk * TL + u];
                }
#pragma unroll
                for (int u = 0; u < TL; ++u)
#pragma unroll
                    for (int v = 0; v < TL; ++v) {
                        const double t = xj[u] * xk[v];
#pragma unroll
                        for (int s = 0; s < NS; ++s) acc[u][v][s] = fma(t, wv[s], acc[u][v][s]);
                    }
            }
        }
    }

    if (S > 1) {                                // the slices of a pair, summed in slice order: one order s at a time through xs
        double* red = xs;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            __syncthreads();
#pragma unroll
            for (int u = 0; u < TL; ++u)
#pragma unroll
                for (int v = 0; v < TL; ++v) red[(u * TL + v) * kVgThreads + tid] = acc[u][v][s];
            __syncthreads();
            if (slice == 0) {
#pragma unroll
                for (int u = 0; u < TL; ++u)
#pragma unroll
                    for (int v = 0; v < TL; ++v) {
                        double sum = 0.0;
                        for (int q = 0; q < S; ++q) sum += red[(u * TL + v) * kVgThreads + q * NP + pair];
                        acc[u][v][s] = sum;
                    }
            }
        }
    }
    if (slice != 0) return;
    const VcGramRec R = vc_gram_rec(Q, mb);
    double* rec = partials + (int64_t)blockIdx.x * R.n;
#pragma unroll
    for (int u = 0; u < TL; ++u)
#pragma unroll
        for (int v = 0; v < TL; ++v) {
            const int j = bj * TL + u, k = bk * TL + v;
            if (j > k) continue;
            if (k < mb) {
#pragma unroll
                for (int s = 0; s < NS; ++s) rec[s * R.tri + vc_gram_tri(mb, j, k)] = acc[u][v][s];
            } else if (k == mb && j < mb) {
#pragma unroll
                for (int a = 0; a <= Q; ++a) rec[R.off_m + a * mb + j] = acc[u][v][a];
            } else if (j == mb + 1 && k == mb + 1) {
                rec[R.off_w] = acc[u][v][0];
            }
        }
}

// out[v] = sum over the G records of entry v, in block order: four interleaved running sums, then (s0 + s1) + (s2 + s3)
__global__ __launch_bounds__(kVgThreads) void k_vc_moments_reduce(const double* __restrict__ partials, int G, int64_t nrec,
                                                                  double* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * kVgThreads + threadIdx.x;
    if (v >= nrec) return;
    const double* p = partials + v;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int b = 0;
    for (; b + 3 < G; b += 4) {
        s0 += p[(int64_t)b * nrec];
        s1 += p[(int64_t)(b + 1) * nrec];
        s2 += p[(int64_t)(b + 2) * nrec];
        s3 += p[(int64_t)(b + 3) * nrec];
    }
    if (b < G) s0 += p[(int64_t)b * nrec];
    if (b + 1 < G) s1 += p[(int64_t)(b + 1) * nrec];
    if (b + 2 < G) s2 += p[(int64_t)(b + 2) * nrec];
    out[v] = (s0 + s1) + (s2 + s3);
}

}  // namespace cdk
