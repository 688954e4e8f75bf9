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
//
// A batch of points per launch (cdh_vc_gram_batch, vc_gram_batch_types.hpp).  k_vc_moments takes a list of points, so it also
// serves the loops that call the above once per point -- locpoly on a grid (varying_coefficient_lasso.jl:217-235),
// lvocv_locpoly (:348-380), split_locpoly (:383-409), each over _expand_Xt_w_X! / _expand_Xt_w_Y! (:572-647) -- with the
// points' (z0, h, left-out row) read from a device array and the partial records laid out [point][workgroup][entry].  In
// either regime every entry of a point goes through the additions above in their order: the same deal of chunks to
// workgroups, the same slices, the same slice-order sum, and k_vc_moments_reduce per point -- so a point's result is
// bit-identical wherever it stands in a batch.  Two regimes, one launch per group of points either way:
//   streamed  <.., false>: workgroups walk several chunks; grid.y = the points, and a (workgroup, point) is
//             vg_point_over_chunks.  The base columns are re-read per point, out of L2 / Infinity Cache for the designs this is
//             for.  A single-point call (cdh_vc_gram) is this instantiation on a grid (G, 1), whatever n is.
//   resident  <.., true>: every workgroup of the single-point deal holds ONE chunk (vc_gram_chunks(n) <= vc_gram_grid(n, Q, mb):
//             n <= 32768 rows, fewer where the partial buffer caps the grid).  grid.x = the chunks, grid.y = shares of the point
//             list.  A workgroup stages its 64 rows of the listed columns, y and the ones once, keeps z and e of its rows in
//             the first wave's registers, and walks its share: per point the first wave writes the weight table w d^s, all
//             threads run the tile accumulation from zero, the slices are summed through an LDS area of their own (the staged
//             rows stay), and one record is written.  Global memory is read once per workgroup, not once per point.  The
//             weight table is double-buffered, so a point costs one barrier plus the 2 (2Q + 1) of the slice sum where S > 1.
//             LDS: 34 KiB rows + 8 KiB tables + 32 KiB slice sums = 74.5 KiB, two workgroups per CU at most.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch in any instantiation; fp32 within 3 registers of fp64):
//                          Q = 0        Q = 1        Q = 2              Q = 3               LDS
//   streamed               100 VGPRs    168          240                256 + 41 AGPRs      38.5 KiB
//   resident               147          213          255 + 28 AGPRs     256 + 90 AGPRs      74.5 KiB
// (the accumulators alone are 32 (2Q + 1) VGPRs: 224 at Q = 3.)  Waves per SIMD: 4, 3, 2, 1 streamed; 2, 2, 1, 1 resident --
// at Q >= 2 the resident kernel's registers, not its LDS, hold a CU to one workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vc_gram_batch_types.hpp"
#include "vc_gram_types.hpp"
#include "vc_kernels.hpp"

namespace cdk {

constexpr int kVgLd = 68;     // LDS row stride in doubles: 64 columns, y, ones, padded to whole tiles of 4 (and to 16 bytes)
constexpr int kVgWs = 8;      // doubles per row of the weight table: w d^s, s = 0 .. 6, padded
static_assert(vc_gram_groups(kVgMaxCols) * kVgTile <= kVgLd && 2 * kVgMaxDegree + 1 <= kVgWs, "");
static_assert(kVgTile * kVgTile * kVgThreads <= kVgRows * kVgLd, "the slices' sums of one order fit the staging area");

// ---- the pieces of k_vc_moments -------------------------------------------------------------------------------------------
// what a thread works on: slice `slice` of the pair (bj, bk) of column groups, bj <= bk
struct VgThread {
    int NB, NP, S, slice, pair, bj, bk;
};
__device__ __forceinline__ VgThread vg_thread(int tid, int mb) {
    VgThread t;
    t.NB = vc_gram_groups(mb), t.NP = vc_gram_pairs(mb), t.S = vc_gram_slices(mb);
    t.slice = tid / t.NP, t.pair = tid - t.slice * t.NP;
    t.bj = 0, t.bk = 0;
    for (int r = t.pair; t.bj < t.NB; ++t.bj) {
        if (r < t.NB - t.bj) { t.bk = t.bj + r; break; }
        r -= t.NB - t.bj;
    }
    return t;
}

// one row of the weight table: w d^s, s = 0 .. 2Q.  live: the row is below n (rows are bounded by n: no pad is trusted)
template <typename T, int NS>
__device__ __forceinline__ void vg_weight_row(double* __restrict__ wrow, bool live, bool left_out, T zi, bool has_e, double ei,
                                              int kind, double h, T z0T, double z0d, int wpow) {
    double w = 0.0, d = 0.0;
    if (live) {
        d = (double)(T)(zi - z0T);
        if (!left_out) {
            const double K = (double)(T)vc_kernel_value(kind, h, (double)zi, z0d);
            w = wpow == 2 ? K * K : K;
            if (has_e) w *= ei;
        }
    }
    double v = w;
#pragma unroll
    for (int s = 0; s < kVgWs; ++s) {
        wrow[s] = s < NS ? v : 0.0;
        v *= d;
    }
}

// the chunk's rows r0 .. r0 + 63 of the listed columns, y and the ones, as doubles, row-major in xs
template <typename T>
__device__ __forceinline__ void vg_stage_chunk(double* __restrict__ xs, const T* __restrict__ X, int64_t ld, int64_t n,
                                               const T* __restrict__ y, const int64_t* scol, int mb, int NB, int64_t r0, int tid) {
    if (tid < kVgRows) {
        const int64_t row = r0 + tid;
        xs[tid * kVgLd + mb] = (y && row < n) ? (double)y[row] : 0.0;
        xs[tid * kVgLd + mb + 1] = 1.0;
        for (int c = mb + 2; c < NB * kVgTile; ++c) xs[tid * kVgLd + c] = 0.0;
    }
    const int i = tid & 63;
    const int64_t row = r0 + i;
    for (int c = tid >> 6; c < mb; c += kVgThreads / 64) xs[i * kVgLd + c] = row < n ? (double)X[scol[c] * ld + row] : 0.0;
}

// the thread's rows of the staged chunk into its tile of every M_s
template <int Q>
__device__ __forceinline__ void vg_tiles(double (&acc)[kVgTile][kVgTile][2 * Q + 1], const double* __restrict__ xs,
                                         const double* __restrict__ ws, const VgThread& t) {
    constexpr int NS = 2 * Q + 1, TL = kVgTile;
    if (t.slice >= t.S) return;
    for (int i = t.slice; i < kVgRows; i += t.S) {
        double wv[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) wv[s] = ws[i * kVgWs + s];
        if (wv[0] == 0.0) continue;
        double xj[TL], xk[TL];
#pragma unroll
        for (int u = 0; u < TL; ++u) {
            xj[u] = xs[i * kVgLd + t.bj * TL + u];
            xk[u] = xs[i * kVgLd + t.bk * TL + u];
        }
#pragma unroll
        for (int u = 0; u < TL; ++u)
#pragma unroll
            for (int v = 0; v < TL; ++v) {
                const double xx = xj[u] * xk[v];
#pragma unroll
                for (int s = 0; s < NS; ++s) acc[u][v][s] = fma(xx, wv[s], acc[u][v][s]);
            }
    }
}

// the slices of a pair, summed in slice order into slice 0: one order s at a time through red (16 x kVgThreads doubles).
// Every thread of the workgroup comes here (S > 1 is uniform); starts with a barrier, so red may be an area just read.
template <int Q>
__device__ __forceinline__ void vg_slice_sum(double (&acc)[kVgTile][kVgTile][2 * Q + 1], double* __restrict__ red, int tid,
                                             const VgThread& t) {
    constexpr int NS = 2 * Q + 1, TL = kVgTile;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < TL; ++u)
#pragma unroll
            for (int v = 0; v < TL; ++v) red[(u * TL + v) * kVgThreads + tid] = acc[u][v][s];
        __syncthreads();
        if (t.slice == 0) {
#pragma unroll
            for (int u = 0; u < TL; ++u)
#pragma unroll
                for (int v = 0; v < TL; ++v) {
                    double sum = 0.0;
                    for (int q = 0; q < t.S; ++q) sum += red[(u * TL + v) * kVgThreads + q * t.NP + t.pair];
                    acc[u][v][s] = sum;
                }
        }
    }
}

// slice 0's tile into the workgroup's record
template <int Q>
__device__ __forceinline__ void vg_write_rec(const double (&acc)[kVgTile][kVgTile][2 * Q + 1], double* __restrict__ rec, int mb,
                                             const VgThread& t) {
    constexpr int NS = 2 * Q + 1, TL = kVgTile;
    const VcGramRec R = vc_gram_rec(Q, mb);
#pragma unroll
    for (int u = 0; u < TL; ++u)
#pragma unroll
        for (int v = 0; v < TL; ++v) {
            const int j = t.bj * TL + u, k = t.bk * TL + v;
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

// One point over the chunks blockIdx.x, blockIdx.x + gridDim.x, ..: the whole of a (workgroup, point) of the streamed regime.
// scol has been written by the caller (the first barrier below covers it).
template <typename T, int Q>
__device__ __forceinline__ void vg_point_over_chunks(const T* __restrict__ X, int64_t ld, int64_t n, const T* __restrict__ z,
                                                     const T* __restrict__ y, const T* __restrict__ e, const int64_t* scol, int mb,
                                                     int kind, double h, double z0, int wpow, int64_t leave_out,
                                                     double* __restrict__ rec, double* xs, double* ws) {
    constexpr int NS = 2 * Q + 1, TL = kVgTile;
    const int tid = threadIdx.x;
    const VgThread t = vg_thread(tid, mb);
    const T z0T = leave_out >= 0 ? z[leave_out] : (T)z0;
    const double z0d = leave_out >= 0 ? (double)z0T : z0;

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
            const bool live = row < n;
            vg_weight_row<T, NS>(ws + tid * kVgWs, live, row == leave_out, live ? z[row] : (T)0, e != nullptr,
                                 (e && live) ? (double)e[row] : 0.0, kind, h, z0T, z0d, wpow);
        }
        vg_stage_chunk<T>(xs, X, ld, n, y, scol, mb, t.NB, r0, tid);
        __syncthreads();
        vg_tiles<Q>(acc, xs, ws, t);
    }
    if (t.S > 1) vg_slice_sum<Q>(acc, xs, tid, t);
    if (t.slice == 0) vg_write_rec<Q>(acc, rec, mb, t);
}

// The points pts[0 .. npts) of one launch group; the record of (point, workgroup) at partials + (point gridDim.x + blockIdx.x) nrec.
// RES = false: grid (G, npts), `per` unused.  RES = true: grid (G, shares), G workgroups of one chunk each, share blockIdx.y walks
// points blockIdx.y per .. min(npts, (blockIdx.y + 1) per) - 1 (vc_gram_batch_types.hpp: vgb_share_points, vgb_share_begin).
template <typename T, int Q, bool RES>
__global__ __launch_bounds__(kVgThreads) void k_vc_moments(const T* __restrict__ X, int64_t ld, int64_t n,
                                                           const T* __restrict__ z, const T* __restrict__ y,
                                                           const T* __restrict__ e, const int64_t* __restrict__ cols,
                                                           int mb, int kind, int wpow,
                                                           const VcGramPoint* __restrict__ pts, int npts, int per,
                                                           double* __restrict__ partials) {
    constexpr int NS = 2 * Q + 1, TL = kVgTile;
    __shared__ __attribute__((aligned(16))) double xs[kVgRows * kVgLd];
    __shared__ __attribute__((aligned(16))) double ws[(RES ? 2 : 1) * kVgRows * kVgWs];
    __shared__ __attribute__((aligned(16))) double red[RES ? TL * TL * kVgThreads : 1];
    __shared__ int64_t scol[kVgMaxCols];
    const int tid = threadIdx.x;
    const int64_t nrec = vc_gram_rec(Q, mb).n;
    if (tid < mb) scol[tid] = cols[tid];
    if constexpr (!RES) {
        const VcGramPoint P = pts[blockIdx.y];
        vg_point_over_chunks<T, Q>(X, ld, n, z, y, e, scol, mb, kind, P.h, P.z0, wpow, P.leave_out,
                                   partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nrec, xs, ws);
    } else {
        const VgThread t = vg_thread(tid, mb);
        const int64_t r0 = (int64_t)blockIdx.x * kVgRows, row = r0 + tid;
        const bool live = tid < kVgRows && row < n;     // the first wave keeps z and e of the chunk's rows
        const T zi = live ? z[row] : (T)0;
        const double ei = (e && live) ? (double)e[row] : 0.0;
        __syncthreads();                                // scol
        vg_stage_chunk<T>(xs, X, ld, n, y, scol, mb, t.NB, r0, tid);
        const int p1 = min(npts, ((int)blockIdx.y + 1) * per);
        for (int p = (int)blockIdx.y * per; p < p1; ++p) {
            const VcGramPoint P = pts[p];
            const T z0T = P.leave_out >= 0 ? z[P.leave_out] : (T)P.z0;
            const double z0d = P.leave_out >= 0 ? (double)z0T : P.z0;
            double* wsp = ws + (p & 1) * (kVgRows * kVgWs);    // the other table may still be read by the previous point's tiles
            if (tid < kVgRows)
                vg_weight_row<T, NS>(wsp + tid * kVgWs, live, row == P.leave_out, zi, e != nullptr, ei, kind, P.h, z0T, z0d, wpow);
            __syncthreads();                            // this point's table (and, the first time round, the staged rows)
            double acc[TL][TL][NS];
#pragma unroll
            for (int u = 0; u < TL; ++u)
#pragma unroll
                for (int v = 0; v < TL; ++v)
#pragma unroll
                    for (int s = 0; s < NS; ++s) acc[u][v][s] = 0.0;
            vg_tiles<Q>(acc, xs, wsp, t);
            if (t.S > 1) vg_slice_sum<Q>(acc, red, tid, t);
            if (t.slice == 0) vg_write_rec<Q>(acc, partials + ((int64_t)p * gridDim.x + blockIdx.x) * nrec, mb, t);
        }
    }
}

// out[point][v] = sum over the G records of entry v of the point blockIdx.y, in block order: four interleaved running sums,
// then (s0 + s1) + (s2 + s3).  partials is [point][G][nrec]; a single-point call is the launch with gridDim.y = 1.
__global__ __launch_bounds__(kVgThreads) void k_vc_moments_reduce(const double* __restrict__ partials, int G, int64_t nrec,
                                                                  double* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * kVgThreads + threadIdx.x;
    if (v >= nrec) return;
    const double* p = partials + (int64_t)blockIdx.y * G * nrec + v;
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
    out[(int64_t)blockIdx.y * nrec + v] = (s0 + s1) + (s2 + s3);
}

}  // namespace cdk
