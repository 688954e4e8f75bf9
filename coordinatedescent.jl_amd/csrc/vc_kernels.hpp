// vc_kernels.hpp -- HIP kernels (gfx950 / CDNA4) of the varying-coefficient lasso: what locpolyl1 recomputes on the host
// for every grid point z0, regenerated on the device from the base design, z and z0.
//
// Reference loops these replace (paths relative to the reference's src/):
//   k_vc_weights   w .= evaluate.(Ref(kernel), z, Ref(z0))     varying_coefficient_lasso.jl:17-21, 63
//   k_vc_expand    _expand_X!(expandX, X, z, z0, degree)       :550-569, fused with
//                  _stdX!(stdX, w, expandX)                    utils.jl:140-151
//   k_vc_reduce    the per-column sums of the latter, in a fixed order
// and, for the leave-one-out loop of lvocv_locpolyl1 (varying_coefficient_lasso.jl:82-137):
//   k_vc_weights   with a left-out row: w[i] = zero(T)                                           :110-111
//   k_vc_expand    <.., LOO = true>: z0 = z[i] read here, and the screening scores' sums
//                  sum_i X_ij w_i y_i of _findLargestCorrelations(w, X, y, s)  utils.jl:108-124, in the same pass
//   (kernels.hpp: k_resid_moments<T, true> takes sum w, sum w r^2 of _getSigma(w, r)             utils.jl:167-175)
//   k_gather_row   wX[i, S] of the prediction                                                    :132
//
// The expanded design keeps base column j at column j (Q + 1); the Q columns after it are that column times powers of
// (z - z0).  One streaming pass: read p_base columns, write p_base Q, with z and w re-read per column from cache.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace cdk {

constexpr int kVcGaussian = 0, kVcEpanechnikov = 1;   // cdh_vc_kernel

// evaluate(k, x, y), restated literally (varying_coefficient_lasso.jl:17-21) -- these are not the textbook forms: the
// Gaussian divides the squared distance by h (not 2 h^2), and both are scaled by 1 / h.
__device__ __forceinline__ double vc_kernel_value(int kind, double h, double x, double y) {
    if (kind == kVcGaussian) {
        const double d = x - y;
        return exp(-(d * d) / h) / h;
    }
    const double u = (x - y) / h;
    return fabs(u) >= 1.0 ? 0.0 : 0.75 * (1.0 - u * u) / h;
}

// w_i = K(z_i, z0) for rows < n, evaluated in double and rounded once to T; the rows of the last vector beyond n are
// written as zeros (the pad of w stays zero).  With a left-out row (leave_out >= 0, a row < n) z0 is z[leave_out] as
// stored, and w[leave_out] = 0.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_vc_weights(const T* __restrict__ z, T* __restrict__ w, int64_t n,
                                                       int64_t nvec, int kind, double h, double z0, int64_t leave_out) {
    using V = typename VecOf<T>::V;
    constexpr int NV = VecOf<T>::N;
    const V* zv = reinterpret_cast<const V*>(z);
    V* wv = reinterpret_cast<V*>(w);
    if (leave_out >= 0) z0 = (double)z[leave_out];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < nvec; j += stride) {
        const V zz = zv[j];
        V ww;
#pragma unroll
        for (int e = 0; e < NV; ++e)
            ww[e] = (j * NV + e < n && j * NV + e != leave_out) ? (T)vc_kernel_value(kind, h, (double)zz[e], z0) : (T)0;
        wv[j] = ww;
    }
}

// Block (chunk, b) expands base column jb0 + b over one row chunk: v_0 = x, v_l = v_{l-1} * (z - z0) in T -- the
// reference's own recurrence (:558-565), not pow -- stored to columns (jb0 + b)(Q + 1) + l, l = 1 .. Q, and
//   partials[((b (Q + 1) + l) * nchunks + chunk] = sum over the chunk of w v_l^2,   l = 0 .. Q,
// accumulated in double.  The split into chunks, the order of a thread's rows and the sums over the block are those of
// k_col_dots, so the totals are the very sums k_col_dots takes of the columns written here.
// Column streams are non-temporal; z and w stay cacheable (every block of a chunk re-reads them).
// LOO (the leave-one-out point): z0 is z[row0] as stored, and from the w v_l the block already holds it also takes
//   partials[(gridDim.y (Q + 1) + b (Q + 1) + l) * nchunks + chunk] = sum over the chunk of w v_l y
// -- a second table behind the first, in the same layout -- with y read per chunk from cache as z and w are.  The first
// table and the columns written are those of LOO = false, sum for sum.
constexpr int kVcUnroll = 4;    // independent column loads per thread in flight

template <typename T, int Q, bool LOO = false>
__global__ __launch_bounds__(kBlock) void k_vc_expand(T* __restrict__ X, int64_t ld, int64_t nvec,
                                                      const T* __restrict__ z, const T* __restrict__ w, T z0,
                                                      int64_t jb0, double* __restrict__ partials,
                                                      const T* __restrict__ y = nullptr, int64_t row0 = -1) {
    using V = typename VecOf<T>::V;
    constexpr int NV = VecOf<T>::N;
    constexpr int NACC = LOO ? 2 * (Q + 1) : Q + 1;      // [0, Q]: sum w v^2; LOO: [Q + 1, 2 Q + 1]: sum w v y
    __shared__ double lds[NACC * (kBlock / 64)];
    const int64_t jb = jb0 + blockIdx.y;
    V* col = reinterpret_cast<V*>(X + jb * (Q + 1) * ld);
    const int64_t ldv = ld / NV;                   // ld is a multiple of 32 elements
    const V* zv = reinterpret_cast<const V*>(z);
    const V* wv = reinterpret_cast<const V*>(w);
    const V* yv = reinterpret_cast<const V*>(y);
    if constexpr (LOO) z0 = z[row0];
    double acc[NACC];
#pragma unroll
    for (int l = 0; l < NACC; ++l) acc[l] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t j0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; j0 < nvec; j0 += stride * kVcUnroll) {
        V xv[kVcUnroll], zz[kVcUnroll], ww[kVcUnroll], yy[kVcUnroll];
#pragma unroll
        for (int u = 0; u < kVcUnroll; ++u) {
            const int64_t j = j0 + u * stride;
            if (j < nvec) {
                xv[u] = ld_stream<true>(col + j);
                zz[u] = zv[j];
                ww[u] = wv[j];
                if constexpr (LOO) yy[u] = yv[j];
            }
        }
#pragma unroll
        for (int u = 0; u < kVcUnroll; ++u) {
            const int64_t j = j0 + u * stride;
            if (j < nvec) {
                V v = xv[u];
                V df;
#pragma unroll
                for (int e = 0; e < NV; ++e) df[e] = zz[u][e] - z0;
#pragma unroll
                for (int l = 0; l <= Q; ++l) {
                    if (l > 0) {
#pragma unroll
                        for (int e = 0; e < NV; ++e) v[e] = v[e] * df[e];
                        __builtin_nontemporal_store(v, col + (int64_t)l * ldv + j);
                    }
#pragma unroll
                    for (int e = 0; e < NV; ++e) {
                        const double wx = (double)ww[u][e] * (double)v[e];
                        acc[l] = fma(wx, (double)v[e], acc[l]);
                        if constexpr (LOO) acc[Q + 1 + l] = fma(wx, (double)yy[u][e], acc[Q + 1 + l]);
                    }
                }
            }
        }
    }
    block_sum<NACC>(acc, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l <= Q; ++l)
            partials[((int64_t)blockIdx.y * (Q + 1) + l) * gridDim.x + blockIdx.x] = acc[l];
        if constexpr (LOO) {
#pragma unroll
            for (int l = 0; l <= Q; ++l)
                partials[((int64_t)(gridDim.y + blockIdx.y) * (Q + 1) + l) * gridDim.x + blockIdx.x] = acc[Q + 1 + l];
        }
    }
}

// one wave per expanded column c0 + blockIdx.x of the launch: out[column] = sum over its chunks, lanes striding the run
// as k_col_dots_reduce does.  Columns outside [lo, hi) belong to another batch and are left alone.
__global__ __launch_bounds__(64) void k_vc_reduce(const double* __restrict__ partials, int nchunks, int64_t c0,
                                                  int64_t lo, int64_t hi, double* __restrict__ out) {
    const int64_t col = c0 + blockIdx.x;
    if (col < lo || col >= hi) return;
    const double* pr = partials + (int64_t)blockIdx.x * nchunks;
    double s = 0.0;
    for (int c = threadIdx.x; c < nchunks; c += 64) s += pr[c];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[col] = s;
}

// out[k] = X[row, cols[k]] as doubles, k < m (cols 0-based): the row of the design a prediction reads.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_gather_row(const T* __restrict__ X, int64_t ld, int64_t row,
                                                       const int64_t* __restrict__ cols, int m, double* __restrict__ out) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k < m) out[k] = (double)X[cols[k] * ld + row];
}

}  // namespace cdk
