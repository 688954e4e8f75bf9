// block_sum.hpp -- the workgroup's size and its sum in a fixed order (wave butterflies, the four waves in order): what
// kernels.hpp's kernels and the second translation unit (cox_efron.hip) share.  Moved here from kernels.hpp word for word.
#pragma once
#include <hip/hip_runtime.h>

namespace cdk {

constexpr int kBlock = 256;   // 4 waves

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Sum NV per-thread values over a kBlock-thread block; result valid in thread 0.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* lds /* [NV * 4] */) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = wave_sum(v[i]);
        if (lane == 0) lds[i * (kBlock / 64) + wid] = v[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; ++w) s += lds[i * (kBlock / 64) + w];
            v[i] = s;
        }
    }
}

}  // namespace cdk
