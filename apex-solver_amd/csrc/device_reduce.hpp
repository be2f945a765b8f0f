// device_reduce.hpp -- the fp64 sum reductions every kernel file shares: one fixed tree per wave and per 256-thread block,
// so a sum reduced in two kernels rounds the same way.  Device-only; include after <hip/hip_runtime.h>.
#pragma once
#include <hip/hip_runtime.h>

namespace apex {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // valid in lane 0
}

// sum over the 256 threads of a block; result valid in thread 0.  `scratch` holds 4 doubles.
__device__ __forceinline__ double block_sum_256(double v, double* scratch) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) scratch[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) r = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
    __syncthreads();
    return r;
}

}  // namespace apex
