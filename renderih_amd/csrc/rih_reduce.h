// rih_reduce.h -- the full-wavefront (64-lane) and 256-thread reductions shared by the kernels.  Every order is fixed: an
// xor butterfly over the lanes 32, 16, ... 1 (the result is valid in every lane), then for block_sum one word per wavefront
// in LDS and the tree (r0 + r1) + (r2 + r3).  Kernels whose results are pinned bitwise rest on these orders: do not change
// them.  Narrower butterflies (row_sum / row_max of rih_attn, group_sum<LPR> of rih_elem) are other functions and stay with
// their kernels.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// sum over the 256 threads of the block (red: 4 floats of LDS); the result is valid in every thread
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
