// select_reduce.hpp -- the block-wide fixed-tree reductions of the one-workgroup
// selection kernels (kernels_select.hip, kernels_laplace.hip): kSelThreads
// values meet in a fixed tree, so a result does not depend on timing.
#pragma once
#include <hip/hip_runtime.h>

namespace psvi {

constexpr int kSelMaxS = 2048;
constexpr int kSelThreads = 512;

// block-wide fixed-tree reductions over kSelThreads values; result in every thread
__device__ __forceinline__ double sel_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = kSelThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}
__device__ __forceinline__ double sel_max(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = kSelThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    return red[0];
}

// the largest value and its first argument: (value, index) pairs in a fixed
// tree; red[0] / redi[0] hold the result for every thread after the call
__device__ __forceinline__ void sel_argmax_first(double best, int besti, double* red, int* redi) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = best;
    redi[tid] = besti;
    __syncthreads();
    for (int o = kSelThreads / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const double v = red[tid + o];
            const int i = redi[tid + o];
            if (v > red[tid] || (v == red[tid] && i < redi[tid])) {
                red[tid] = v;
                redi[tid] = i;
            }
        }
        __syncthreads();
    }
}

}  // namespace psvi
