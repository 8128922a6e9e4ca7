// block_reduce.hpp -- every wave- and workgroup-wide reduction of the kernels
// (device only; psvi_internal.hpp includes it).
//
// Each of them adds in a fixed order: the xor butterfly of a wave, the waves'
// partials in wave order, or a pairwise tree over the threads.  None uses an
// atomic, so a result depends on its operands alone, never on timing: two runs
// give the same bits.  Three shapes, by what the caller holds:
//   wave_* / lanes_*   one value per lane, registers only
//   block_*            one value per thread, blockDim.x / 64 LDS slots: the
//                      butterfly per wave, then the waves in order
//   tree_*<NT>         one value per thread of an NT-thread workgroup, NT LDS
//                      slots per value: red[t] (+)= red[t + o], o = NT / 2 .. 1
// Every workgroup form starts with a barrier, so `red` may still be in use
// (by an earlier reduction's result, say) when a thread arrives.
#pragma once
#include <hip/hip_runtime.h>

namespace psvi {

constexpr int kWave = 64;

// The wave's index in its workgroup, in an SGPR: the compiler cannot prove
// threadIdx.x >> 6 wave-uniform, and treats loops and branches on it as
// divergent (exec-masked, with conservative s_waitcnt that drain every
// outstanding load at the branch).
__device__ __forceinline__ int wave_id() {
    return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}

// ------------------------------------------------------------------- a wave
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, kWave));
    return v;
}

template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// max / sum over the first W lanes of each aligned group of W (W = 2, 4:
// quad permutes; 16: DPP row rotations by 8, 4, 2, 1, every lane of the row
// active); the result is valid on those lanes
template <int W>
__device__ __forceinline__ float lanes_max(float v) {
    static_assert(W == 2 || W == 4 || W == 16, "2, 4 or 16 lanes");
    if constexpr (W == 16) {
        v = fmaxf(v, dppf<0x128>(v));
        v = fmaxf(v, dppf<0x124>(v));
        v = fmaxf(v, dppf<0x122>(v));
        return fmaxf(v, dppf<0x121>(v));
    } else {
        v = fmaxf(v, dppf<0xB1>(v));              // quad_perm [1, 0, 3, 2]: lane ^ 1
        if constexpr (W == 4) v = fmaxf(v, dppf<0x4E>(v));  // quad_perm [2, 3, 0, 1]: lane ^ 2
        return v;
    }
}
template <int W>
__device__ __forceinline__ float lanes_sum(float v) {
    static_assert(W == 2 || W == 4 || W == 16, "2, 4 or 16 lanes");
    if constexpr (W == 16) {
        v += dppf<0x128>(v);
        v += dppf<0x124>(v);
        v += dppf<0x122>(v);
        return v + dppf<0x121>(v);
    } else {
        v += dppf<0xB1>(v);
        if constexpr (W == 4) v += dppf<0x4E>(v);
        return v;
    }
}
__device__ __forceinline__ float row16_max(float v) { return lanes_max<16>(v); }
__device__ __forceinline__ float row16_sum(float v) { return lanes_sum<16>(v); }

// ------------------------------------------- a workgroup, in wave order
// `red` is >= blockDim.x / 64 slots of LDS.  All threads call.  The double
// sum valid in thread 0 takes the thread count as the trees do: its callers
// (the conjugate-gradient grid sums) then keep a four-term unrolled tail
// instead of a run-time loop over blockDim.x / 64.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = wave_id();
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    return t;  // valid in thread 0
}
template <int NT>
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = wave_id();
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < NT / 64; ++i) t += red[i];
    return t;  // valid in thread 0
}
// the same with the result in every thread
__device__ __forceinline__ double block_sum_all(double v, double* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = wave_id(), nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}
__device__ __forceinline__ double block_max_all(double v, double* red) {
    v = wave_max(v);
    const int lane = threadIdx.x & 63, wid = wave_id(), nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double t = -INFINITY;
    for (int i = 0; i < nw; ++i) t = fmax(t, red[i]);
    return t;
}

// ------------------------------------- a workgroup of NT threads, as a tree
// `red` is NT doubles of LDS per value; the result is in every thread (and in
// red[0] until the next call).  All NT threads call.
template <int NT>
__device__ __forceinline__ double tree_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}
template <int NT>
__device__ __forceinline__ double tree_max(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    return red[0];
}
// two sums through one walk of the tree, each its own tree (value k in
// red[k NT ..]); red[0] / red[NT] hold the results for every thread after the
// call
template <int NT>
__device__ __forceinline__ void tree_sum(const double (&v)[2], double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v[0];
    red[NT + tid] = v[1];
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (tid < o) {
            red[tid] += red[tid + o];
            red[NT + tid] += red[NT + tid + o];
        }
        __syncthreads();
    }
}

// the largest value and its first argument: (value, index) pairs in the same
// tree; red[0] / redi[0] hold the result for every thread after the call
template <int NT>
__device__ __forceinline__ void tree_argmax_first(double best, int besti, double* red, int* redi) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = best;
    redi[tid] = besti;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
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
