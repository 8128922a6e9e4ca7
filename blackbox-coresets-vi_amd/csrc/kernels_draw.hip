// kernels_draw.hip -- psvi_coreset_draw: coreset rows drawn in proportion to
// their weights f(v), with (prune: Efraimidis-Spirakis keys, sorted in LDS) or
// without (increment: inverse CDF by binary search) removal, on the library's
// Philox4x32-10 stream, and the gather of the drawn rows / targets.
//
// Everything that decides an index is fp64 from exact uniforms
// U = (word + 0.5) 2^-32; the semantics are stated in include/psvi_hip.h.
#include <limits.h>

#include "psvi_internal.hpp"

namespace psvi {

namespace {

constexpr int kDrawThreads = 256;
constexpr int kSortThreads = 1024;
constexpr int kGatherThreads = 256;

// a weight the draw refuses: negative, NaN or infinite
__device__ __forceinline__ bool bad_weight(float w) { return !(w >= 0.f) || isinf(w); }

// REPLACE.  Every workgroup forms the same fp64 prefix C of w in LDS (each
// thread sums a run of consecutive weights in index order, thread 0 the run
// totals in run order; C_i = runs before + within the run: a fixed association,
// equal in every workgroup and every launch), then walks its quads of draws:
// t = U C_{M-1}, the smallest i with C_i > t, clamped to the last positive
// weight.  A zero weight repeats its predecessor's prefix value bit for bit,
// so it is never the smallest such i.
__global__ __launch_bounds__(kDrawThreads) void draw_replace_kernel(CoresetDraw r, bool vec) {
    __shared__ double sC[kDrawMaxM];
    __shared__ double sRun[kDrawThreads];
    __shared__ int sLast;
    const int tid = threadIdx.x, M = r.M;
    if (tid == 0) sLast = -1;
    __syncthreads();
    int bad = 0, last = -1;
    for (int i = tid; i < M; i += kDrawThreads) {
        const float w = r.w[i];
        bad |= bad_weight(w);
        if (w > 0.f) last = i;
        sC[i] = (double)w;
    }
    if (last >= 0) atomicMax(&sLast, last);
    bad = __syncthreads_or(bad);
    const int status = bad ? 1 : (sLast < 0 ? 2 : 0);
    if (blockIdx.x == 0 && tid == 0) r.status_out[0] = status;
    if (status == 0) {
        const int K = (M + kDrawThreads - 1) / kDrawThreads;
        const int lo = min(tid * K, M), hi = min(lo + K, M);
        double run = 0.0;
        for (int i = lo; i < hi; ++i) {
            run += sC[i];
            sC[i] = run;
        }
        sRun[tid] = run;
        __syncthreads();
        if (tid == 0) {
            double before = 0.0;
            for (int t = 0; t < kDrawThreads; ++t) {
                const double tot = sRun[t];
                sRun[t] = before;
                before += tot;
            }
        }
        __syncthreads();
        const double before = sRun[tid];
        for (int i = lo; i < hi; ++i) sC[i] = before + sC[i];
        __syncthreads();
    }
    const double total = status == 0 ? sC[M - 1] : 0.0;
    const int lastpos = sLast;
    const int64_t n = r.n, nq = (n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * kDrawThreads + tid; q < nq;
         q += (int64_t)gridDim.x * kDrawThreads) {
        int out[4] = {-1, -1, -1, -1};
        if (status == 0) {
            uint32_t c[4];
            draw_words(r.seed, r.offset, q, c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double t = draw_uniform(c[j]) * total;
                int a = 0, b = M;  // the answer lies in [a, b]; b == M: no C_i > t
                while (a < b) {
                    const int mid = (a + b) >> 1;
                    if (sC[mid] > t) b = mid; else a = mid + 1;
                }
                out[j] = min(a, lastpos);
            }
        }
        const int64_t base = q * 4;
        if (vec && base + 3 < n) {
            *reinterpret_cast<int4*>(r.idx_out + base) = make_int4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (base + j < n) r.idx_out[base + j] = out[j];
        }
    }
}

// a sorts before b: the larger key, equal keys by the lower index
__device__ __forceinline__ bool draw_before(double ka, int ia, double kb, int ib) {
    return ka > kb || (ka == kb && ia < ib);
}

// NOREPLACE.  One workgroup: key_i = log(U_i) / w_i (-inf for w_i == 0), a
// bitonic sort of (key, index) over the next power of two P >= M in LDS --
// the padding sorts behind every row (key -inf, index >= M) -- and the first
// n indices out.  The order is total (indices differ), so the network's
// result does not depend on its shape.
__global__ __launch_bounds__(kSortThreads) void draw_noreplace_kernel(CoresetDraw r, int P) {
    __shared__ double sKey[kDrawMaxM];
    __shared__ int sIdx[kDrawMaxM];
    __shared__ int sPos;
    const int tid = threadIdx.x, M = r.M;
    if (tid == 0) sPos = 0;
    __syncthreads();
    int bad = 0, pos = 0;
    for (int i = tid; i < P; i += kSortThreads) {
        double key = -INFINITY;
        if (i < M) {
            const float w = r.w[i];
            bad |= bad_weight(w);
            if (w > 0.f) {
                uint32_t c[4];
                draw_words(r.seed, r.offset, i >> 2, c);
                const int e = i & 3;
                const uint32_t word = e == 0 ? c[0] : e == 1 ? c[1] : e == 2 ? c[2] : c[3];
                key = log(draw_uniform(word)) / (double)w;
                ++pos;
            }
        }
        sKey[i] = key;
        sIdx[i] = i;
    }
    if (pos) atomicAdd(&sPos, pos);
    bad = __syncthreads_or(bad);
    const int npos = sPos;
    const int status = bad ? 1 : (npos == 0 ? 2 : (npos < r.n ? 3 : 0));
    if (tid == 0) r.status_out[0] = status;
    if (status == 0) {
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += kSortThreads) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                    const double ki = sKey[i], kl = sKey[l];
                    const int ii = sIdx[i], il = sIdx[l];
                    const bool up = (i & k) == 0;
                    if (up ? draw_before(kl, il, ki, ii) : draw_before(ki, ii, kl, il)) {
                        sKey[i] = kl; sIdx[i] = il;
                        sKey[l] = ki; sIdx[l] = ii;
                    }
                }
                __syncthreads();
            }
        }
    }
    for (int j = tid; j < (int)r.n; j += kSortThreads) r.idx_out[j] = status == 0 ? sIdx[j] : -1;
}

// rows_out[j] <- rows[idx[j]] (one wave per output row) and targets_out[j] <-
// targets[idx[j]] (one thread per slot), as bits.  A draw that failed left
// every index at -1: nothing is written.
template <bool VEC>
__global__ __launch_bounds__(kGatherThreads) void draw_gather_kernel(CoresetDraw r) {
    const int64_t n = r.n;
    const int M = r.M;
    if (r.targets) {
        const uint32_t* __restrict__ src = static_cast<const uint32_t*>(r.targets);
        uint32_t* __restrict__ dst = static_cast<uint32_t*>(r.targets_out);
        for (int64_t j = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x; j < n;
             j += (int64_t)gridDim.x * kGatherThreads) {
            const int i = r.idx_out[j];
            if (i >= 0 && i < M) dst[j] = src[i];
        }
    }
    if (!r.rows || r.D == 0) return;
    constexpr int kWaves = kGatherThreads / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t D = r.D;
    for (int64_t j = (int64_t)blockIdx.x * kWaves + wave_id(); j < n;
         j += (int64_t)gridDim.x * kWaves) {
        const int i = __builtin_amdgcn_readfirstlane(r.idx_out[j]);
        if (i < 0 || i >= M) continue;
        const float* __restrict__ src = r.rows + (int64_t)i * D;
        float* __restrict__ dst = r.rows_out + j * D;
        if (VEC) {
            const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
            float4* __restrict__ d4 = reinterpret_cast<float4*>(dst);
            for (int64_t c = lane; c < D / 4; c += kWave) d4[c] = s4[c];
        } else {
            for (int64_t c = lane; c < D; c += kWave) dst[c] = src[c];
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

hipError_t launch_coreset_draw(const CoresetDraw& r, hipStream_t st) {
    if (!r.w || !r.idx_out || !r.status_out || r.M < 1 || r.M > kDrawMaxM || r.n < 1 ||
        r.D < 0 || (r.rows && !r.rows_out) || (r.targets && !r.targets_out))
        return hipErrorInvalidValue;
    if (r.replace) {
        const int64_t nq = (r.n + 3) / 4;
        const int blocks = (int)std::min<int64_t>((nq + kDrawThreads - 1) / kDrawThreads, 512);
        hipLaunchKernelGGL(draw_replace_kernel, dim3(blocks), dim3(kDrawThreads), 0, st, r,
                           aligned16(r.idx_out));
    } else {
        if (r.n > r.M) return hipErrorInvalidValue;
        int P = 1;
        while (P < r.M) P <<= 1;
        hipLaunchKernelGGL(draw_noreplace_kernel, dim3(1), dim3(kSortThreads), 0, st, r, P);
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (!r.targets && (!r.rows || r.D == 0)) return hipSuccess;
    constexpr int kWaves = kGatherThreads / kWave;
    const int blocks = (int)std::min<int64_t>((r.n + kWaves - 1) / kWaves, 4096);
    const bool vec = r.rows && r.D % 4 == 0 && aligned16(r.rows) && aligned16(r.rows_out);
    if (vec)
        hipLaunchKernelGGL(draw_gather_kernel<true>, dim3(blocks), dim3(kGatherThreads), 0, st, r);
    else
        hipLaunchKernelGGL(draw_gather_kernel<false>, dim3(blocks), dim3(kGatherThreads), 0, st, r);
    return hipGetLastError();
}

}  // namespace psvi
