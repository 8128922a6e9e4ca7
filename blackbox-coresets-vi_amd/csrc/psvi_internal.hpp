// psvi_internal.hpp -- shared host/device definitions of libpsvi_hip.so.
// Written for gfx950 (CDNA4, wave64) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "block_reduce.hpp"
#include "psvi_hip.h"
#include "ws_carve.hpp"

namespace psvi {

constexpr int kMaxL = PSVI_MAX_LAYERS;
constexpr int kMaxWorld = 8;      // ranks per node (xGMI)

// ---------------------------------------------------------------- numerics
// a * b rounded on its own: never fused into an fma with the add that uses it
// (hipcc contracts a * b + c across statements and through __fmul_rn), for
// two kernels that must give the same bits from the same operands
__device__ __forceinline__ float mul_unfused(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// torch.nn.functional.softplus(beta=1, threshold=20)
__device__ __forceinline__ float softplus_f(float x) {
    return x > 20.f ? x : log1pf(expf(x));
}
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// ------------------------------------------------------- buffer loads (T8)
// 128-bit SRD in SGPRs + 32-bit per-lane byte offset; the hardware range
// check returns 0 for any offset >= `bytes`, which is how the kernels mask
// ragged / triangular tiles without exec-mask branches around the loads.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr uint32_t kOOB = 0x80000000u;  // byte offset past every buffer we map

__device__ __forceinline__ rsrc_t make_rsrc(const void* base, int64_t bytes) {
    const uint32_t nb = bytes > 0x7fffffff ? 0x7fffffffu : (uint32_t)bytes;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)nb,
                                             0x00020000);
}
// A 16-byte buffer store whose data registers stay untouched for the two wait
// states after it.  hipcc (ROCm 7.2) does not pad the VMEM-store data hazard
// for __builtin_amdgcn_raw_buffer_store_b128 (it does for global stores): a
// VALU write of a data VGPR in the next instruction can reach memory instead
// of the stored value -- seen as LDS-offset bit patterns in the streaming
// update's tiled Adam state.  The asm reads the data after the store, so no
// instruction in between may redefine those registers, and pads two states.
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
#define BSTORE128(v, r, voff, soff, aux)                                    \
    do {                                                                    \
        const u32x4_t bst_v_ = (v);                                         \
        __builtin_amdgcn_raw_buffer_store_b128(bst_v_, r, voff, soff, aux); \
        asm volatile("s_nop 1" ::"v"(bst_v_));                              \
    } while (0)
__device__ __forceinline__ float bload(rsrc_t r, uint32_t off) {
    // the builtin returns the raw 32 bits as an integer
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}

// ------------------------------------------------- Philox4x32-10 normals
// psvi_randn's stream: normal i of (seed, offset) is element i % 4 of
// Philox4x32-10(counter = offset / 4 + i / 4, key = seed) through Box-Muller.
// Shared by randn_kernel and the network kernel's fused next-step draw.
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
    const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
}

__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// the Philox output words 4q .. 4q+3 of the stream (seed, offset), and the
// uniform of a word: exact in fp64, strictly inside (0, 1) -- the stream of
// psvi_coreset_draw and of psvi_kmeans' seeding
__device__ __forceinline__ void draw_words(uint64_t seed, uint64_t offset, int64_t q,
                                           uint32_t (&c)[4]) {
    const uint64_t ctr = offset / 4 + (uint64_t)q;
    c[0] = (uint32_t)ctr;
    c[1] = (uint32_t)(ctr >> 32);
    c[2] = 0u;
    c[3] = 0u;
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}
__device__ __forceinline__ double draw_uniform(uint32_t word) {
    return ((double)word + 0.5) * 0x1p-32;
}

// normals 4q .. 4q+3 of the stream (Philox counter offset / 4 + q, Box-Muller)
__device__ __forceinline__ void randn_quad_vals(uint64_t seed, uint64_t offset, int64_t q,
                                                float (&r)[4]) {
    const uint64_t ctr = offset / 4 + (uint64_t)q;
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        // Box-Muller on the native transcendentals: u1 in (0, 1], u2 in [0, 1);
        // v_log_f32 is log2, v_sin/v_cos_f32 take revolutions (sin(2 pi u2))
        const float u1 = ((float)(c[2 * j] >> 8) + 1.0f) * (1.0f / 16777216.0f);
        const float u2 = (float)(c[2 * j + 1] >> 8) * (1.0f / 16777216.0f);
        const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));
        r[2 * j] = rad * __builtin_amdgcn_cosf(u2);
        r[2 * j + 1] = rad * __builtin_amdgcn_sinf(u2);
    }
}

// normals 4q .. 4q+3 of the stream into out[0, n)
template <bool VEC>
__device__ __forceinline__ void randn_quad(float* __restrict__ out, int64_t n, uint64_t seed,
                                           uint64_t offset, int64_t q) {
    float r[4];
    randn_quad_vals(seed, offset, q, r);
    const int64_t base = q * 4;
    if (VEC && base + 3 < n) {
        *reinterpret_cast<float4*>(out + base) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
        for (int j = 0; j < 4 && base + j < n; ++j) out[base + j] = r[j];
    }
}

// ------------------------------------------- bf16 planes of a full-cov draw
// fp32-faithful products on the bf16 matrix cores: x = x0 + x1 + x2, each
// piece bf16 (round to nearest even) and the sum exact for normal fp32 (the
// second residual has <= 8 significant bits); a product of two split operands
// is the six piece products down to 2^-27 relative, below fp32's rounding.
__device__ __forceinline__ uint16_t bf_bits(float x) {
    return __builtin_bit_cast(uint16_t, (__bf16)x);
}
__device__ __forceinline__ float bf_val(uint32_t b) { return __uint_as_float(b << 16); }
__device__ __forceinline__ void split3(float x, uint16_t& x0, uint16_t& x1, uint16_t& x2) {
    x0 = bf_bits(x);
    const float r1 = x - bf_val(x0);
    x1 = bf_bits(r1);
    x2 = bf_bits(r1 - bf_val(x1));
}

// A full-cov eps draw also as three bf16 planes (the streaming update's MFMA
// operands): plane p holds piece p of element (l, s, c) at poff[l] + s npad[l]
// + c, rows padded to npad[l] = a 64-multiple with zeros (the pads are never
// drawn).  eoff: the layers' [S][n] blocks in the fp32 draw order (eoff[L] =
// the draw's length).
struct EpsPlanes {
    int L;
    int64_t pl;  // elements per plane; planes back to back
    int64_t eoff[kMaxL + 1];
    int n[kMaxL], npad[kMaxL];
    int64_t poff[kMaxL];
};

// Element i's place in the planes for the layers of an EpsPlanes (selects over
// the layers: a dynamic index into P would put it in scratch).  The row
// division runs on 32 bits when the whole draw is below 2^31 elements.
struct EpsPlaneMap {
    const EpsPlanes& P;
    bool small;  // uniform: the draw's length < 2^31
    __device__ __forceinline__ int64_t operator()(int64_t i, int& c, int& nl) const {
        int64_t e0 = P.eoff[0], po = P.poff[0];
        int np = P.npad[0];
        nl = P.n[0];
#pragma unroll
        for (int k = 1; k < kMaxL; ++k)
            if (k < P.L && i >= P.eoff[k]) {
                e0 = P.eoff[k];
                po = P.poff[k];
                np = P.npad[k];
                nl = P.n[k];
            }
        const int64_t rem = i - e0;
        const int s = small ? (int)((uint32_t)rem / (uint32_t)nl) : (int)(rem / nl);
        c = (int)(rem - (int64_t)s * nl);
        return po + (int64_t)s * np + c;
    }
};

// normals 4q .. 4q+3 of the stream into out[0, n) and, with planes, their
// three bf16 pieces (randn_quad's values); place(i, c, nl): element i's offset
// in a plane, its column c and its row's length nl; pl: elements per plane
template <class Place>
__device__ __forceinline__ void randn_quad_planes_at(float* __restrict__ out, int64_t n, uint64_t seed,
                                                     uint64_t offset, int64_t q, const Place& place,
                                                     int64_t pl, uint16_t* __restrict__ planes) {
    float r[4];
    randn_quad_vals(seed, offset, q, r);
    const int64_t base = q * 4;
    if (base + 3 < n) {
        *reinterpret_cast<float4*>(out + base) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
        for (int j = 0; j < 4 && base + j < n; ++j) out[base + j] = r[j];
    }
    if (!planes) return;
    uint16_t pc[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split3(r[j], pc[0][j], pc[1][j], pc[2][j]);
    int c0, nl;
    const int64_t o = place(base, c0, nl);
    if (c0 + 3 < nl && base + 3 < n && (o & 3) == 0) {  // the quad in one row
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
            *reinterpret_cast<u16x4*>(planes + p * pl + o) = u16x4{pc[p][0], pc[p][1], pc[p][2], pc[p][3]};
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (base + j >= n) break;
        int cj, nj;
        const int64_t oj = place(base + j, cj, nj);
#pragma unroll
        for (int p = 0; p < 3; ++p) planes[p * pl + oj] = pc[p][j];
    }
}
__device__ __forceinline__ void randn_quad_planes(float* __restrict__ out, int64_t n, uint64_t seed,
                                                  uint64_t offset, int64_t q, const EpsPlanes& P,
                                                  uint16_t* __restrict__ planes) {
    randn_quad_planes_at(out, n, seed, offset, q, EpsPlaneMap{P, n < (int64_t(1) << 31)}, P.pl, planes);
}

// Adam, both reference variants; returns new p, updates m, v in place.
struct AdamC {
    float lr, b1, b2, eps, omb1, omb2;
    float inv_bc1, inv_sqrt_bc2;  // 1/(1-b1^t), 1/sqrt(1-b2^t)
    float lr_bc1;                 // lr/(1-b1^t)
    float inv_bc2;                // 1/(1-b2^t)
    int kind;
};

__device__ __forceinline__ float adam_apply(const AdamC& a, float p, float g, float& m,
                                            float& v) {
    m = a.b1 * m + a.omb1 * g;
    if (a.kind == PSVI_ADAM_HIGHER) {
        // optim.py:339-367: v stored without the 1e-8; denom = sqrt(v+1e-8)/sqrt(bc2)+eps
        v = a.b2 * v + a.omb2 * g * g;
        const float denom = sqrtf(v + 1e-8f) * a.inv_sqrt_bc2 + a.eps;
        return p - a.lr_bc1 * (m / denom);
    } else if (a.kind == PSVI_ADAM_TORCH) {
        // torch.optim.Adam (single-tensor path): denom = sqrt(v)/sqrt(bc2) + eps
        v = a.b2 * v + a.omb2 * g * g;
        const float denom = sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
        return p - a.lr_bc1 * (m / denom);
    } else {
        // diff_optimizers.py:197-213: v += 1e-12 stored; denom = sqrt(v/bc2)+eps
        v = a.b2 * v + a.omb2 * g * g + 1e-12f;
        const float denom = sqrtf(v * a.inv_bc2) + a.eps;
        return p - a.lr * ((m * a.inv_bc1) / denom);
    }
}

// Same update with the raw v_sqrt_f32 / v_rcp_f32 (1 ulp each) instead of the
// IEEE-exact expansions: the full-cov update runs it on 4.7 M entries per step.
__device__ __forceinline__ float adam_apply_fast(const AdamC& a, float p, float g, float& m,
                                                 float& v) {
    m = a.b1 * m + a.omb1 * g;
    if (a.kind == PSVI_ADAM_HIGHER) {
        v = a.b2 * v + a.omb2 * g * g;
        const float denom = __builtin_amdgcn_sqrtf(v + 1e-8f) * a.inv_sqrt_bc2 + a.eps;
        return p - a.lr_bc1 * m * __builtin_amdgcn_rcpf(denom);
    } else if (a.kind == PSVI_ADAM_TORCH) {
        v = a.b2 * v + a.omb2 * g * g;
        const float denom = __builtin_amdgcn_sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
        return p - a.lr_bc1 * m * __builtin_amdgcn_rcpf(denom);
    } else {
        v = a.b2 * v + a.omb2 * g * g + 1e-12f;
        const float denom = __builtin_amdgcn_sqrtf(v * a.inv_bc2) + a.eps;
        return p - a.lr * (m * a.inv_bc1) * __builtin_amdgcn_rcpf(denom);
    }
}

// ------------------------------------------------------------- plan layout
struct LayerInfo {
    int din, dout;
    int n;          // out*in + out (sampled elements per layer and sample)
    int64_t nc;     // full-cov: packed corr count (n-1)(n-2)/2
    int64_t poff;   // offset of the layer in the flat parameter vector
    int64_t eoff;   // offset of the layer in the flat eps vector (all S)
    int woff;       // offset of the layer in the per-sample weight space [0, n_tot)
    int64_t tbase;  // full-cov tiled layout: first 64x64 tile of the layer
    int nb;         // full-cov: 64-row bands covering rows 0 .. n-1
};

// Full-cov forward work item: rows [r0, r1) (<= kFwdRows) of layer `layer`
// (global row ids, clipped to the rank's row range), columns c in [k0, k1) of L.
constexpr int kFwdRows = 64;
struct FwdItem {
    int layer, r0, r1, k0, k1, xcol;  // xcol: x_shard column of row r0
    int slot;                         // partial-sum slot ([S][kFwdRows] floats) of this item
};
// Rows [r0, r0 + R) (R <= kFwdRows) of one layer: their x = sum of the nk partial
// slots slot0 .. slot0 + nk - 1 (split-K over the columns of L, no atomics).
struct FwdRowBlock {
    int slot0, nk, R, xcol;
    int layer, r0;  // absolute first row (the reduce adds mean + softplus(sd) eps)
    int s0;         // first sample of the block's slots (segmented sample: a pass's 128)
};
// Segmented sample (mvn_fwd_seg_kernel, K = S > 128): units (row block,
// 128-sample pass, 64-column block of L), row block-major then pass then
// column block, cut into equal contiguous runs, one per workgroup; a run's
// piece of one (row block, pass) is a segment with its own partial slot
// ([128][kFwdRows] floats), and the reduce adds a (row block, pass)'s slots.
struct FsSeg {
    int layer, r0, r1, pass;  // rows [r0, r1) of layer, samples [128 pass, 128 pass + 128)
    int k0, k1, slot, pad;    // columns [k0, k1) of L (64-column blocks)
};
// Full-cov update work item: the 64-row band [r0, r0+64) of layer `layer`
// (r0 a multiple of 64; the rank owns rows [rlo, rhi)) against the c-blocks
// [k0, k1) (columns [64 k0, 64 k1)).  The band's G slice is staged once and
// reused across the chunk's c-blocks; the chunk holding c-block r0/64 (diag)
// also updates the band's mean and sd.  xcol: g_shard column of row r is xcol + r.
struct UpdChunk {
    int layer, r0, k0, k1, rlo, rhi, xcol, diag;
    int slot;  // fused next-step sample: partial-sum slot ([S][64] floats), -1 if none
};

// K-split streaming update (mvn_kstream_kernel; Adam, packed state, K = S >
// 128): the rank's 64 x 64 tiles, each K = S samples cut in passes of 128;
// the (tile, pass) units, tile-major, are cut into equal contiguous runs, one
// per workgroup.  A tile whose passes span several runs is "split": each
// contributor writes its partial dL (and diagonal sums) to its slot, and the
// contributor whose count comes last adds the partials in pass order and
// runs the tile's Adam epilogue.
struct KsTile {
    int layer, r0, k, diag;  // band rows [r0, r0 + 64), c-block k, k == band
    int rlo, rhi, xcol;      // rows of the band that exist (< n); g_shard column of row r: xcol + r
    int cnt;                 // counter index of a split tile (-1: never split)
};
constexpr int kKsPass = 128;               // samples per pass (the kernel's LDS stage)
constexpr int kKsSlotFloats = 4096 + 512;  // a split tile's partial: dL fragments, diagonal sums
struct KsSeg {
    int tile, p0, p1;  // passes [p0, p1) of the tile
    int slot, nc, ci;  // split tiles: first slot, contributors, this one's index (slot -1: whole tile)
};

// Streaming fused update (mvn_stream_kernel): workgroup w walks tiles
// [t0, t1) of the layer-major, band-major tile list; its x' partial of each
// band it touches goes to slots slot0, slot0 + 1, ... (a band's slots are
// consecutive over the workgroups).
struct StreamRange {
    int t0, t1, slot0;
    uint32_t lbk0;  // tile t0 as layer << 28 | b << 14 | k
};

// A rank's full-cov rows: rows [lo, hi) of `layer` sit at x-shard columns
// col .. col + hi - lo (world > 1: runs of whole 64-row bands; world 1 and the
// replicated families: one run per layer)
struct ShardRun {
    int layer, lo, hi, col;
};

// world > 1 full-cov network kernel: g_send offset of a 64-row band's first
// row for local sample 0 (owner block + column - first row) and the owner's
// row stride (its rows_total)
struct NetBand {
    int64_t base;
    int32_t stride, pad;
};

struct NetArgs;  // kernels_net.hip

// The R-op kernels' dynamic-LDS layouts (lds_layout.hpp: rop_valu_lds,
// rop_mfma_lds) as float offsets from the LDS base, handed to the kernels by
// value.  net_rop_kernel (VALU), rows in chunks of rc:
struct RopValuLds {
    int rc;    // rows per chunk
    int maxd;  // odd row stride of the delta buffers
    // W_l / W_dot_l: rows of an odd stride ldw[l] (a lane per output row then
    // hits its own bank), layer l at xo[l] of the X (lx) / X_dot (lxd) regions,
    // b after W
    int lx, lxd, ldw[kMaxL], xo[kMaxL];
    int lg, lgd;                         // G / G_dot accumulators [n_tot] (chunked rows only)
    int lh[kMaxL + 1], lhd[kMaxL + 1];   // h_l / h_dot_l [rc][width_l]
    int ld0, ld1, ldd0, ldd1;            // delta / delta_dot, double-buffered [rc][maxd]
    size_t bytes;
};
// net_rop_mfma_kernel (matrix cores), a row block in one pass.  X_l (l = 0..L)
// at mxo[l], rows of ldxm[l] floats = [h | h_dot] halves of kx[l] = rup16(width)
// (X_0: the u rows alone; X_L: logits and their tangents); W2_l at mwo[l],
// rup16(dout) rows of ldwm[l] = [W | W_dot] halves of kx[l]; b_l | b_dot_l at
// mbo[l] (halves of kx[l + 1]); the diagnostics' phase clocks at lstamp.
// Load jobs: layer l's W2 rows from jw[l], bias rows from jb + jbl[l], u rows from ju
struct RopMfmaLds {
    int mxo[kMaxL + 1], ldxm[kMaxL + 1], kx[kMaxL + 1], mwo[kMaxL], ldwm[kMaxL], mbo[kMaxL], lstamp;
    int jw[kMaxL], jbl[kMaxL], jb, ju;
    size_t bytes;
};
// What launch_net_rop launches for a plan (rop_geometry, lds_shapes.cpp): both
// forms, since PSVI_DBG_ROP_VALU picks between them at launch time.
struct RopGeometry {
    int nsplit;       // workgroups per sample (row blocks), each with its own G / G_dot slot
    bool mfma_fits;   // the matrix-core form's row block fits the LDS in one pass
    int mfma_rows;    // its rows, padded to a 16-multiple
    RopMfmaLds mfma;
    int single;       // VALU: a workgroup's rows are one chunk (no LDS accumulators)
    RopValuLds valu;  // valu.rc == 0: the model's weights alone do not fit (unsupported)
};

// Outer-objective passes of the network kernel (psvi_outer_elbo_grad).
struct NetOuter {
    int mode;             // 1 forward (per-row NLL), 2 backward (row coefficients)
    int n_pseudo;         // rows [0, n_pseudo) are pseudopoints, the rest data
    float* nll_rows;      // mode 1: [S][M] unweighted NLL
    const float* rowcoef; // mode 2: [S][2] d loss / d pseudo_s, d loss / d data_s
    const float* ck;      // mode 2: [S] d loss / d nkl_s
    float* du_part;       // mode 2, nullable: [S][n_pseudo][D] input gradient
    float* prob_rows;     // mode 1, nullable: [S][M - n_pseudo][C] softmax of the data rows
                          // (Gaussian plans: the raw output f, C = 1)
    float* dz_part;       // mode 2, nullable, Gaussian plans: [S][n_pseudo] d loss_s / d z_m
    bool loglik = false;  // mode 1, Bernoulli plans: nll_rows receives -NLL (psvi_row_loglik)
};

// ------------------------------------------------------ plan-owned memory
// A work list of a plan: the host copy, built with the plan, and the device
// copy upload() makes of it, freed with the table.  The list's length is the
// host vector's (an empty list has no device copy).
template <class T>
struct DevTable {
    std::vector<T> host;
    T* dev = nullptr;
    DevTable() = default;
    DevTable(const DevTable&) = delete;
    DevTable& operator=(const DevTable&) = delete;
    ~DevTable() {
        if (dev) (void)hipFree(dev);
    }
    int n() const { return (int)host.size(); }
    // *what: the call that failed, as the error message names it
    hipError_t upload(const char** what) {
        if (host.empty()) return hipSuccess;
        *what = "hipMalloc((void**)dst, sizeof(T) * v.size())";
        hipError_t e = hipMalloc((void**)&dev, sizeof(T) * host.size());
        if (e != hipSuccess) {
            dev = nullptr;
            return e;
        }
        *what = "hipMemcpy(*dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice)";
        return hipMemcpy(dev, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice);
    }
};

// Plan-owned device scratch, freed with the buffer.
template <class T>
struct DevBuffer {
    T* dev = nullptr;
    DevBuffer() = default;
    DevBuffer(const DevBuffer&) = delete;
    DevBuffer& operator=(const DevBuffer&) = delete;
    ~DevBuffer() {
        if (dev) (void)hipFree(dev);
    }
    void release() {
        if (dev) (void)hipFree(dev);
        dev = nullptr;
    }
    bool alloc(size_t bytes, bool zero = false) {
        if (hipMalloc((void**)&dev, bytes) != hipSuccess) {
            dev = nullptr;
            return false;
        }
        return !zero || hipMemset(dev, 0, bytes) == hipSuccess;
    }
};

// A side stream of a plan with the events that fork it from and join it to the
// caller's stream.
struct AuxStream {
    hipStream_t st = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    AuxStream() = default;
    AuxStream(const AuxStream&) = delete;
    AuxStream& operator=(const AuxStream&) = delete;
    ~AuxStream() {
        if (fork) (void)hipEventDestroy(fork);
        if (join) (void)hipEventDestroy(join);
        if (st) (void)hipStreamDestroy(st);
    }
    bool create() {
        return hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
               hipEventCreateWithFlags(&fork, hipEventDisableTiming) == hipSuccess &&
               hipEventCreateWithFlags(&join, hipEventDisableTiming) == hipSuccess;
    }
};

}  // namespace psvi

// The device members own their memory: a plan is not copyable, and deleting
// it releases everything.
struct psvi_plan {
    int family = 0;
    // observation model (psvi_plan_create_lik): PSVI_LIK_GAUSSIAN plans are
    // mean-field, C = 1, world 1; z / z_all then point to fp32 targets
    int lik = PSVI_LIK_CATEGORICAL;
    float lik_tau = 1.f;
    psvi_net_desc d{};
    int world = 1, rank = 0;
    int L = 0;
    psvi::LayerInfo lay[psvi::kMaxL];
    int64_t P = 0;        // parameter count
    int64_t Peps = 0;     // eps floats for all S
    int n_tot = 0;        // per-sample weight-space size (sum n)
    // sample shards
    int s_off[psvi::kMaxWorld], s_cnt[psvi::kMaxWorld];
    // full-cov row shards: each rank's runs of rows (whole 64-row bands at
    // world > 1, dealt largest first to the least-loaded rank), its x-shard
    // columns layer-major in row order
    std::vector<psvi::ShardRun> runs[psvi::kMaxWorld];
    int rows_tot[psvi::kMaxWorld];
    int xcol_l[psvi::kMaxWorld][psvi::kMaxL];  // column of layer l's first row in a shard
    // world > 1 full-cov: owner rank and (x-shard column - first row) of every
    // 64-row band, bands numbered layer by layer from band_base[l]
    std::vector<int> band_owner, band_coloff;
    int band_base[psvi::kMaxL + 1] = {0};
    // network kernel: LDS destination of every x element the workgroup loads
    // (stage position -> W_l / b_l offset | W_l^T offset << 16, 0xFFFF = none)
    // and, world > 1, the band table (owner, column offset); filled at upload
    psvi::DevTable<uint32_t> xmap;
    psvi::DevTable<psvi::NetBand> net_bands;
    bool on_device = false;  // the tables are uploaded and the scratch allocated
    // sample phase: forward items, their row blocks, split-K partial slots
    // (fwd.n() x S x kFwdRows floats)
    psvi::DevTable<psvi::FwdItem> fwd;
    psvi::DevTable<psvi::FwdRowBlock> frb;
    psvi::DevBuffer<float> fwd_part;
    // update chunks (XCD order, padded with empty chunks)
    psvi::DevTable<psvi::UpdChunk> upd;
    int upd_tiles = 0;  // c-blocks over all chunks (work measure)
    // fused update + next-step sample (world == 1, S <= 128): one row block
    // per 64-row band, one partial slot per chunk
    bool fuse_sample = false;
    // tiled corr/m/v (world == 1, S <= 128 inner loops): 64x64 tiles (b, k <= b)
    // per layer in MFMA fragment order, tiles_total * 4096 floats per array
    int64_t tiles_total = 0;
    psvi::DevTable<psvi::FwdRowBlock> ufrb;
    int n_uslots = 0;
    psvi::DevBuffer<float> upd_part;
    // streaming fused update (fuse_sample plans with S % 32 == 0): one
    // workgroup per range, band row blocks over its slots
    psvi::DevTable<psvi::StreamRange> str;
    psvi::DevTable<psvi::FwdRowBlock> sfrb;
    psvi::DevBuffer<float> str_part;
    psvi::DevBuffer<int> str_cnt;    // the in-kernel band combine's arrival counters (sfrb.n())
    psvi::DevBuffer<float> str_bms;  // per band: new mean + softplus(sd), 128 floats (sfrb.n())
    int str_max_ends = 0;            // most band ends (slots) in one run of the stream
    int n_sslots = 0;
    // K-split streaming update (full-cov Adam steps with S > 128): tiles, the
    // workgroups' segment lists (offsets [n_kwg() + 1]), split-tile partial slots
    // (kKsSlotFloats each) and their arrival counters (zeroed, reset by use)
    psvi::DevTable<psvi::KsTile> ks_tiles;
    psvi::DevTable<psvi::KsSeg> ks_segs;
    psvi::DevTable<int> ks_off;
    psvi::DevBuffer<float> ks_slots;
    psvi::DevBuffer<int> ks_cnt;
    int n_ks_slots = 0, n_ks_cnt = 0;
    // segmented sample (S > 128): segments, per-workgroup offsets, (row block,
    // pass) reduce blocks, partial slots ([n_fs_slots][128][kFwdRows])
    psvi::DevTable<psvi::FsSeg> fs_segs;
    psvi::DevTable<int> fs_off;
    psvi::DevTable<psvi::FwdRowBlock> fs_rb;
    psvi::DevBuffer<float> fs_part;
    int n_fs_slots = 0;
    // psvi_hvp's sample pair (one eight-wave workgroup per CU): the same units
    // over 256 workgroups, slots in fs_part (sized for both tables)
    psvi::DevTable<psvi::FsSeg> fp_segs;
    psvi::DevTable<int> fp_off;
    psvi::DevTable<psvi::FwdRowBlock> fp_rb;
    int n_fp_slots = 0;
    // workgroups of a segment table: its offset list less the closing entry
    static int n_wg(const psvi::DevTable<int>& off) { return std::max(0, off.n() - 1); }
    int n_kwg() const { return n_wg(ks_off); }
    int n_fswg() const { return n_wg(fs_off); }
    int n_fpwg() const { return n_wg(fp_off); }
    // net kernel geometry
    int mchunks = 1, mc = 0, net_threads = 256, net_roles = 1;
    bool net_mloop = false;  // full-cov inner objective: the LDS-forced chunks looped in a workgroup
    size_t net_lds = 0;
    psvi::RopGeometry rop{};  // psvi_hvp's R-op (mean-field and full-cov)
    size_t ws_bytes = 0;
    int64_t acc_count = 0;
    // LeNet: plan-owned activation / gradient scratch (kernels_lenet.hip)
    psvi::DevBuffer<void> lenet_scratch;
    // mean-field: plan-owned per-(sample, pseudopoint chunk) gradient slots
    // [s_cnt[rank]][mchunks][n_tot]; one writer per element, summed in a fixed
    // order by the update (run-to-run bitwise reproducible, no float atomics)
    psvi::DevBuffer<float> mf_slots;
    // mean-field categorical, world 1: psvi_predict_scores's scratch (the
    // workgroups' statistics partials, then softplus(rho); predict_scratch_bytes)
    psvi::DevBuffer<void> pred_scratch;
    // full-cov with pseudopoint chunks: per-chunk dW slots [mchunks][s_cnt[rank]][n_tot],
    // added in chunk order into g_send (no float atomics)
    psvi::DevBuffer<float> net_slots;
    // tiled-state inner loops: the packed -> tiled conversion runs on aux.st,
    // forked from / joined to the caller's stream by the two events, behind the
    // first sample and network step (not re-entrant across host threads)
    psvi::AuxStream aux;
    // bf16-plane streaming update (tiled S = 128 loops): every eps draw of
    // the loop also as three bf16 planes (EpsPlanes; device copy for the
    // network kernel's fused draw), two plane buffers in the loop workspace
    bool bf_stream = false;
    bool eps_planes_ok = false;  // eps_planes describes this plan's draw (full-cov, world 1)
    psvi::EpsPlanes eps_planes{};
    psvi::DevTable<psvi::EpsPlanes> eps_planes_tab;  // eps_planes, for the device
    // psvi_inner_loop_ex(PSVI_LOOP_KEEP): what the last call left in its
    // workspace -- the tiled corr / m / v, the draw at `offset` (eps buffer
    // `ebuf`, and its planes) and the sample x from it -- and for which
    // arrays; any loop call clears it first (mutable: the API's plans are const)
    struct Resident {
        bool valid = false;
        const void* ws = nullptr;
        const float *params = nullptr, *m = nullptr, *v = nullptr;
        uint64_t seed = 0, offset = 0;
        int ebuf = 0;
    };
    mutable Resident resident{};
};

namespace psvi {
// input features per row: D, or 1x28x28 for LeNet
inline int plan_in_dim(const psvi_plan& p) {
    return p.family == PSVI_FAMILY_LENET ? 784 : p.lay[0].din;
}
// layers whose sampled KL enters psvi_elbo (LeNet: the VILinear layers only,
// psvi_classes.py:455-459 sums sampled_nkl over VILinear modules)
inline unsigned plan_nkl_mask(const psvi_plan& p) {
    return p.family == PSVI_FAMILY_LENET ? 0x1Cu : 0xFFu;
}
// Plan building (plan_tables.cpp: host only, no HIP call): the layout, the
// shards, the network geometry and every work list of a plan whose family, d,
// world and rank are set.  Returns 0, or a PSVI_E* code with its message in err.
int build_plan(psvi_plan& p, std::string& err);
// the network kernel's chunking and LDS size (kernels_net.hip: its LDS layout)
size_t net_plan_geometry(psvi_plan& p);
// A launch of `kernel` with up to `bytes` of dynamic LDS (above the 64 KiB a
// launch gets unasked) on the current device: the opt-in is made once per
// (kernel, device), whichever thread asks first (capi_plan.cpp)
hipError_t allow_dynamic_lds(const void* kernel, size_t bytes);
// the same for every network kernel (kernels_net.hip) and every R-op kernel
// (kernels_rop.hip): at plan creation, so launch_net and launch_net_rop make
// no runtime call for it
hipError_t net_allow_lds();
hipError_t rop_allow_lds();
// psvi_debug_set values read when a plan is built
struct PlanDebug {
    int stream_wgs = 0;       // PSVI_DBG_STREAM_WGS: streaming-update workgroups (0 = 256)
    int stream_rr = 0;        // PSVI_DBG_STREAM_RR, 1: runs dealt round-robin over XCDs (A/B)
    int stream_cost = -1;     // PSVI_DBG_STREAM_COST, first% + 1000 diag%: tile cost weights (tuning)
    int upd_chunk_tiles = 0;  // PSVI_DBG_UPD_CHUNK: c-blocks per update chunk (0 = auto)
    int ks_wgs = 0;           // PSVI_DBG_KSTREAM_WGS: K-split update workgroups (0 = 512)
};
extern PlanDebug g_plan_dbg;
// psvi_debug_set / psvi_debug_set_ptr values read when a kernel is launched (and
// by net_plan_geometry): A/B switches, ablation masks and stamp buffers, all 0 /
// nullptr in production unless a default says otherwise (psvi_diag.h; capi_plan.cpp)
struct Diag {
    using Stamps = unsigned long long*;  // 16 slots per workgroup
    int net_ablation = 0;         // PSVI_DBG_NET_ABLATION, mask
    int net_threads = 0;          // PSVI_DBG_NET_THREADS, n: 0 = by chunk size
    int net_split_below = 256;    // PSVI_DBG_NET_SPLIT_BELOW, n: split when a rank has fewer samples than CUs
    int net_wg_target = 256;      // PSVI_DBG_NET_WG_TARGET, n: workgroups a split rank aims for
    int net_mloop_off = 0;        // PSVI_DBG_NET_MLOOP_OFF, 1: a workgroup per pseudopoint chunk + slots (A/B)
    int net_scalar_loads = 0;     // PSVI_DBG_NET_SCALAR_LOADS, 1: the scalar load path (A/B)
    int net_geo_off = 0;          // PSVI_DBG_NET_GEO_OFF, 1: the run-time geometry for fn2 too (A/B)
    int net_draw_role1 = 17;      // PSVI_DBG_NET_DRAW_ROLE1, n: role 1's 32nds of the fused draw
    int net_draw_spare_off = 0;   // PSVI_DBG_NET_DRAW_SPARE_OFF, 1: the whole draw at the end (A/B)
    Stamps net_stamps = nullptr;  // PSVI_DBG_NET_STAMPS
    uint16_t* net_draw_planes = nullptr;  // PSVI_DBG_NET_DRAW_PLANES
    int fwd_ablation = 0;         // PSVI_DBG_FWD_ABLATION, mask
    Stamps fwd_stamps = nullptr;  // PSVI_DBG_FWD_STAMPS
    int fs_off = 0;               // PSVI_DBG_FWD_SEG_OFF, 1: the item-grid sample kernel at S > 128 (A/B)
    int fs_bf_off = 0;            // PSVI_DBG_FWD_SEG_BF_OFF, 1: the fp32 segmented sample (A/B)
    int fwd_pair_bf = 1;          // PSVI_DBG_FWD_PAIR_BF, 0: the HVP's sample pair on the fp32 item grid (A/B)
    int upd_ablation = 0;         // PSVI_DBG_UPD_ABLATION, mask
    Stamps upd_stamps = nullptr;  // PSVI_DBG_UPD_STAMPS
    int stream_off = 0;           // PSVI_DBG_UPD_STREAM_OFF, 1: the chunked kernel (A/B)
    int stream_bf_off = 0;        // PSVI_DBG_STREAM_BF_OFF, 1: the fp32-MFMA streaming kernel (A/B)
    int stream_fold_off = 0;      // PSVI_DBG_STREAM_FOLD_OFF, 1: the band combine as mvn_fwd_reduce_kernel (A/B)
    Stamps bf_stamps = nullptr;   // PSVI_DBG_BF_STAMPS
    int ks_off = 0;               // PSVI_DBG_KSTREAM_OFF, 1: the chunked kernel at S > 128 (A/B)
    int ks_bf_off = 0;            // PSVI_DBG_KSTREAM_BF_OFF, 1: the fp32 K-split update (A/B)
    int rop_valu = 0;             // PSVI_DBG_ROP_VALU, 1: the VALU R-op kernel (the form for row blocks past the LDS) on every shape (A/B)
    Stamps rop_stamps = nullptr;  // PSVI_DBG_ROP_STAMPS
    int lenet_abl = 0;            // PSVI_DBG_LENET_ABLATION, mask: backward parts skipped
};
extern Diag g_diag;
// the full-cov network kernel's x map and band table (kernels_net.hip)
void net_xmap(const psvi_plan& p, std::vector<uint32_t>& xmap, std::vector<NetBand>& bands);
// Per-row targets of the loss head: class labels (categorical plans) or fp32
// values (Gaussian plans), one 4-byte slot per row either way.
struct Targets {
    const void* p = nullptr;
    static Targets labels(const int32_t* z) { return Targets{z}; }
    static Targets values(const float* y) { return Targets{y}; }
    // the slots as the kernels' argument structs declare them (`const int32_t*
    // z`; the Gaussian head reads the same slots as fp32): the one cast
    const int32_t* slots() const { return static_cast<const int32_t*>(p); }
};

// launchers (defined in the .hip translation units).  Those with optional
// inputs take a request struct: every optional field defaults to "absent", a
// caller assigns the fields it means.
struct NetLaunch {
    // rows
    const float* u = nullptr;
    Targets targets;
    const float* w = nullptr;
    // mean-field inputs (mf_slots: the plan's gradient slots)
    const float* params = nullptr;
    const float* eps = nullptr;
    float* mf_slots = nullptr;
    // full-cov inputs
    const float* xrecv = nullptr;
    float* gsend = nullptr;
    double* nll_out = nullptr;
    // fused draw of the next step's eps: normals [0, n) of the Philox stream
    // (seed, offset) into out (and their bf16 planes), this launch drawing
    // part `part` of `nparts` of its quads
    struct Draw {
        float* out = nullptr;
        int64_t n = 0;
        uint64_t seed = 0, offset = 0;
        uint16_t* planes = nullptr;
        int part = 0, nparts = 1;
    } draw;
    // the rank's local samples [s_begin, s_begin + s_count) (-1: to the last)
    int s_begin = 0, s_count = -1;
    const NetOuter* outer = nullptr;
};
hipError_t launch_net(const psvi_plan& p, const NetLaunch& r, hipStream_t st);
// acc == nullptr: the accumulators come from the plan's mean-field gradient
// slots, reduced in a fixed order against slot_eps (the step's eps)
struct MfUpdate {
    const float* acc = nullptr;
    const float* slot_eps = nullptr;
    float* params = nullptr;
    float* m = nullptr;
    float* v = nullptr;
    const psvi_adam_hp* hp = nullptr;
    double* kl_out = nullptr;
    float* grad_out = nullptr;  // gradient mode: no Adam step
    int include_kl = 0;
};
hipError_t launch_mf_update(const psvi_plan& p, const MfUpdate& r, hipStream_t st);
// acc = [sum_s dW_s | sum_s dW_s eps_s] from the plan's mean-field gradient slots
hipError_t launch_mf_slot_acc(const psvi_plan& p, const float* eps, float* acc, hipStream_t st);
// diag_of (HVP tangent sample): params is the direction, the diagonal
// sigmoid(diag_of's sd) * its sd slot
hipError_t launch_mvn_fwd(const psvi_plan& p, const float* eps, const float* params,
                          float* x_shard, hipStream_t st, const float* diag_of = nullptr);
hipError_t launch_mvn_fwd_pair(const psvi_plan& p, const float* eps, const float* params,
                               float* x, const float* vec, float* x2, float* part2,
                               hipStream_t st);
struct MvnUpdate {
    const float* eps = nullptr;
    const float* g_shard = nullptr;
    const float* g_shard2 = nullptr;  // see mvn_grad_takes_slots
    float* params = nullptr;
    float* m = nullptr;
    float* v = nullptr;
    const psvi_adam_hp* hp = nullptr;
    double* kl_out = nullptr;
    float* grad_out = nullptr;  // gradient mode: no Adam step
    int include_kl = 0;
    const float* kl_vec = nullptr;  // gradient mode: + kl_vec / s0^2 on the corr entries
    // the next step's sample x from the updated parameters (planes: eps as bf16 planes)
    struct Next {
        const float* eps = nullptr;
        float* x = nullptr;
        const uint16_t* planes = nullptr;
    } next;
    float* tstate = nullptr;  // tiled corr / m / v (psvi_inner_loop on a fusable plan)
    bool packed_out = false;  // tiled state: write corr / m / v back to the packed arrays
    bool padded = false;      // eps, next.eps and g_shard end in 64 zeroed floats
    const uint16_t* eps_planes = nullptr;
};
hipError_t launch_mvn_update(const psvi_plan& p, const MvnUpdate& r, hipStream_t st);
// the gradient-mode update takes a second G slot (g_shard2: added to g_shard at
// staging, the R-op's row-block slots unsummed) when this holds
bool mvn_grad_takes_slots(const psvi_plan& p);
// pads (to_tiled, nullable): three 64-float regions the first workgroup zeroes
hipError_t launch_mvn_tile_convert(const psvi_plan& p, float* params, float* m, float* v,
                                   float* tstate, bool to_tiled, hipStream_t st,
                                   float* const* pads = nullptr);
struct RandnLaunch {
    float* out = nullptr;
    int64_t n = 0;
    uint64_t seed = 0, offset = 0;
    double* zero = nullptr;  // the same launch also clears zero[0, nzero)
    int64_t nzero = 0;
    const EpsPlanes* planes_desc = nullptr;  // with planes: the draw also as bf16 planes
    uint16_t* planes = nullptr;
    int64_t q_lo = 0, q_hi = -1;  // quads [q_lo, q_hi) only (-1: all)
};
hipError_t launch_randn(const RandnLaunch& r, hipStream_t st);
hipError_t launch_adam(int64_t n, float* p, const float* g, float* m, float* v,
                       const psvi_adam_hp* hp, hipStream_t st);
AdamC make_adam(const psvi_adam_hp* hp);
hipError_t launch_adam_adjoint(int64_t n, const float* lt, float* lm, float* lv, const float* m,
                               const float* v, const float* g, float* lg,
                               const psvi_adam_hp* hp, hipStream_t st);
// sampled KL of a mean-field plan (kernels_mf.hip): nkl_out [S] doubles
// (nullable), grad_out [P] += d(-sum_s nkl_s) / d params (nullable)
hipError_t launch_mf_sampled_kl(const psvi_plan& p, const float* eps, const float* params,
                                double* nkl_out, float* grad_out, hipStream_t st);
// sparse black-box VI (kernels_select.hip): selection scores and the weight
// objective from ll [S][Nu + B] and nkl [S]
hipError_t launch_select_scores(int S, int Nu, int B, const float* ll, const double* nkl,
                                const float* w, double sum_scaling, float* W_out, float* corr,
                                float* corecorr, double* result, hipStream_t st);
hipError_t launch_select_weight_grad(int S, int Nu, int B, const float* ll, const double* nkl,
                                     const float* w, double N, double* loss, float* grad_w,
                                     hipStream_t st);
// Laplace coreset baselines (kernels_laplace.hip).  The fit: T torch-Adam steps
// on theta [d] of the weighted logistic log-joint of x [Nu][d] / y / w in one
// workgroup, then the diagonal precision and (eps given) S samples from it.
constexpr int kSelThreads = 512;   // the one-workgroup selection, scores and GIGA kernels
constexpr int kLapThreads = 256;   // the fit's and the full-precision samples' workgroup
constexpr size_t kLapLds = 160 * 1024;  // their dynamic-LDS cap
constexpr int kSelMaxS = 2048;     // their per-sample terms live in LDS
constexpr int kLapMaxD = 256;      // one column owner per thread of the fit's workgroup
constexpr int kLapMaxNu = 4096;    // the fit's per-row terms live in LDS
constexpr int kLapMaxRows = 2048;  // the scores' per-row means live in LDS
constexpr int kLapMaxT = 1 << 20;
struct LaplaceFit {
    int Nu = 0, d = 0, S = 0, T = 0;
    const float* x = nullptr;
    const float* y = nullptr;
    const float* w = nullptr;
    double mu0 = 0.0, sd0 = 1.0;
    float* theta = nullptr;  // in / out
    double lr = 1e-3, beta1 = 0.9, beta2 = 0.999, adam_eps = 1e-8;
    const float* eps = nullptr;    // [S][d], nullable
    double* loss_out = nullptr;    // [T], nullable
    float* prec_out = nullptr;     // [d]
    float* samples_out = nullptr;  // [S][d], written when eps is given
};
hipError_t launch_laplace_fit(const LaplaceFit& r, hipStream_t st);
// the full precision P = I + x^T diag(w p (1 - p)) x at theta, its reverse
// Cholesky factor A (A^T A = P) and S samples theta + A^-1 eps_s, one workgroup
constexpr int kLapFullMaxD = 128;  // the packed triangle of P and the samples' y live in LDS
struct LaplaceSampleFull {
    int Nu = 0, d = 0, S = 0;
    const float* x = nullptr;
    const float* w = nullptr;
    const float* theta = nullptr;
    const float* eps = nullptr;     // [S][d], null iff S == 0
    float* prec_out = nullptr;      // [d][d], nullable
    float* factor_out = nullptr;    // [d][d], nullable
    float* samples_out = nullptr;   // [S][d]
    double* logdet_out = nullptr;   // [1], nullable
};
hipError_t launch_laplace_sample_full(const LaplaceSampleFull& r, hipStream_t st);
// scores, weight gradient and pseudo-input gradient from samples [S][d] and
// rows [Nu + B][d] (core rows first)
struct LaplaceScores {
    int S = 0, d = 0, Nu = 0, B = 0;
    const float* samples = nullptr;
    const float* rows = nullptr;
    const float* labels = nullptr;
    const float* w = nullptr;
    double sum_scaling = 1.0;
    float* corr = nullptr;      // [B]
    float* corecorr = nullptr;  // [Nu]
    double* result = nullptr;   // [4]
    float* grad_w = nullptr;    // [Nu], nullable
    float* ll_out = nullptr;    // [S][Nu + B], nullable
    float* grad_u = nullptr;    // [Nu][d], nullable
};
hipError_t launch_laplace_scores(const LaplaceScores& r, hipStream_t st);
// one geodesic-ascent step of GIGA from samples [S][d] and the minibatch rows
struct GigaStep {
    int S = 0, d = 0, n_data = 0;
    const float* samples = nullptr;
    const float* rows = nullptr;    // [n_data][d]
    const float* labels = nullptr;  // [n_data]
    const float* lw_in = nullptr;   // [S]
    float* score = nullptr;         // [n_data]
    float* lw_out = nullptr;        // [S], not lw_in
    float* ll_out = nullptr;        // [S][n_data], nullable
    double* result = nullptr;       // [8]
};
hipError_t launch_giga_step(const GigaStep& r, hipStream_t st);
// coreset rows drawn in proportion to their weights (kernels_draw.hip), with
// the gather of the drawn rows and targets
constexpr int kDrawMaxM = 4096;       // the fp64 prefix / the sort's keys live in LDS
constexpr int64_t kDrawMaxN = 1 << 24;
struct CoresetDraw {
    const float* w = nullptr;  // [M]
    int M = 0;
    int64_t n = 0;
    bool replace = true;
    uint64_t seed = 0, offset = 0;
    const float* rows = nullptr;    // [M][D], nullable
    int64_t D = 0;
    const void* targets = nullptr;  // [M] 4-byte slots, nullable
    int32_t* idx_out = nullptr;     // [n]
    float* rows_out = nullptr;      // [n][D]
    void* targets_out = nullptr;    // [n]
    int32_t* status_out = nullptr;  // [1]
};
hipError_t launch_coreset_draw(const CoresetDraw& r, hipStream_t st);
// k-means clustering of rows (kernels_kmeans.hip): k-means++ seeding on the
// Philox stream and Lloyd iterations, every deciding number in fp64
constexpr int kKmMaxK = 128, kKmMaxD = 4096;
constexpr int64_t kKmMaxN = 1 << 24;
constexpr int kKmThreads = 256;
constexpr int kKmRows = 64;        // rows of a tile, and of a run of the seeding's prefix sum
constexpr int kKmMaxGrid = 512;    // assignment workgroups: the partials of the one-pass sums
constexpr int kKmMaxParts = 256;   // row chunks of the second-pass sums
constexpr int kKmChunk = 16;       // iterations enqueued between two host reads of `done`
constexpr size_t kKmLds = 76 * 1024;  // dynamic LDS of an assignment workgroup: two per CU
// what a shape needs (host only): the column tile, the grids and the bytes
struct KmeansShape {
    int DT = 0;       // columns of a tile: the centres' fp64 tile and the rows' fp32 tile share kKmLds
    int XS = 0;       // stride of the row tile (odd: no bank conflicts down a column)
    int tiles = 0, tpb = 0, G = 0;  // row tiles, tiles per assignment workgroup, workgroups
    int nruns = 0;    // runs of kKmRows rows
    int cy = 0;       // combine grid: (K, cy), kKmThreads columns each
    size_t part = 0;  // bytes of one [K][D] fp64 partial
    size_t fixed = 0; // bytes before the partials
    size_t min_bytes = 0, full_bytes = 0;  // one partial / G partials
};
// (fixed: what the workspace's carve takes before the partials, kernels_kmeans.hip)
KmeansShape kmeans_shape(int64_t N, int D, int K);
struct Kmeans {
    const float* x = nullptr;  // [N][D]
    int N = 0, D = 0, K = 0;
    const double* centres_in = nullptr;  // [K][D], nullable
    uint64_t seed = 0, offset = 0;
    int max_iter = 0;
    double tol = 0.0;
    double* centres = nullptr;     // [K][D]: the working centres and the result
    int32_t* labels = nullptr;     // [N]
    int32_t* counts = nullptr;     // [K]
    int32_t* seeds = nullptr;      // [K], nullable
    double* inertia = nullptr;     // [1]
    int32_t* n_iter = nullptr;     // [1]
    int32_t* status = nullptr;     // [1]
    void* ws = nullptr;
    size_t ws_bytes = 0;
};
// synchronises the stream once per kKmChunk iterations (the `done` word)
hipError_t launch_kmeans(const Kmeans& r, hipStream_t st);
// MFVI regressor fit (kernels_mfvi_fit.hip): T chained steps of a mean-field
// Gaussian-likelihood MLP on a fixed batch for G members, one workgroup each.
constexpr int kMfFitThreads = 512;
constexpr size_t kMfFitLds = 160 * 1024;
constexpr int kMfFitMaxL = 4;    // affine layers: 1..3 hidden layers and the head
constexpr int kMfFitMaxG = 16;
constexpr int kMfFitMaxD = 128, kMfFitMaxH = 64, kMfFitMaxB = 512, kMfFitMaxS = 64;
constexpr int kMfFitMaxT = 1 << 20;
// what a descriptor's fit needs: the placement of the state (params / m / v,
// the accumulators and the batch: LDS, or global memory with the per-member
// workspace ws_bytes), the rows per chunk and the LDS strides
struct MfviFitShape {
    int L = 0, B = 0, S = 0, n_tot = 0, hs = 0, xs = 0, RB = 0;
    int64_t eps_count = 0;
    bool lds = false;
    size_t ws_bytes = 0;
};
// 0, or PSVI_EUNSUP when not even one row fits beside the working set
int mfvi_fit_shape(const psvi_net_desc& d, MfviFitShape& s);
struct MfviFit {
    MfviFitShape shape;
    int dims[kMfFitMaxL + 1] = {};
    int G = 0, T = 0, step0 = 0;
    const float* x = nullptr;       // [B][D]
    const float* y = nullptr;       // [B]
    double scale = 1.0;
    float prior_sd = 1.f;
    const float* tau = nullptr;     // host, [G]
    const uint64_t* offset = nullptr;  // host, [G]; null with eps
    uint64_t seed = 0;
    const float* eps = nullptr;     // [G][T][eps_count], null: Philox
    float *params = nullptr, *m = nullptr, *v = nullptr;  // [G][2 n_tot], in / out
    double lr = 1e-3, beta1 = 0.9, beta2 = 0.999, adam_eps = 1e-8;
    double* loss_out = nullptr;     // [G][T], nullable
    void* ws = nullptr;             // G * shape.ws_bytes
};
hipError_t launch_mfvi_fit(const MfviFit& r, hipStream_t st);
// predictive scores of the MFVI selection baselines (kernels_predict.hip): the
// mean-logit forward of a mean-field categorical plan over n_rows rows, rows
// [k rpd, (k + 1) rpd) on eps block k, and the scores read off its softmax
constexpr int kPredThreads = 256;
constexpr size_t kPredLds = 160 * 1024;
constexpr int kPredMaxGrid = 2048;  // workgroups (and statistics partials) of a launch
constexpr int kPredMaxRows = 64;    // rows of a group: its inputs, activations and logit sums in LDS
// bytes of a plan's scratch: the partials, then softplus(rho) in weight-space order
inline size_t predict_scratch_bytes(int n_tot) {
    return sizeof(double) * 2 * kPredMaxGrid + sizeof(float) * (size_t)n_tot;
}
struct PredictShape {
    int L = 0, S = 0, D = 0, C = 0, n_tot = 0, hs = 0, xs = 0;
    int RG = 0;          // rows per group
    int wcap = 0;        // floats of the W tile
    int ut[kMaxL] = {};  // output units per tile of every layer
    int64_t eps_count = 0;
};
// 0, or PSVI_EUNSUP when one unit's weights of some layer do not fit beside one row
int predict_shape(const psvi_plan& p, int64_t rpd, PredictShape& s);
struct PredictScores {
    PredictShape shape;
    int64_t n_rows = 0, rpd = 0;
    const float *x = nullptr, *eps = nullptr, *params = nullptr;
    const int32_t* z = nullptr;
    float *mean_logits = nullptr, *least_conf = nullptr, *entropy = nullptr, *el2n = nullptr,
          *correct = nullptr;
    float *last_acc = nullptr, *forgetting = nullptr, *never_learnt = nullptr;
    double* stats_out = nullptr;
};
hipError_t launch_predict_scores(const psvi_plan& p, const PredictScores& r, hipStream_t st);
// outer objective (kernels_outer.hip)
hipError_t launch_outer_stats(const psvi_plan& p, const float* params, const float* eps,
                              const float* x, double* stats, hipStream_t st);
hipError_t launch_outer_combine(const psvi_plan& p, int n_pseudo, const float* params,
                                const float* w, const float* nll, const double* stats,
                                double* loss, float* rowcoef, float* ck, float* sck,
                                float* grad_w, double* sample_out, int ablated,
                                hipStream_t st);
hipError_t launch_eval(const psvi_plan& p, int n_pseudo, const float* params, const float* w,
                       const int32_t* z, const float* nll, const double* stats,
                       const float* prob, int correction, float* W, float* probs_out,
                       double* out, hipStream_t st);
hipError_t launch_outer_gradw(const psvi_plan& p, int n_pseudo, const float* nll,
                              const float* rowcoef, float* grad_w, hipStream_t st);
hipError_t launch_outer_finish(const psvi_plan& p, int n_pseudo, const float* params,
                               const float* sck, float* grad, const float* du_part,
                               float* grad_u, hipStream_t st);
// out[m] = sum_s part[s][m] in sample order (one writer per element): the
// target gradients of the outer backward and of the R-op
hipError_t launch_sample_sum(int S, int n, const float* part, float* out, hipStream_t st);
// psvi_evaluate_regression: W = softmax_s(sampled_nkl_s) (correction 0: 1 / S),
// y_pred_j = sum_s W_s (f_sj y_std + y_mean); out[2] += sum_j (y_pred_j - y_j)^2,
// out[3] += sum_j log N(y_j; y_pred_j, 1 / sqrt(tau))
hipError_t launch_eval_regression(const psvi_plan& p, int n_pseudo, const float* params,
                                  const float* y, const double* stats, const float* f,
                                  int correction, float y_mean, float y_std, float* W,
                                  float* pred_out, double* out, hipStream_t st);
// LeNet (kernels_lenet.hip): scratch carve of the plan-owned buffer
struct LenetWs {
    float *wsamp, *dws, *p1, *x2, *h1, *h2, *d, *dh2, *dh1, *dx2, *part;
    int8_t *r1, *r2;
    int nchunk;
    float *g1, *part1;  // MFMA backward: routed d P1 [S][M][1176], conv1 partials [S][nch1][156]
    int nch1;
    size_t bytes;
};
int lenet_nchunk(const psvi_plan& p);
LenetWs lenet_ws(const psvi_plan& p, void* base);  // base nullptr: sizes only
// per-sample weight draw, forward, weighted NLL (+= nll_out), backward, and
// acc = [sum_s dW | sum_s dW eps] over the rank's samples (acc fully written)
// outer (psvi_outer_elbo_grad / psvi_evaluate): mode 1 forward only (per-row
// NLL, softmax of the data rows), mode 2 backward of the row coefficients with
// the pathwise sampled-KL term on the VILinear layers and d u of the pseudo rows
hipError_t launch_lenet(const psvi_plan& p, const float* u, const int32_t* z, const float* w,
                        const float* params, const float* eps, float* acc, double* nll_out,
                        void* ws, hipStream_t st, const NetOuter* outer = nullptr);
// LeNet HVP (kernels_lenet.hip): tangent scratch in the caller's workspace;
// the primal pass uses the plan-owned scratch
struct LenetTanWs {
    double* nll;
    float *acc, *wdot, *gd, *p1d, *x2d, *h1d, *h2d, *ld, *prob, *dh2d, *dh1d, *dx2d, *part, *du,
        *nlld;
    size_t bytes;
};
LenetTanWs lenet_tan_ws(const psvi_plan& p, void* base);
hipError_t launch_lenet_hvp(const psvi_plan& p, const float* u, const int32_t* z, const float* w,
                            const float* eps, const float* params, const float* vec, float* hv,
                            float* d_u, float* d_w, void* tws, hipStream_t st,
                            bool include_kl = true);
hipError_t launch_nonfinite(const void* x, int64_t n, int dtype, int32_t* flag, hipStream_t st);
// hyper_step's conjugate-gradient iteration (kernels_cg.hip)
size_t cg_ws_bytes();
hipError_t launch_cg_scale(int64_t n, const float* hv, double lr, float* out, hipStream_t st);
hipError_t launch_cg_pap(int64_t n, const float* hv1, const float* hv2, double lr, const double* p,
                         double* state, void* ws, hipStream_t st);
hipError_t launch_cg_residual(int64_t n, const float* hv1, const float* hv2, double lr, double* r,
                              double* state, double tol, void* ws, hipStream_t st);
hipError_t launch_cg_update(int64_t n, double* x, double* p, float* p32, const double* r,
                            const double* state, hipStream_t st);
// Hessian-vector products (kernels_rop.hip)
// row blocks per sample (G / G_dot slots): two workgroups per sample while the
// samples alone leave CUs idle
inline int rop_splits(const psvi_plan& p) { return (p.d.S < 256 && p.d.M > 1) ? 2 : 1; }
// the R-op's form choice, rows per chunk and LDS layouts (lds_shapes.cpp: host only)
RopGeometry rop_geometry(const psvi_plan& p);
struct NetRop {
    const float* u = nullptr;
    Targets targets;
    const float* w = nullptr;
    const float* x = nullptr;   // full-cov: the sample and its tangent
    const float* xd = nullptr;
    const float* params = nullptr;
    const float* vec = nullptr;
    const float* eps = nullptr;
    float* G = nullptr;
    float* Gd = nullptr;
    float* du = nullptr;        // nullable
    float* nlld = nullptr;      // nullable
    float* dzd = nullptr;       // nullable, Gaussian plans
    bool sum_slots = true;      // add the row blocks' G / G_dot slots into the first
};
hipError_t launch_net_rop(const psvi_plan& p, const NetRop& r, hipStream_t st);
struct HvpAssemble {
    const float* params = nullptr;
    const float* vec = nullptr;
    const float* eps = nullptr;
    const float* G = nullptr;
    const float* Gd = nullptr;
    const float* du = nullptr;
    const float* nlld = nullptr;
    float* hv = nullptr;
    float* d_u = nullptr;  // nullable
    float* d_w = nullptr;  // nullable
    bool include_kl = true;
    int64_t slot2 = 0;  // offset of the second G / G_dot slot (0: summed already)
};
hipError_t launch_hvp_assemble(const psvi_plan& p, const HvpAssemble& r, hipStream_t st);
}  // namespace psvi
