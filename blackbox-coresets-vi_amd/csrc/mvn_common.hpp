// mvn_common.hpp -- what more than one full-covariance unit uses
// (kernels_mvn_fwd / _update / _kstream / _stream.hip), one copy of each.
//
// Reference (/root/reference):
//   scale_tril  psvi/models/neural_net.py:452-461  L = diag(softplus(sd)) + corr
//               scattered row-major into the strict lower (n-1)x(n-1) block
//   rsample     neural_net.py:467-476  x_s = mean + L eps_s  (torch _batch_mv)
//   kl          neural_net.py:435-436  KL(N(mean, LL^T) || N(0, s0^2 I)); torch
//               evaluates it with an O(n^3) triangular solve, here it is the
//               exactly equal O(n^2) sum  n log s0 - sum log diag L
//               + (|L|_F^2 + |mean|^2) / (2 s0^2) - n/2
// Backward: G (S x n) = per-sample grads of x_s;
//   d mean = sum_s G_s + mean/s0^2,  dL = G^T eps (lower triangle only),
//   d sd = diag(dL) sigmoid(sd) + (sp/s0^2 - 1/sp) sigmoid(sd),
//   d corr = dL[tril] + corr/s0^2.
//
// L is never materialised: both GEMMs read the packed corr vector directly
// (row r starts at r(r-1)/2) and run on v_mfma_f32_32x32x2_f32 (exact fp32,
// gfx950 has no xf32).  The backward never writes dL to HBM: the Adam update
// of corr (p, m, v read + written once) is the GEMM epilogue.
#pragma once
#include "psvi_internal.hpp"

namespace psvi {

typedef float floatx16 __attribute__((ext_vector_type(16)));

struct MvnLayerArgs {
    int n;
    int64_t poff, eoff;
    int64_t tbase;  // tiled layout: first tile of the layer
};

// Tiled corr/m/v (world == 1 inner loops): tile (b, k <= b) of a layer holds
// rows [64b, 64b+64) x columns [64k, 64k+64) of L's strict lower part (0
// elsewhere) in the update MFMA's fragment order: wave w = 2 wr + wc, column
// group g, lane = 32 h + l32 hold the float4 of row 64b + 32 wr + l32, columns
// 64k + 32 wc + 8 g + 4 h .. +3, at ((w * 4 + g) * 64 + lane) * 4.  Every
// wave instruction of the update then moves 1 KB of contiguous memory.
__device__ __forceinline__ int64_t tile_index(const MvnLayerArgs& l, int b, int k) {
    return l.tbase + (int64_t)b * (b + 1) / 2 + k;
}

inline void fill_layers(const psvi_plan& p, MvnLayerArgs* la) {
    for (int l = 0; l < p.L; ++l) {
        la[l].n = p.lay[l].n;
        la[l].poff = p.lay[l].poff;
        la[l].eoff = p.lay[l].eoff;
        la[l].tbase = p.lay[l].tbase;
    }
}

// bf16 pieces (fp32-faithful products on v_mfma_f32_32x32x16_bf16): the
// cache policy of mvn_stream_bf2_kernel's tiled-state loads: read once per
// launch, so nt (2) -- the L2 keeps the eps planes, which every tile of a
// column re-reads.  C3 (tools/gpu_g25.sh): 180.8 -> 175.7 MB per launch
// (FETCH_SIZE x 2 + WRITE_SIZE), kernel time unchanged (38.3 us); sc1 nt (18)
// the same.  Other values: A/B builds only.
#ifndef PSVI_STATE_LOAD_AUX
#define PSVI_STATE_LOAD_AUX 2
#endif

// helpers of mvn_stream_bf2_kernel, mvn_fwd_seg_bf_kernel and the bf16 K-split update
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short bf8v __attribute__((ext_vector_type(8)));
typedef short s4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ floatx16 mfma6(const bf8v (&x)[3], const bf8v (&y)[3], floatx16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[2], y[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[1], y[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[0], y[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[1], y[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[0], y[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[0], y[0], c, 0, 0, 0);
    return c;
}
__device__ __forceinline__ bf8v cat44(s4v lo, s4v hi) {
    return bf8v{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// LDS images of a 128 x 64 bf16 block, 128-byte rows.  Column image (the
// transposed reads): 16-byte chunk c / 8 XORed with 4 on rows 2, 3 (mod 4), so
// a 32-lane half's four rows of one 64-byte run fall on four bank ranges.  Row
// image (x''s A operand, 8 columns per lane: c0 .. c0 + 3 and c0 + 8 .. c0 +
// 11 for c0 = 16 m + 4 h): each 16-column group stored in the order 0-3, 8-11,
// 4-7, 12-15, so a lane's 8 columns are one 16-byte chunk 2 m + h, and the
// chunk XORed with (s / 2) mod 8, so a ds_read_b128 lane group's 16 rows fall
// on 16 distinct (bank half, chunk) pairs.
// split3 on two entries at once: packed conversions (v_cvt_pk_bf16_f32) and
// packed subtractions; word p holds piece p of both entries (entry 0 low)
__device__ __forceinline__ void split3_pk(f32x2 x, uint32_t& w0, uint32_t& w1, uint32_t& w2) {
    typedef __bf16 bf2v __attribute__((ext_vector_type(2)));
    auto cvt = [](f32x2 v) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf2v)); };
    auto val = [](uint32_t w) { return f32x2{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)}; };
    w0 = cvt(x);
    const f32x2 r1 = x - val(w0);
    w1 = cvt(r1);
    w2 = cvt(r1 - val(w1));
}
// entries j, j + 1 of a fragment as fp32 (the pieces' values)
__device__ __forceinline__ f32x2 bf_pair(bf8v v, int j) {
    const uint32_t w = (uint32_t)(uint16_t)v[j] | ((uint32_t)(uint16_t)v[j + 1] << 16);
    return f32x2{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
}
constexpr int kBfImg = 128 * 128;  // bytes per plane image
__device__ __forceinline__ int img_col(int s, int c) {
    return s * 128 + (((c >> 3) ^ (((s >> 1) & 1) << 2)) << 4) + ((c & 7) << 1);
}
__device__ __forceinline__ int img_row(int s, int c) {
    // column c: group m = c / 16, quarter q = (c / 4) % 4 -> chunk 2 m + (q & 1),
    // half q >> 1 of the chunk
    const int q = (c >> 2) & 3;
    return s * 128 + ((((c >> 4) * 2 + (q & 1)) ^ ((s >> 1) & 7)) << 4) + ((q >> 1) << 3) + ((c & 3) << 1);
}

// Branch-free 16-byte loads.  gfx950 global loads need only 4-byte
// alignment, so a float4 may start at any float offset; the offset is clamped
// into the buffer [lo, hi) (hi - lo >= 4) so the load is unconditional (loads
// under divergent branches make the compiler's vmcnt bookkeeping fall back to
// vmcnt(0), which would drain every prefetch), and fix4 -- applied where the
// value is consumed -- shifts the clamped vector back, zeroing elements
// outside [lo, hi).  Offsets are 32-bit (the plan rejects larger buffers).
__device__ __forceinline__ int clamp4(int off, int lo, int hi) {
    return off < lo ? lo : (off > hi - 4 ? hi - 4 : off);
}
__device__ __forceinline__ float4 ld4u(const float* base, int off, int lo, int hi) {
    return *reinterpret_cast<const float4*>(base + clamp4(off, lo, hi));
}
__device__ __forceinline__ float4 fix4(float4 v, int off, int lo, int hi) {
    const int d = off - clamp4(off, lo, hi);
    if (d == 0) return v;  // VALU-only branch
    const float x[4] = {v.x, v.y, v.z, v.w};
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = i + d;
        r[i] = k == 0 ? x[0] : k == 1 ? x[1] : k == 2 ? x[2] : k == 3 ? x[3] : 0.f;
    }
    return make_float4(r[0], r[1], r[2], r[3]);
}
__device__ __forceinline__ float f4get(const float4& v, int i) {
    return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}

// diagnostics: slot k of the workgroup's 16 stamp slots (a.stamps nullptr in production)
#define MVN_STAMP(k, val)                                                          \
    do {                                                                           \
        if (a.stamps && threadIdx.x == 0) a.stamps[blockIdx.x * 16 + (k)] = (val); \
    } while (0)

// the update's tile geometry (the chunked and the K-split kernels)
constexpr int UB = 64;    // band rows = c-block columns
constexpr int USB = 128;  // samples staged per pass (K of the dL GEMM)
constexpr int ULD = 68;   // LDS row stride: 16-byte aligned rows for float4 stores
constexpr int TLD = 68;   // LDS stride of the transposed accumulator tile
// S <= 128: G resident (all samples), eps staged in halves of UEH samples
// (52 KB of LDS: three workgroups per CU); S > 128: both staged per pass.
constexpr int UEH = 64;
template <bool MULTI>
struct UpdShared {
    float Gs[USB * ULD];
    float Es[(MULTI ? USB : UEH) * ULD];
    float red[2 * 4 * 64];
};

// What every full-cov update kernel takes: UpdArgs, StrArgs and KsArgs derive
// from it and add only their own fields.
struct MvnUpdCommon {
    const float* eps;
    const float* g;  // g_shard [S][ldg]
    int ldg, S;
    int64_t g_total, e_total;  // floats in g_shard / eps (load guards)
    float *params, *m, *v;
    double* kl_out;  // nullable
    int include_kl;
    unsigned long long* stamps;  // diagnostics: 16 slots per workgroup (nullptr in production)
    float inv_s0sq, log_s0;
    AdamC adam;
    MvnLayerArgs lay[kMaxL];
};
// the packed-state kernels (chunked, K-split): the parameter count and gradient mode
struct MvnUpdGrad {
    int64_t pcount;       // parameter vector length
    float* grad_out;      // GRAD mode output (the HVP's J^T G_dot instead of Adam)
    const float* kl_vec;  // GRAD mode, nullable: + kl_vec / s0^2 on the corr entries (an HVP's direction)
};
// the tiled-state kernels (chunked TILED / FUSE, streaming): + the next draw, the partial x_next slots
struct MvnUpdTiled {
    float *tp, *tm, *tv;
    const float* eps_next;
    float* part;
};

inline void fill_update(const psvi_plan& p, const MvnUpdate& r, MvnUpdCommon& a) {
    a.eps = r.eps;
    a.g = r.g_shard;
    a.ldg = p.rows_tot[p.rank];
    a.S = p.d.S;
    a.g_total = (int64_t)p.d.S * p.rows_tot[p.rank];
    a.e_total = p.Peps;
    a.params = r.params;
    a.m = r.m;
    a.v = r.v;
    a.kl_out = r.kl_out;
    a.include_kl = r.include_kl;
    a.stamps = g_diag.upd_stamps;
    const float s0 = p.d.prior_sd;
    a.inv_s0sq = 1.f / (s0 * s0);
    a.log_s0 = logf(s0);
    if (r.hp) a.adam = make_adam(r.hp);
    fill_layers(p, a.lay);
}
inline void fill_grad(const psvi_plan& p, const MvnUpdate& r, MvnUpdGrad& a) {
    a.pcount = p.P;
    a.grad_out = r.grad_out;
    a.kl_vec = r.kl_vec;
}
inline void fill_tiled(const psvi_plan& p, const MvnUpdate& r, float* part, MvnUpdTiled& a) {
    if (r.tstate) {
        a.tp = r.tstate;
        a.tm = a.tp + p.tiles_total * 4096;
        a.tv = a.tm + p.tiles_total * 4096;
    }
    a.eps_next = r.next.eps;
    a.part = part;
}

// The diagonal head: a band row's mean / sd gradients from its sums over the
// samples, gm = sum_s G and gs = sum_s G eps (kl: + the KL's):
//   sp = softplus(sdr), sg = sigmoid(sdr)
//   gmean = gm (+ mu / s0^2),  gsd = gs sg (+ (sp / s0^2 - 1 / sp) sg)
__device__ __forceinline__ void diag_head(float mu, float sdr, float gm, float gs, bool kl, float inv_s0sq,
                                          float log_s0, float& sp, float& gmean, float& gsd, float& klp) {
    sp = softplus_f(sdr);
    const float sg = sigmoid_f(sdr);
    gmean = gm;
    gsd = gs * sg;
    if (kl) {
        gmean += mu * inv_s0sq;
        gsd += (sp * inv_s0sq - 1.f / sp) * sg;
        klp += log_s0 - logf(sp) + 0.5f * ((sp * sp + mu * mu) * inv_s0sq - 1.f);
    }
}
__device__ __forceinline__ void diag_grad(float mu, float sdr, float gm, float gs, bool kl,
                                          float inv_s0sq, float& sp, float& gmean, float& gsd) {
    float unused = 0.f;
    diag_head(mu, sdr, gm, gs, kl, inv_s0sq, 0.f, sp, gmean, gsd, unused);
}
__device__ __forceinline__ void diag_head(const MvnUpdCommon& a, float mu, float sdr, float gm,
                                          float gs, float& gmean, float& gsd, float& klp) {
    float sp;
    diag_head(mu, sdr, gm, gs, a.include_kl, a.inv_s0sq, a.log_s0, sp, gmean, gsd, klp);
}
// Adam on a band row's mean and sd entries, given their moments (registers, or
// the state in memory: read and written in place, the mean's before the sd's)
__device__ __forceinline__ void adam_diag(const AdamC& ad, float mu, float gmean, float& mm, float& mv,
                                          float sd, float gsd, float& sm, float& sv, float& mun,
                                          float& sdn) {
    float m_ = mm, v_ = mv;
    mun = adam_apply(ad, mu, gmean, m_, v_);
    mm = m_;
    mv = v_;
    m_ = sm;
    v_ = sv;
    sdn = adam_apply(ad, sd, gsd, m_, v_);
    sm = m_;
    sv = v_;
}

// The update accumulator D[i = c][j = r] (j = lane & 31, i = (q & 3) + 8 (q >> 2)
// + 4 h) of wave (wr, wc): float4 g (entries 4 g .. 4 g + 3) in the transposed
// tile T[r][c], and all four from x (the accumulators, or 16 floats in their order)
struct FragPos {
    int wr, wc, h, l32;
};
__device__ __forceinline__ float4& frag_T(float* T, const FragPos& f, int g) {
    return *reinterpret_cast<float4*>(&T[(32 * f.wr + f.l32) * TLD + 32 * f.wc + 8 * g + 4 * f.h]);
}
template <class X>
__device__ __forceinline__ void store_frag_T(float* T, const FragPos& f, const X& x) {
#pragma unroll
    for (int g = 0; g < 4; ++g) frag_T(T, f, g) = make_float4(x[4 * g], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3]);
}
// One row's float4 run of N packed arrays -- columns cb .. cb + 3 of row r at
// packed offset o: whole left of the diagonal, element by element (the strict
// lower part) on the run that crosses it
template <int N>
__device__ __forceinline__ void store_packed_run(float* const (&dst)[N], const float4 (&x)[N], int o,
                                                 int cb, int r) {
    if (cb + 3 < r) {
#pragma unroll
        for (int k = 0; k < N; ++k) *reinterpret_cast<float4*>(dst[k] + o) = x[k];
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (cb + i < r) {
#pragma unroll
                for (int k = 0; k < N; ++k) dst[k][o + i] = f4get(x[k], i);
            }
    }
}

// The route of one update request: the kernel, its form, and what follows it
// (mvn_route decides, launch_mvn_update switches: kernels_mvn_update.hip)
struct MvnRoute {
    enum Kernel { CHUNKED, STREAM_F32, STREAM_BF, KSPLIT } kernel;
    bool grad, fuse, tiled, pko;  // CHUNKED's template flags; grad: KSPLIT's too
    bool fold;                    // STREAM_BF: the band combine in the kernel
    bool bf;                      // KSPLIT: the dL GEMM on bf16 pieces
    int mode;                     // CHUNKED: samples per LDS pass (0: <= 64, 1: <= 128, 2: more)
    enum After { NONE, REDUCE_UFRB, REDUCE_SFRB, FWD } after;
};
// x_next = mean' + softplus(sd') eps_next + each row block's partial slots (kernels_mvn_fwd.hip)
hipError_t launch_next_reduce(const psvi_plan& p, const MvnUpdate& r, const FwdRowBlock* rbs,
                              int nrb, const float* part, hipStream_t st);
hipError_t launch_mvn_stream(const psvi_plan& p, const MvnUpdate& r, const MvnRoute& rt, hipStream_t st);
hipError_t launch_mvn_kstream(const psvi_plan& p, const MvnUpdate& r, const MvnRoute& rt, hipStream_t st);
constexpr int kFoldMax = 64;  // band ends per run the in-kernel combine can take (FOLD)

}  // namespace psvi
