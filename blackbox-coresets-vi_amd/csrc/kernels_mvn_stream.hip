// kernels_mvn_stream.hip -- the streaming fused update, on fp32 MFMAs and on
// bf16 pieces (see mvn_common.hpp).
#include "mvn_common.hpp"

namespace psvi {

// The inner loop's steady-state update (Adam, tiled corr/m/v state, world 1,
// S a multiple of 32 up to 128) fused with the next step's sample, as one
// persistent workgroup per CU walking a contiguous run of the layer-major,
// band-major tile list (band b: tiles k = 0 .. b, the diagonal last).
// Per 64x64 tile (l, b, k), wave (wr, wc) owns rows 64b + 32wr + [0, 32) x
// columns 64k + 32wc + [0, 32):
//   dL^T[c][r] = sum_s eps[s][c] G[s][r]      v_mfma_f32_32x32x2_f32, K = S;
//       A = eps (the tile's column block), B = G (the band's slice), both
//       from LDS with ds_read_b32 (the band's slice is staged once per band);
//   corr/m/v <- Adam on the accumulators (tiled state: the fragment order, 1 KB
//       per wave instruction); the new L entries stay in registers;
//   x'[s][r] += sum_c eps'[s][c] L'[r][c]     K = the wave's 32 columns:
//       B = L' straight from the registers (K permuted to the fragment
//       order), A = eps' from LDS, one ds_read_b128 per 4 MFMAs.
// x' accumulates in registers over the run's tiles of one band; at the band's
// end the two column-half waves add their partials through LDS and write the
// segment's slot ([S][64]); mvn_fwd_reduce_kernel adds a band's slots.
// Prefetch: tile i+1's corr/m/v and eps / eps' blocks are loaded behind tile
// i's x' GEMM (eps blocks into the other LDS buffer after it), the next
// band's G slice too.  LDS rows of the eps blocks are 16 float4 slots, slot
// c4 stored at c4 ^ (s & 15): the dL reads (one row, 32 columns) and the x'
// reads (16 rows, one float4 column) are both bank-conflict free.
// One barrier per tile (three at a band's end).
struct StrArgs : MvnUpdCommon, MvnUpdTiled {  // stamps: the DIAG builds only
    const StreamRange* ranges;
    int nb[kMaxL];         // bands per layer
    int xcol[kMaxL];
    // mvn_stream_bf2_kernel: the bf16 planes of eps / eps_next (EpsPlanes layout)
    const uint16_t* ep;
    const uint16_t* enp;
    int64_t pl;
    int64_t ppoff[kMaxL];
    int npad[kMaxL];
    // mvn_stream_bf2_kernel<FOLD>: the band combine in the kernel (the
    // stream's row-block table, one arrival counter per band, x' and its row
    // stride)
    const FwdRowBlock* rbs;
    int* bcnt;
    float* bms;  // per band: the new mean (64) and softplus(sd) (64)
    float* x;
    int ldx;
};

struct StrTile {
    int l, b, k, n, eoff, xc;
    int64_t tb, poff;
    int64_t pe;  // bf16 planes: element of (layer l, sample 0, column 64 k)
    int npad;    // bf16 planes: row length of layer l
};

__device__ __forceinline__ StrTile str_tile(const StrArgs& a, int l, int b, int k) {
    StrTile T;
    T.l = l;
    T.b = b;
    T.k = k;
    T.n = a.lay[l].n;
    T.eoff = (int)a.lay[l].eoff;
    T.xc = a.xcol[l];
    T.poff = a.lay[l].poff;
    T.tb = tile_index(a.lay[l], b, k) * 4096;
    T.pe = a.ppoff[l] + 64 * k;
    T.npad = a.npad[l];
    return T;
}

constexpr int kStrBuf = 128 * 16;  // float4 per eps block buffer ([128 samples][16 slots])
typedef float f32x4 __attribute__((ext_vector_type(4)));  // plain vector loads / stores (no memcpy)

// Adam with the variant fixed at compile time (adam_apply_fast's arithmetic)
// on two entries at once: the arithmetic as v_pk_mul_f32 /
// v_pk_fma_f32 / v_pk_add_f32 (two fp32 lanes per instruction on gfx950),
// the square root and reciprocal per entry
template <int KIND>
__device__ __forceinline__ f32x2 adam_fast_k2(const AdamC& a, f32x2 p, f32x2 g, f32x2& m, f32x2& v) {
    const f32x2 b1 = {a.b1, a.b1}, omb1 = {a.omb1, a.omb1}, b2 = {a.b2, a.b2}, omb2 = {a.omb2, a.omb2};
    m = __builtin_elementwise_fma(b1, m, omb1 * g);
    f32x2 d;
    if (KIND == PSVI_ADAM_HIGHER || KIND == PSVI_ADAM_TORCH) {
        v = __builtin_elementwise_fma(b2, v, (omb2 * g) * g);
        const f32x2 vv = KIND == PSVI_ADAM_HIGHER ? v + f32x2{1e-8f, 1e-8f} : v;
        const f32x2 sq = {__builtin_amdgcn_sqrtf(vv[0]), __builtin_amdgcn_sqrtf(vv[1])};
        d = __builtin_elementwise_fma(sq, f32x2{a.inv_sqrt_bc2, a.inv_sqrt_bc2}, f32x2{a.eps, a.eps});
        const f32x2 r = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
        return p - (f32x2{a.lr_bc1, a.lr_bc1} * m) * r;
    } else {
        v = __builtin_elementwise_fma(b2, v, (omb2 * g) * g) + f32x2{1e-12f, 1e-12f};
        const f32x2 vb = v * f32x2{a.inv_bc2, a.inv_bc2};
        d = f32x2{__builtin_amdgcn_sqrtf(vb[0]), __builtin_amdgcn_sqrtf(vb[1])} + f32x2{a.eps, a.eps};
        const f32x2 r = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
        return p - f32x2{a.lr, a.lr} * (m * f32x2{a.inv_bc1, a.inv_bc1}) * r;
    }
}

// NS = S / 32; KIND: Adam variant; DIAG: the diagnostics build (phase stamps);
// SC1: corr / m / v stores write-through with sc1, which drops the lines from
// the XCD's L2 (MI355X_MICROARCH.md, store flavours): the 60 MB of state written
// per launch then no longer evicts the eps / eps' blocks and G slices that
// later tiles re-read from L2 (false: plain stores, A/B)
template <int NS, int KIND, bool DIAG = false, bool SC1 = true, bool PAD = false>
__global__ __launch_bounds__(256, 1) void mvn_stream_kernel(StrArgs a) {
    constexpr int KT = 16 * NS;  // K steps of the dL GEMM (2 samples each)
    // [0, 4 kStrBuf): eps / eps' blocks, two buffers; then the band's G slice [128][64]
    __shared__ __attribute__((aligned(16))) f32x4 sm[4 * kStrBuf + 2048];
    f32x4* const Gl4 = sm + 4 * kStrBuf;
    const float* const Gl = reinterpret_cast<const float*>(Gl4);
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id();
    const int wr = wv >> 1, wc = wv & 1, h = lane >> 5, l32 = lane & 31;
    const StreamRange R = a.ranges[blockIdx.x];
    const int t0 = __builtin_amdgcn_readfirstlane(R.t0);
    const int t1 = __builtin_amdgcn_readfirstlane(R.t1);
    int slot = __builtin_amdgcn_readfirstlane(R.slot0);
    const int S = a.S;
    // diagnostics: shader clocks per phase summed over the run's tiles (thread 0)
    unsigned long long tph[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tlast = 0;
    auto ph = [&](int q) __attribute__((always_inline)) {
        if (DIAG && tid == 0) {
            const unsigned long long tt = __builtin_amdgcn_s_memtime();
            if (q >= 0) tph[q] += tt - tlast;
            tlast = tt;
        }
    };
    // PAD (psvi_inner_loop's own eps / G buffers, each followed by 64 zeroed
    // floats): the loads past a layer's last column block run into the pad,
    // so they need no clamp at the buffer's end and no fix-up at use
    const int e_hi = PAD ? 0x7fffffff : (int)a.e_total - 4;
    const int g_hi = PAD ? 0x7fffffff : (int)a.g_total - 4;
    constexpr int SMAX = 32 * NS - 1;  // the staged sample rows: f >> 4 <= 127 needs no clamp at NS = 4

    // eps / eps' block of a tile: 8 + 8 float4 per thread, registers then LDS
    f32x4 ereg[8], enreg[8];
    auto load_E = [&](const StrTile& T) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int f = tid + 256 * j, s = min(f >> 4, SMAX), c4 = f & 15;
            const int off = min(T.eoff + s * T.n + 64 * T.k + 4 * c4, e_hi);
            ereg[j] = *reinterpret_cast<const f32x4*>(a.eps + off);
            enreg[j] = *reinterpret_cast<const f32x4*>(a.eps_next + off);
        }
    };
    // the float4 clamped at the buffer's end holds columns shifted by d: move
    // them back (applied where the registers are consumed, after the loads land)
    auto fix_E = [&](const StrTile& T) __attribute__((always_inline)) {
        if constexpr (PAD) return;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int f = tid + 256 * j, s = min(f >> 4, SMAX), c4 = f & 15;
            const int o = T.eoff + s * T.n + 64 * T.k + 4 * c4, d = o - min(o, e_hi);
            if (d > 0) {  // VALU-only: the loads are already unconditional
                ereg[j] = f32x4{d < 4 ? ereg[j][min(d, 3)] : 0.f, d < 3 ? ereg[j][min(d + 1, 3)] : 0.f,
                                d < 2 ? ereg[j][min(d + 2, 3)] : 0.f, d < 1 ? ereg[j][3] : 0.f};
                enreg[j] = f32x4{d < 4 ? enreg[j][min(d, 3)] : 0.f, d < 3 ? enreg[j][min(d + 1, 3)] : 0.f,
                                 d < 2 ? enreg[j][min(d + 2, 3)] : 0.f, d < 1 ? enreg[j][3] : 0.f};
            }
        }
    };
    auto store_E = [&](int bi, const StrTile& T) __attribute__((always_inline)) {
        fix_E(T);
        f32x4* E = sm + 2 * bi * kStrBuf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int f = tid + 256 * j, s = f >> 4, c4 = f & 15;
            const int o = s * 16 + (c4 ^ (s & 15));
            E[o] = ereg[j];
            E[kStrBuf + o] = enreg[j];
        }
    };
    // the band's G slice [s][64 rows]: 8 float4 per thread
    f32x4 greg[8];
    auto load_G = [&](const StrTile& T) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int f = tid + 256 * j, s = min(f >> 4, SMAX), c4 = f & 15;
            greg[j] = *reinterpret_cast<const f32x4*>(
                a.g + min(s * a.ldg + T.xc + 64 * T.b + 4 * c4, g_hi));
        }
    };
    auto store_G = [&](const StrTile& T) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int f = tid + 256 * j, s = min(f >> 4, SMAX), c4 = f & 15;
            const int o = s * a.ldg + T.xc + 64 * T.b + 4 * c4, d = o - min(o, g_hi);
            f32x4 gv = greg[j];
            if (!PAD && d > 0)  // clamped at the buffer's end (see fix_E)
                gv = f32x4{d < 4 ? gv[min(d, 3)] : 0.f, d < 3 ? gv[min(d + 1, 3)] : 0.f,
                           d < 2 ? gv[min(d + 2, 3)] : 0.f, 0.f};
            Gl4[tid + 256 * j] = gv;
        }
    };
    f32x4 P[4], M4[4], V4[4];
    auto frag_off = [&](const StrTile& T, int g) __attribute__((always_inline)) {
        return T.tb + (int64_t)((wv * 4 + g) * 64 + lane) * 4;
    };
    // tm / tv follow tp in one allocation (tstate) of < 2 GB: one descriptor,
    // the m / v arrays at a scalar byte offset
    const rsrc_t rs_t = make_rsrc(a.tp, 0x7fffffff);
    const int tmb = __builtin_amdgcn_readfirstlane((int)((a.tm - a.tp) * 4));
    const int tvb = __builtin_amdgcn_readfirstlane((int)((a.tv - a.tp) * 4));
    auto load_pmv = [&](const StrTile& T) __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t o = frag_off(T, g);
            P[g] = *reinterpret_cast<const f32x4*>(a.tp + o);
            M4[g] = *reinterpret_cast<const f32x4*>(a.tm + o);
            V4[g] = *reinterpret_cast<const f32x4*>(a.tv + o);
        }
    };

    floatx16 xacc[NS];
#pragma unroll
    for (int sb = 0; sb < NS; ++sb)
#pragma unroll
        for (int q = 0; q < 16; ++q) xacc[sb][q] = 0.f;
    float klp = 0.f, kld = 0.f;  // sum corr^2 (scaled at the end), diagonal KL terms
    f32x2 kl2 = {0.f, 0.f};      // sum corr^2, two lanes (packed with the Adam arithmetic)

    // per-lane LDS offsets of the XOR-swizzled reads
    int okd[8];  // dL A operand (floats): row s = 2t + h, column 32wc + l32; index t & 7
    {
        const int c = 32 * wc + l32, c4 = c >> 2;
#pragma unroll
        for (int k = 0; k < 8; ++k) okd[k] = h * 64 + 4 * ((c4 ^ h) ^ (2 * k)) + (c & 3);
    }
    int okx[4];  // x' A operand (float4): row l32 (+ 32 sb), slot 8wc + 2g + h
#pragma unroll
    for (int g = 0; g < 4; ++g) okx[g] = l32 * 16 + ((8 * wc + 2 * g + h) ^ (l32 & 15));
    const int ogb = h * 64 + 32 * wr + l32;  // G[2t + h][32wr + l32] at ogb + 128 t

    if (DIAG && tid == 0) {
        a.stamps[(size_t)blockIdx.x * 16 + 12] = __builtin_amdgcn_s_memtime();
        a.stamps[(size_t)blockIdx.x * 16 + 13] = __builtin_amdgcn_s_memrealtime();
    }
    // prologue: tile t0
    // tile (l, b, k) of t0, then walked in list order with scalar arithmetic
    int tl = __builtin_amdgcn_readfirstlane(R.lbk0 >> 28);
    int tb_ = __builtin_amdgcn_readfirstlane((R.lbk0 >> 14) & 0x3fff);
    int tk = __builtin_amdgcn_readfirstlane(R.lbk0 & 0x3fff);
    StrTile cur = str_tile(a, tl, tb_, tk);
    load_E(cur);
    load_G(cur);
    store_E(0, cur);
    store_G(cur);
    __syncthreads();

    // one tile; HAS_NEXT / NEWBAND compile-time so that every load is unconditional
    auto tile = [&](int i, const StrTile& nxt, auto has_next_c, auto newband_c) __attribute__((always_inline)) {
        constexpr bool has_next = decltype(has_next_c)::value;
        constexpr bool newband = decltype(newband_c)::value;
        const int bi = (i - t0) & 1;
        ph(-1);
        const float* Ef = reinterpret_cast<const float*>(sm + 2 * bi * kStrBuf);
        const f32x4* En = sm + (2 * bi + 1) * kStrBuf;
        // ---- this tile's corr/m/v: in flight behind the dL GEMM
        load_pmv(cur);
        // ---- dL^T = eps^T G over the samples
        floatx16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
        for (int t = 0; t < KT; ++t)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ef[okd[t & 7] + 128 * t], Gl[ogb + 128 * t],
                                                       acc, 0, 0, 0);
        ph(0);
        const int n = cur.n, r = 64 * cur.b + 32 * wr + l32;
        // ---- diagonal tile: sum_s G and sum_s G eps of the band's rows -> mean / sd
        if (cur.k == cur.b && wc == 0) {
            // row c of the band per lane pair; the sums run in the chunked
            // kernel's order (four partials over sample groups 16w + [0, 16)
            // (+ 64), added left to right), so both kernels agree bit for bit
            const int c = 32 * wr + l32;
            float pm2[2], ps2[2];
#pragma unroll
            for (int ww = 0; ww < 2; ++ww) {
                const int w = 2 * h + ww;
                float gm = 0.f, gsum = 0.f;
#pragma unroll
                for (int hh = 0; hh < (NS > 2 ? 2 : 1); ++hh)
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int sm_ = hh * 64 + 16 * w + j;
                        if (sm_ < 32 * NS) {
                            const float gv = Gl[sm_ * 64 + c];
                            gm += gv;
                            gsum = fmaf(gv, Ef[sm_ * 64 + 4 * ((c >> 2) ^ (sm_ & 15)) + (c & 3)],
                                        gsum);
                        }
                    }
                pm2[ww] = gm;
                ps2[ww] = gsum;
            }
            const float m2 = __shfl_xor(pm2[0], 32, kWave), m3 = __shfl_xor(pm2[1], 32, kWave);
            const float s2 = __shfl_xor(ps2[0], 32, kWave), s3 = __shfl_xor(ps2[1], 32, kWave);
            const float dgm = ((pm2[0] + pm2[1]) + m2) + m3;
            const float dgs = ((ps2[0] + ps2[1]) + s2) + s3;
            if (h == 0 && r < n) {
                const int pm = (int)cur.poff + r, ps = pm + n;
                const float mu = a.params[pm], sdr = a.params[ps];
                float gmean, gsd;
                diag_head(a, mu, sdr, dgm, dgs, gmean, gsd, kld);
                adam_diag(a.adam, mu, gmean, a.m[pm], a.v[pm], sdr, gsd, a.m[ps], a.v[ps], a.params[pm],
                          a.params[ps]);
            }
        }
        ph(1);
        // ---- per column group g: Adam on the accumulators (fragment order =
        // tiled order), the stores, then g's share of the x' GEMM with the next
        // tile's loads spread between its MFMAs (a burst of them stalls the
        // in-order wave on the memory queue)
        const bool rv = r >= 1 && r <= n - 2;
        const float kls = a.include_kl ? a.inv_s0sq : 0.f;
        float Lf[16];
        auto issue_load = [&](int q) __attribute__((always_inline)) {
            // q < 16: the next tile's eps blocks (8 + 8); then (NEWBAND) the
            // next band's G slice (8)
            if constexpr (has_next) {
                if (q < 16) {
                    const int j = q >> 1;
                    const int f = tid + 256 * j, s = min(f >> 4, SMAX), c4 = f & 15;
                    const int off = min(nxt.eoff + s * nxt.n + 64 * nxt.k + 4 * c4, e_hi);
                    if ((q & 1) == 0) ereg[j] = *reinterpret_cast<const f32x4*>(a.eps + off);
                    else enreg[j] = *reinterpret_cast<const f32x4*>(a.eps_next + off);
                } else if constexpr (newband) {
                    const int j = q - 16;
                    const int f = tid + 256 * j, s = min(f >> 4, SMAX), c4 = f & 15;
                    greg[j] = *reinterpret_cast<const f32x4*>(
                        a.g + min(s * a.ldg + nxt.xc + 64 * nxt.b + 4 * c4, g_hi));
                }
            }
        };
        constexpr int NLOAD = has_next ? (newband ? 24 : 16) : 0;
        f32x4 avn = En[okx[0]];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int cb = 64 * cur.k + 32 * wc + 8 * g + 4 * h;
            float pn[4], mn[4], vn[4];
            // two entries per packed instruction (entries e, e + 1)
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
                const f32x2 p = {P[g][e], P[g][e + 1]};
                kl2 = __builtin_elementwise_fma(p, p, kl2);
                const f32x2 gv = __builtin_elementwise_fma(p, f32x2{kls, kls},
                                                           f32x2{acc[4 * g + e], acc[4 * g + e + 1]});
                const f32x2 gm = {rv && cb + e < r ? gv[0] : 0.f, rv && cb + e + 1 < r ? gv[1] : 0.f};
                f32x2 mm = {M4[g][e], M4[g][e + 1]}, vv = {V4[g][e], V4[g][e + 1]};
                const f32x2 pv = adam_fast_k2<KIND>(a.adam, p, gm, mm, vv);
                pn[e] = pv[0];
                pn[e + 1] = pv[1];
                mn[e] = mm[0];
                mn[e + 1] = mm[1];
                vn[e] = vv[0];
                vn[e + 1] = vv[1];
                Lf[4 * g + e] = pn[e];
                Lf[4 * g + e + 1] = pn[e + 1];
            }
            const int64_t o = frag_off(cur, g);
            if constexpr (SC1) {
                const uint32_t ob = (uint32_t)(o * 4);
                BSTORE128(
                    __builtin_bit_cast(u32x4, f32x4{pn[0], pn[1], pn[2], pn[3]}), rs_t, ob, 0, 16);
                BSTORE128(
                    __builtin_bit_cast(u32x4, f32x4{mn[0], mn[1], mn[2], mn[3]}), rs_t, ob, tmb, 16);
                BSTORE128(
                    __builtin_bit_cast(u32x4, f32x4{vn[0], vn[1], vn[2], vn[3]}), rs_t, ob, tvb, 16);
            } else {
                *reinterpret_cast<f32x4*>(a.tp + o) = f32x4{pn[0], pn[1], pn[2], pn[3]};
                *reinterpret_cast<f32x4*>(a.tm + o) = f32x4{mn[0], mn[1], mn[2], mn[3]};
                *reinterpret_cast<f32x4*>(a.tv + o) = f32x4{vn[0], vn[1], vn[2], vn[3]};
            }
            // x' += eps' L'^T over this group's 8 columns, all sample blocks; the
            // A fragments are read one slot ahead, and each slot is pinned
            // (sched_barrier) so the loads stay spread between the MFMAs
#pragma unroll
            for (int sb = 0; sb < NS; ++sb) {
                const int k = g * NS + sb;
                const f32x4 av = avn;
                if (k + 1 < 4 * NS) avn = En[okx[(k + 1) / NS] + 512 * ((k + 1) % NS)];
                xacc[sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], Lf[4 * g + 0], xacc[sb], 0, 0, 0);
                xacc[sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], Lf[4 * g + 1], xacc[sb], 0, 0, 0);
                xacc[sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], Lf[4 * g + 2], xacc[sb], 0, 0, 0);
                xacc[sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], Lf[4 * g + 3], xacc[sb], 0, 0, 0);
                // this slot's share of the next tile's loads (slot k of 4 NS)
                constexpr int NSLOT = 4 * NS;
#pragma unroll
                for (int q = 0; q < NLOAD; ++q)
                    if ((q * NSLOT) / (NLOAD > 0 ? NLOAD : 1) == k) issue_load(q);
                __builtin_amdgcn_sched_barrier(0x6);  // VALU / SALU may cross, memory and MFMA may not
            }
        }
        ph(2);
        ph(3);
        ph(4);
        if constexpr (has_next) store_E(bi ^ 1, nxt);
        ph(5);
        // ---- band end (or run end): the two column halves' x' partials -> the slot
        if constexpr (!has_next || newband) {
            __syncthreads();  // every wave done reading buffer bi and the G slice
            float* X = reinterpret_cast<float*>(sm + 2 * bi * kStrBuf);
            if (wc == 1) {
#pragma unroll
                for (int sb = 0; sb < NS; ++sb)
#pragma unroll
                    for (int q = 0; q < 16; ++q) X[((wr * NS + sb) * 16 + q) * 64 + lane] = xacc[sb][q];
            }
            if constexpr (newband) store_G(nxt);
            __syncthreads();
            if (wc == 0) {
                float* dst = a.part + (size_t)slot * S * 64 + 32 * wr + l32;
#pragma unroll
                for (int sb = 0; sb < NS; ++sb)
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int s = 32 * sb + (q & 3) + 8 * (q >> 2) + 4 * h;
                        dst[(size_t)s * 64] = xacc[sb][q] + X[((wr * NS + sb) * 16 + q) * 64 + lane];
                    }
            }
#pragma unroll
            for (int sb = 0; sb < NS; ++sb)
#pragma unroll
                for (int q = 0; q < 16; ++q) xacc[sb][q] = 0.f;
            ++slot;
        }
        ph(6);
        __syncthreads();  // buffer bi ^ 1 complete; buffer bi free
        ph(7);
        if (DIAG && tid == 0) ++tph[9];
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    for (int i = t0; i + 1 < t1; ++i) {
        if (++tk > tb_) {
            tk = 0;
            int nbl = a.nb[0];  // select: a dynamic index into the argument copies it to scratch
#pragma unroll
            for (int l = 1; l < kMaxL; ++l)
                if (tl == l) nbl = a.nb[l];
            if (++tb_ == nbl) {
                tb_ = 0;
                ++tl;
            }
        }
        const StrTile nxt = str_tile(a, tl, tb_, tk);
        if (nxt.l != cur.l || nxt.b != cur.b)
            tile(i, nxt, T_{}, T_{});
        else
            tile(i, nxt, T_{}, F_{});
        cur = nxt;
    }
    tile(t1 - 1, cur, F_{}, F_{});
    if (DIAG && tid == 0) {
        unsigned long long* o = a.stamps + (size_t)blockIdx.x * 16;
#pragma unroll
        for (int q = 0; q < 10; ++q) o[q] = tph[q];
        o[10] = __builtin_amdgcn_s_memtime();
        o[11] = __builtin_amdgcn_s_memrealtime();
    }
    klp = (klp + (kl2[0] + kl2[1])) * (0.5f * a.inv_s0sq) + kld;
    if (a.kl_out && a.include_kl) {
        const float tot = block_sum(klp, reinterpret_cast<float*>(sm));
        if (tid == 0) atomicAdd(a.kl_out, (double)tot);
    }
}


// ---------------------------------------------------------------------------
// The bf16-piece streaming update: mvn_stream_kernel's tile walk with both
// products on the bf16 matrix cores, fp32-faithful.  Every operand is split into three bf16
// pieces (split3: exact) and each product is the six piece products that
// matter (the dropped ones are below 2^-26 of the product, under fp32's own
// rounding); the matrix cores accumulate in fp32.  v_mfma_f32_32x32x16_bf16
// does 16 K per 32 cycles against v_mfma_f32_32x32x2_f32's 2 per 64, so the
// six products take 3/8 of the fp32 MFMA time, and the vector unit keeps
// issuing beside a bf16 MFMA (it holds the SIMD for 8 of its 32 cycles;
// MI355X_MICROARCH.md, cycle constants), where the fp32 form serialises
// with the Adam epilogue.
//   eps  (dL's A operand, K = samples): the draw's planes staged into an
//        LDS image [s][64 columns] per plane, read column-wise with
//        ds_read_b64_tr_b16;
//   G    (dL's B operand): the band's slice split once per band into a
//        second column image;
//   eps' (x''s A operand, K = columns): the next draw's planes in a row image;
//   L'   (x''s B operand): the new corr entries, split in the accumulators'
//        registers (the accumulator-as-operand order of the 32x32x16 form).
// Tiled state, slots, the diagonal's mean / sd and the KL as mvn_stream_kernel.
//
// mvn_stream_bf2_kernel: that tile walk with two waves per SIMD (the round-5
// four-wave form, one wave per SIMD, ran 37.6 us against 33.8 at C3).  Eight
// waves per workgroup: wave (q, hk) with quadrant q = wv & 3 -- rows 32 wr,
// columns 32 wc of the 64 x 64 tile, (wr, wc) = (q >> 1, q & 1) -- and sample
// half hk = wv >> 2 (samples 64 hk .. 64 hk + 63).  The two waves of a
// quadrant sit on one SIMD (waves w and w + 4), so one's vector work, LDS
// waits and stores run beside the other's MFMAs:
//   dL: each wave its samples' half of K (4 K-steps), the halves exchanged
//       through LDS -- each wave gets the partner's partial of its own two
//       column groups g = 2 hk, 2 hk + 1 and adds it (hk 0's + hk 1's, the
//       same sum in both orders);
//   Adam: each wave its two groups (corr / m / v fragments loaded, stored),
//       and their L' pieces -- K-half st = hk of x''s B operand -- swapped
//       with the partner through LDS;
//   x': each wave its samples' two 32-row blocks over both K-halves (x'
//       accumulators: 32 registers per wave);
//   band end: the wc = 1 waves' x' partials added by the wc = 0 waves (per
//       sample half) and written to the segment's slot, as before.
// The exchanges use the eps column image after the dL reads (16 + 24 KB); the
// next tile's eps planes are stored after them.  Images, pieces, swizzles and
// the slot layout as described above.  DIAG: per-phase shader clocks summed
// over the run's tiles (thread 0) into the stamp buffer (tools/bf_stamps.py).
//
// FOLD: the band's x' rows are finished in the kernel instead of by
// mvn_fwd_reduce_kernel.  At a band's end each segment stores its slot
// write-through (sc1), drains (vmcnt 0), and one lane adds to the band's
// counter (relaxed, agent scope); the segment that draws the last ticket
// reads the band's slots with sc1 loads and writes x' = mean + softplus(sd)
// eps' + the slots' sum, in the reduce's order (slot k into partial k mod 4),
// so the result is the reduce's bit for bit.  The band's new mean / sd come
// from its diagonal tile, the band's last: stored write-through by that
// segment before its own drain and ticket, read with agent-scope loads.  The
// hand-off is the K-split update's (MI355X_MICROARCH.md hand-off table, first
// row); no workgroup waits on another.
template <int KIND, bool DIAG = false, bool FOLD = false>
__global__ __launch_bounds__(512, 1) void mvn_stream_bf2_kernel(StrArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t smb[9 * kBfImg];
    uint8_t* const Eb = smb;
    uint8_t* const Gb = smb + 3 * kBfImg;
    uint8_t* const En = smb + 6 * kBfImg;
    float* const Xs = reinterpret_cast<float*>(En);
    float* const Xd = reinterpret_cast<float*>(Eb);                  // dL partials: 8 waves x 8 x 64 (16 KB)
    uint32_t* const Xl = reinterpret_cast<uint32_t*>(Eb + 16384);    // L' pieces: 8 waves x 12 x 64 (24 KB)
    float* const Xg = reinterpret_cast<float*>(Eb + 40960);          // diagonal sums: 8 waves x 2 x 64 (4 KB)
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id();
    const int q = wv & 3, hk = wv >> 2, wr = q >> 1, wc = q & 1, h = lane >> 5, l32 = lane & 31;
    const int pw = wv ^ 4;  // the partner wave (same quadrant, other sample half)
    const StreamRange R = a.ranges[blockIdx.x];
    const int t0 = __builtin_amdgcn_readfirstlane(R.t0);
    const int t1 = __builtin_amdgcn_readfirstlane(R.t1);
    int slot = __builtin_amdgcn_readfirstlane(R.slot0);
    const int S = a.S;  // 128
    unsigned long long tph[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tlast = 0;
    // (wave 0 as a whole: the stamps stay wave-uniform, in scalar registers)
    if (DIAG && tid == 0) a.stamps[(size_t)blockIdx.x * 16 + 13] = __builtin_amdgcn_s_memtime();
    auto ph = [&](int qq) __attribute__((always_inline)) {
        if (DIAG && wv == 0) {
            const unsigned long long tt = __builtin_amdgcn_s_memtime();
            if (qq >= 0) tph[qq] += tt - tlast;
            tlast = tt;
        }
    };

    // ---- staging: 6 chunks of 16 bytes per thread: chunk j = plane j >> 1, row
    // (tid >> 3) + 64 (j & 1), chunk tid % 8 of the tile's 64 columns
    u32x4 stg[6];
    const int srow0 = tid >> 3, ch = tid & 7;
    const int st_col = srow0 * 128 + ((ch ^ (((srow0 >> 1) & 1) << 2)) << 4);
    const int st_row0 = img_row(srow0, 8 * ch), st_row1 = img_row(srow0, 8 * ch + 4);
    auto store_col = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 6; ++j)
            *reinterpret_cast<u32x4*>(Eb + st_col + (j >> 1) * kBfImg + 8192 * (j & 1)) = stg[j];
    };
    auto store_row = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            uint8_t* img = En + (j >> 1) * kBfImg + 8192 * (j & 1);
            *reinterpret_cast<u32x2*>(img + st_row0) = u32x2{stg[j][0], stg[j][1]};
            *reinterpret_cast<u32x2*>(img + st_row1) = u32x2{stg[j][2], stg[j][3]};
        }
    };
    // ---- the band's G slice [128 samples][64 rows]: 4 float4 per thread
    f32x4 greg[4];
    auto split_G = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int f = tid + 512 * j, s = f >> 4, c4 = f & 15;
            uint32_t x[3][2];
            split3_pk(f32x2{greg[j][0], greg[j][1]}, x[0][0], x[1][0], x[2][0]);
            split3_pk(f32x2{greg[j][2], greg[j][3]}, x[0][1], x[1][1], x[2][1]);
#pragma unroll
            for (int p = 0; p < 3; ++p)
                *reinterpret_cast<u32x2*>(Gb + p * kBfImg + img_col(s, 4 * c4)) = u32x2{x[p][0], x[p][1]};
        }
    };
    // this wave's two fragment groups g = 2 hk + gi of its quadrant (tiled order)
    f32x4 P[2], M4[2], V4[2];
    const rsrc_t rs_t = make_rsrc(a.tp, 0x7fffffff);
    const rsrc_t rs_e = make_rsrc(a.ep, 0x7fffffff), rs_en = make_rsrc(a.enp, 0x7fffffff);
    const rsrc_t rs_g = make_rsrc(a.g, 0x7fffffff);
    const int tmb = __builtin_amdgcn_readfirstlane((int)((a.tm - a.tp) * 4));
    const int tvb = __builtin_amdgcn_readfirstlane((int)((a.tv - a.tp) * 4));
    const uint32_t vo_f = (uint32_t)(((q * 4 + 2 * hk) * 64 + lane) * 16);  // + 1024 gi
    const uint32_t vo_g = (uint32_t)(4 * ((tid >> 4) * a.ldg + 4 * (tid & 15)));  // G rows tid / 16 (+ 32 j)
    auto vo_planes = [&](const StrTile& T) __attribute__((always_inline)) {
        return (uint32_t)(2 * (srow0 * T.npad + 8 * ch));
    };
    auto so_planes = [&](const StrTile& T, int j) __attribute__((always_inline)) {
        return __builtin_amdgcn_readfirstlane((int)(2 * (T.pe + (j >> 1) * a.pl + (int64_t)(64 * (j & 1)) * T.npad)));
    };
    auto ldb = [&](rsrc_t r, uint32_t vo, int so) __attribute__((always_inline)) {
        return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, vo, so, 0));
    };
    auto load_G = [&](const StrTile& T, int j) __attribute__((always_inline)) {
        const int so = __builtin_amdgcn_readfirstlane(4 * (32 * j * a.ldg + T.xc + 64 * T.b));
        greg[j] = __builtin_bit_cast(f32x4, ldb(rs_g, vo_g, so));
    };
    floatx16 xacc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int qq = 0; qq < 16; ++qq) xacc[j][qq] = 0.f;
    float kld = 0.f;
    f32x2 kl2 = {0.f, 0.f};
    const int g16 = lane >> 4, qq4 = (lane >> 2) & 3, pp = lane & 3;
    const int ca = 32 * wc + 16 * (g16 & 1) + 4 * pp;  // eps column (dL's A)
    const int cg = 32 * wr + 16 * (g16 & 1) + 4 * pp;  // G column (dL's B)
    const uint8_t* const rda = Eb + img_col(8 * h + qq4, ca);
    const uint8_t* const rdb = Gb + img_col(8 * h + qq4, cg);
    const int xsw = (l32 >> 1) & 7;

    int tl = __builtin_amdgcn_readfirstlane(R.lbk0 >> 28);
    int tb_ = __builtin_amdgcn_readfirstlane((R.lbk0 >> 14) & 0x3fff);
    int tk = __builtin_amdgcn_readfirstlane(R.lbk0 & 0x3fff);
    StrTile cur = str_tile(a, tl, tb_, tk);
    {
        const uint32_t vo = vo_planes(cur);
#pragma unroll
        for (int j = 0; j < 4; ++j) load_G(cur, j);
#pragma unroll
        for (int j = 0; j < 6; ++j) stg[j] = ldb(rs_e, vo, so_planes(cur, j));
        store_col();
#pragma unroll
        for (int j = 0; j < 6; ++j) stg[j] = ldb(rs_en, vo, so_planes(cur, j));
        store_row();
        split_G();
    }
    __syncthreads();

    // phase A's loads: 0..5 this tile's corr / m / v fragments (2 groups x 3),
    // 6..11 the next tile's eps planes
    auto issue_a = [&](int qi, const StrTile& nxt, bool has_next, uint32_t vo_n) __attribute__((always_inline)) {
        if (qi < 6) {
            const int gi = qi / 3, which = qi % 3;
            const int so = __builtin_amdgcn_readfirstlane((int)(cur.tb * 4));
            const u32x4 x = __builtin_bit_cast(
                u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_t, vo_f + 1024 * gi,
                                                             which == 0 ? so : which == 1 ? so + tmb : so + tvb,
                                                             PSVI_STATE_LOAD_AUX));
            if (which == 0) P[gi] = __builtin_bit_cast(f32x4, x);
            else if (which == 1) M4[gi] = __builtin_bit_cast(f32x4, x);
            else V4[gi] = __builtin_bit_cast(f32x4, x);
        } else if (has_next) {
            stg[qi - 6] = ldb(rs_e, vo_n, so_planes(nxt, qi - 6));
        }
    };
    // phase B's loads: 0..5 the next tile's eps' planes, 6..9 the next band's G
    auto issue_b = [&](int qi, const StrTile& nxt, bool has_next, bool newband, uint32_t vo_n) __attribute__((always_inline)) {
        if (qi < 6) {
            if (has_next) stg[qi] = ldb(rs_en, vo_n, so_planes(nxt, qi));
        } else if (newband) {
            load_G(nxt, qi - 6);
        }
    };

    // the band's index in the stream's row-block table (layer-major)
    auto band_id = [&](const StrTile& T) __attribute__((always_inline)) {
        int bid = T.b;
#pragma unroll
        for (int l = 0; l < kMaxL - 1; ++l)
            if (l < T.l) bid += a.nb[l];
        return __builtin_amdgcn_readfirstlane(bid);
    };
    // FOLD: the band's arrival after its slot is stored; the last arriver
    // notes the band and finishes its x' rows after the walk, where the tile
    // walk's prefetch registers are free (see above)
    __shared__ int fold_list[kFoldMax];
    int nfold = 0;
    auto band_arrive = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's slot (and mean / sd) stores
        __syncthreads();                                 // ... and every other wave's
        const int bid = band_id(cur);
        const int nk = __builtin_amdgcn_readfirstlane(a.rbs[bid].nk);
        if (nk > 1) {
            if (tid == 0)
                Xs[0] = __int_as_float(
                    __hip_atomic_fetch_add(a.bcnt + bid, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            __syncthreads();
            const int old = __builtin_amdgcn_readfirstlane(__float_as_int(Xs[0]));
            if (old != nk - 1) return;  // uniform: another segment finishes the band
            if (tid == 0) __hip_atomic_store(a.bcnt + bid, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (tid == 0) fold_list[nfold] = bid;  // read after the walk's later barriers
        ++nfold;
    };
    // x' rows of band bid from its slots (fragment order, see the band end):
    // thread t takes float4 f = t + 512 m (m = 0..3) of every slot -- row 32
    // (m >> 1) + (t & 31) of the band, samples 64 (m & 1) + 32 j + 4 h + 8 qg +
    // e (e = 0..3) with (j, qg) = ((t >> 8) & 1, (t >> 6) & 3), h = (t >> 5) & 1.
    // Runs after the walk, where the walk's registers are free: mean / sd, eps'
    // and the first four slots' loads in flight together.
    auto band_combine = [&](int bid) __attribute__((always_inline)) {
        const FwdRowBlock rb = a.rbs[bid];
        const int nk = __builtin_amdgcn_readfirstlane(rb.nk), slot0 = __builtin_amdgcn_readfirstlane(rb.slot0);
        const int R = __builtin_amdgcn_readfirstlane(rb.R), xcol = __builtin_amdgcn_readfirstlane(rb.xcol);
        const int l = __builtin_amdgcn_readfirstlane(rb.layer), r0 = __builtin_amdgcn_readfirstlane(rb.r0);
        const int n = a.lay[l].n;
        const float* const bm = a.bms + 128 * (int64_t)bid;
        const int lt = tid & 31, hh = (tid >> 5) & 1, qg = (tid >> 6) & 3, jj = (tid >> 8) & 1;
        // rows rr[w] = 32 w + lt (w = m >> 1): the band's new mean and softplus(sd)
        float mu[2], dg[2], ev[4][4];
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            mu[w] = __hip_atomic_load(bm + 32 * w + lt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            dg[w] = __hip_atomic_load(bm + 64 + 32 * w + lt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        auto smp = [&](int m, int e) { return 64 * (m & 1) + 32 * jj + 4 * hh + 8 * qg + e; };
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float* ec = a.eps_next + a.lay[l].eoff + r0 + min(32 * (m >> 1) + lt, R - 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) ev[m][e] = ec[(int64_t)smp(m, e) * n];
        }
        const rsrc_t rs_p = make_rsrc(a.part, 0x7fffffff);
        f32x4 A[4][4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) A[m][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        // slot k into partial k mod 4, in slot order (mvn_fwd_reduce_kernel's
        // sum); eight slots' loads in flight per round (the walk's registers
        // are free here): a round trip of sc1 loads is the combine's cost
        // (four in the stamps build, whose stamp registers would spill)
        constexpr int KR = DIAG ? 4 : 8;
        for (int k0 = 0; k0 < nk; k0 += KR) {  // uniform
            f32x4 v[4][KR];
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                const int so = __builtin_amdgcn_readfirstlane((slot0 + min(k0 + i, nk - 1)) * S * 64 * 4);
                if (k0 + i < nk || i == 0) {  // uniform
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        v[m][i] = __builtin_bit_cast(
                            f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_p, (uint32_t)((tid + 512 * m) * 16), so, 16));
                }
            }
#pragma unroll
            for (int i = 0; i < KR; ++i)
                if (k0 + i < nk)  // uniform
#pragma unroll
                    for (int m = 0; m < 4; ++m) A[m][i & 3] += v[m][i];
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const f32x4 t = (A[m][0] + A[m][1]) + (A[m][2] + A[m][3]);
            const int rr = 32 * (m >> 1) + lt;
            if (rr < R) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    a.x[(int64_t)smp(m, e) * a.ldx + xcol + rr] =
                        (mu[m >> 1] + mul_unfused(dg[m >> 1], ev[m][e])) + t[e];  // mvn_fwd_reduce_kernel's rounding
            }
        }
    };

    auto tile = [&](const StrTile& nxt, auto has_next_c, auto newband_c) __attribute__((always_inline)) {
        constexpr bool has_next = decltype(has_next_c)::value;
        constexpr bool newband = decltype(newband_c)::value;
        ph(-1);
        const bool diag = cur.k == cur.b && wc == wr;  // wave-uniform
        const uint32_t vo_n = vo_planes(nxt);
        // ---- phase A: this wave's half of K (sample rows 64 hk + 16 t')
        floatx16 acc;
#pragma unroll
        for (int qq = 0; qq < 16; ++qq) acc[qq] = 0.f;
        float dgm = 0.f, dgs = 0.f;
        auto read_ab = [&](int t, bf8v (&av)[3], bf8v (&bv)[3]) __attribute__((always_inline)) {
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                typedef __attribute__((address_space(3))) s4v* lds_s4;
                const int o = p * kBfImg + 2048 * t;
                av[p] = cat44(__builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(rda + o)),
                              __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(rda + o + 512)));
                bv[p] = cat44(__builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(rdb + o)),
                              __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(rdb + o + 512)));
            }
        };
        // one K-step of fragments at a time: the SIMD's other wave covers the
        // LDS latency (a second set would spill)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            bf8v fa[3], fb[3];
            read_ab(4 * hk + t, fa, fb);
#pragma unroll
            for (int qi = 3 * t; qi < 3 * t + 3; ++qi) issue_a(qi, nxt, has_next, vo_n);
            acc = mfma6(fa, fb, acc);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (diag) {
#pragma unroll 1
            for (int t = 0; t < 4; ++t) {
                bf8v av[3], bv[3];
                read_ab(4 * hk + t, av, bv);
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    const f32x2 e = (bf_pair(av[0], j) + bf_pair(av[1], j)) + bf_pair(av[2], j);
                    const f32x2 gg = (bf_pair(bv[0], j) + bf_pair(bv[1], j)) + bf_pair(bv[2], j);
                    dgm += gg[0] + gg[1];
                    dgs = fmaf(gg[1], e[1], fmaf(gg[0], e[0], dgs));
                }
            }
        }
        ph(1);
        __syncthreads();  // B1: every wave done with the eps and G images of this tile
        ph(2);
        // ---- the partner's partial of this wave's groups: send the other two
        // (wave-uniform selects between constant accumulator indices: a
        // run-time index into the accumulators would go through scratch)
        auto accg = [&](int gsel, int e) __attribute__((always_inline)) {
            return hk == 0 ? acc[4 * (gsel + 2) + e] : acc[4 * gsel + e];  // gsel of the OTHER half
        };
        auto accown = [&](int gi, int e) __attribute__((always_inline)) {
            return hk == 0 ? acc[4 * gi + e] : acc[4 * (gi + 2) + e];
        };
        {
#pragma unroll
            for (int gi = 0; gi < 2; ++gi)
                *reinterpret_cast<f32x4*>(Xd + ((wv * 2 + gi) * 64 + lane) * 4) =
                    f32x4{accg(gi, 0), accg(gi, 1), accg(gi, 2), accg(gi, 3)};
            if (diag && hk == 1) {
                // the diagonal sums of this half for the partner (hk 0 runs the mean / sd Adam)
                Xg[wv * 128 + lane] = dgm;
                Xg[wv * 128 + 64 + lane] = dgs;
            }
        }
        __syncthreads();  // B2
        float dv[8];
        {
#pragma unroll
            for (int gi = 0; gi < 2; ++gi) {
                const f32x4 o4 = *reinterpret_cast<const f32x4*>(Xd + ((pw * 2 + gi) * 64 + lane) * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) dv[4 * gi + e] = accown(gi, e) + o4[e];
            }
            if (diag && hk == 0) {
                dgm += Xg[pw * 128 + lane];
                dgs += Xg[pw * 128 + 64 + lane];
            }
        }
        const int n = cur.n, r = 64 * cur.b + 32 * wr + l32;
        // ---- diagonal tile: mean / sd of the band's rows (the hk = 0 wave)
        if (diag && hk == 0) {
            dgm += __shfl_xor(dgm, 32, kWave);
            dgs += __shfl_xor(dgs, 32, kWave);
            if (h == 0 && r < n) {
                const int pm = (int)cur.poff + r, ps = pm + n;
                const float mu = a.params[pm], sdr = a.params[ps];
                float gmean, gsd, mun, sdn;
                diag_head(a, mu, sdr, dgm, dgs, gmean, gsd, kld);
                adam_diag(a.adam, mu, gmean, a.m[pm], a.v[pm], sdr, gsd, a.m[ps], a.v[ps], mun, sdn);
                a.params[pm] = mun;
                a.params[ps] = sdn;
                if constexpr (FOLD) {
                    // the band's new mean and softplus(sd) for its combine, on
                    // lines of the band's own, write-through: the combine may
                    // run on another XCD, and the params lines are shared with
                    // the neighbouring bands, whose diagonal tiles and combines
                    // load them (an sc1 load is served by the reader's L2, so a
                    // line another band's reader brought there would be stale)
                    float* const bm = a.bms + 128 * (int64_t)band_id(cur);
                    __hip_atomic_store(bm + 32 * wr + l32, mun, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(bm + 64 + 32 * wr + l32, softplus_f(sdn), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        ph(3);
        // ---- Adam on this wave's two groups, their stores and L' pieces
        const bool rv = r >= 1 && r <= n - 2;
        const float kls = a.include_kl ? a.inv_s0sq : 0.f;
        uint32_t lwo[3][4], lwp[3][4];  // L' pieces [plane][element pair]: K-half hk, the partner's
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
            const int g = 2 * hk + gi;
            const int cb = 64 * cur.k + 32 * wc + 8 * g + 4 * h;
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
                const f32x2 pv0 = {P[gi][e], P[gi][e + 1]};
                kl2 = __builtin_elementwise_fma(pv0, pv0, kl2);
                const f32x2 gvv = __builtin_elementwise_fma(pv0, f32x2{kls, kls}, f32x2{dv[4 * gi + e], dv[4 * gi + e + 1]});
                const f32x2 gm = {rv && cb + e < r ? gvv[0] : 0.f, rv && cb + e + 1 < r ? gvv[1] : 0.f};
                f32x2 mm = {M4[gi][e], M4[gi][e + 1]}, vv = {V4[gi][e], V4[gi][e + 1]};
                const f32x2 pv = adam_fast_k2<KIND>(a.adam, pv0, gm, mm, vv);
                P[gi][e] = pv[0];
                P[gi][e + 1] = pv[1];
                M4[gi][e] = mm[0];
                M4[gi][e + 1] = mm[1];
                V4[gi][e] = vv[0];
                V4[gi][e + 1] = vv[1];
                uint32_t w0, w1, w2;
                split3_pk(pv, w0, w1, w2);
                const int jp = (4 * gi + e) >> 1;  // g & 1 == gi
                lwo[0][jp] = w0;
                lwo[1][jp] = w1;
                lwo[2][jp] = w2;
            }
            const uint32_t ob = (uint32_t)((cur.tb + (int64_t)((q * 4 + g) * 64 + lane) * 4) * 4);
            BSTORE128(__builtin_bit_cast(u32x4, P[gi]), rs_t, ob, 0, 16);
            BSTORE128(__builtin_bit_cast(u32x4, M4[gi]), rs_t, ob, tmb, 16);
            BSTORE128(__builtin_bit_cast(u32x4, V4[gi]), rs_t, ob, tvb, 16);
        }
        // the pieces of K-half hk to the partner, its K-half back
#pragma unroll
        for (int p = 0; p < 3; ++p)
            *reinterpret_cast<u32x4*>(Xl + ((wv * 3 + p) * 64 + lane) * 4) =
                u32x4{lwo[p][0], lwo[p][1], lwo[p][2], lwo[p][3]};
        // ---- x' += eps' L'^T for this wave's sample blocks sb = 2 hk + j: its own
        // K-half (st = hk) first, before the partner's pieces are waited for --
        // the SIMD's other wave may still be in its Adam
        auto xprime = [&](int ss, const uint32_t (&lwx)[3][4]) __attribute__((always_inline)) {
            const int st = ss == 0 ? hk : 1 - hk;
            const uint8_t* const rx = En + l32 * 128 + (((2 * (2 * wc + st) + h) ^ xsw) << 4);
            bf8v lb[3];
#pragma unroll
            for (int p = 0; p < 3; ++p)
                lb[p] = __builtin_bit_cast(bf8v, u32x4{lwx[p][0], lwx[p][1], lwx[p][2], lwx[p][3]});
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int sb = 2 * hk + j;
                bf8v fx[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) fx[p] = *reinterpret_cast<const bf8v*>(rx + p * kBfImg + 4096 * sb);
                xacc[j] = mfma6(fx, lb, xacc[j]);
                // the own half issues the next band's G (6..9), the partner's half
                // the next tile's eps' planes (0..5: stg holds the next eps planes
                // until store_col, between the halves)
                {
                    const int q0 = ss == 0 ? 6 + 2 * j : 3 * j, q1 = ss == 0 ? 8 + 2 * j : 3 * j + 3;
#pragma unroll
                    for (int qi = q0; qi < q1; ++qi) issue_b(qi, nxt, has_next, newband, vo_n);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        ph(4);
        xprime(0, lwo);
        __syncthreads();  // B3
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const u32x4 o4 = *reinterpret_cast<const u32x4*>(Xl + ((pw * 3 + p) * 64 + lane) * 4);
#pragma unroll
            for (int jp = 0; jp < 4; ++jp) lwp[p][jp] = o4[jp];
        }
        __syncthreads();  // B4: the exchange scratch read; the eps image is free
        if constexpr (has_next) store_col();  // the next tile's eps image
        xprime(1, lwp);
        ph(5);
        // ---- band end (or run end): the two column halves' x' partials -> the slot
        if constexpr (!has_next || newband) {
            __syncthreads();  // every wave done reading the eps' image (the scratch)
            if (wc == 1) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int qq = 0; qq < 16; ++qq)
                        Xs[(((wr * 2 + hk) * 2 + j) * 16 + qq) * 64 + lane] = xacc[j][qq];
            }
            __syncthreads();
            if (wc == 0) {
                // buffer stores: a scalar slot base, a per-lane 32-bit offset
                const rsrc_t rs_p = make_rsrc(a.part, 0x7fffffff);
                const int sob = __builtin_amdgcn_readfirstlane(slot * S * 64 * 4);
                if constexpr (FOLD) {
                    // fragment order, 16-byte write-through stores (a 4-byte sc1
                    // store is one fabric write each): float4 ((((wr 2 + hk) 2 +
                    // j) 4 + qg) 64 + lane) holds accumulators 4 qg .. 4 qg + 3
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int qg = 0; qg < 4; ++qg) {
                            u32x4 v4;
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                v4[e] = __float_as_uint(xacc[j][4 * qg + e] +
                                                        Xs[(((wr * 2 + hk) * 2 + j) * 16 + 4 * qg + e) * 64 + lane]);
                            BSTORE128(v4, rs_p, (uint32_t)((((((wr * 2 + hk) * 2 + j) * 4 + qg) * 64 + lane)) * 16),
                                      sob, 16);
                        }
                } else {
                    const uint32_t vb = (uint32_t)((32 * wr + l32 + 64 * (64 * hk + 4 * h)) * 4);
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int qq = 0; qq < 16; ++qq) {
                            const int sl = 32 * j + (qq & 3) + 8 * (qq >> 2);  // sample - 64 hk - 4 h
                            const float v = xacc[j][qq] + Xs[(((wr * 2 + hk) * 2 + j) * 16 + qq) * 64 + lane];
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), rs_p,
                                                                  vb + (uint32_t)(sl * 256), sob, 0);
                        }
                }
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int qq = 0; qq < 16; ++qq) xacc[j][qq] = 0.f;
            ++slot;
            if constexpr (FOLD) band_arrive();
        }
        ph(6);
        __syncthreads();  // every wave done with the eps' image
        ph(7);
        if constexpr (has_next) store_row();
        if constexpr (newband) {
            split_G();
            __syncthreads();  // the new band's G image written before any wave's dL reads it
        }
        ph(8);
        if (DIAG && wv == 0) ++tph[9];
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    for (int i = t0; i + 1 < t1; ++i) {
        if (++tk > tb_) {
            tk = 0;
            int nbl = a.nb[0];
#pragma unroll
            for (int l = 1; l < kMaxL; ++l)
                if (tl == l) nbl = a.nb[l];
            if (++tb_ == nbl) {
                tb_ = 0;
                ++tl;
            }
        }
        const StrTile nxt = str_tile(a, tl, tb_, tk);
        if (nxt.l != cur.l || nxt.b != cur.b)
            tile(nxt, T_{}, T_{});
        else
            tile(nxt, T_{}, F_{});
        cur = nxt;
    }
    tile(cur, F_{}, F_{});
    if constexpr (FOLD) {
        ph(-1);
        for (int i = 0; i < nfold; ++i) band_combine(__builtin_amdgcn_readfirstlane(fold_list[i]));
        ph(10);  // DIAG: the combines' clocks (stamp slot 12)
    }
    if (DIAG && tid == 0) {
        unsigned long long* o = a.stamps + (size_t)blockIdx.x * 16;
#pragma unroll
        for (int qq = 0; qq < 10; ++qq) o[qq] = tph[qq];
        o[10] = __builtin_amdgcn_s_memtime();
        o[11] = __builtin_amdgcn_s_memrealtime();
        o[12] = tph[10];
    }
    float klp = (kl2[0] + kl2[1]) * (0.5f * a.inv_s0sq) + kld;
    if (a.kl_out && a.include_kl) {
        const float tot = block_sum(klp, Xs);
        if (tid == 0) atomicAdd(a.kl_out, (double)tot);
    }
}

// The instantiations of one Adam kind; the diagnostics builds (DIAG: phase
// stamps) exist for PSVI_ADAM_HIGHER only.  fp32 MFMAs, four 32-sample groups:
template <int KIND>
static void launch_stream_f32(bool diag, bool pad, dim3 g, hipStream_t st, const StrArgs& b) {
    const dim3 bl(256);
    if (KIND == PSVI_ADAM_HIGHER && diag)
        hipLaunchKernelGGL((mvn_stream_kernel<4, PSVI_ADAM_HIGHER, true>), g, bl, 0, st, b);
    else if (pad)
        hipLaunchKernelGGL((mvn_stream_kernel<4, KIND, false, true, true>), g, bl, 0, st, b);
    else
        hipLaunchKernelGGL((mvn_stream_kernel<4, KIND>), g, bl, 0, st, b);
}
// both products on the bf16 matrix cores (fp32-faithful pieces)
template <int KIND>
static void launch_stream_bf(bool diag, bool fold, dim3 g, hipStream_t st, const StrArgs& b) {
    const dim3 bl(512);
    if (KIND == PSVI_ADAM_HIGHER && diag && fold)
        hipLaunchKernelGGL((mvn_stream_bf2_kernel<PSVI_ADAM_HIGHER, true, true>), g, bl, 0, st, b);
    else if (fold)
        hipLaunchKernelGGL((mvn_stream_bf2_kernel<KIND, false, true>), g, bl, 0, st, b);
    else
        hipLaunchKernelGGL(mvn_stream_bf2_kernel<KIND>, g, bl, 0, st, b);
}

// the streaming update of a tiled-state step with a next one (launch_mvn_update)
hipError_t launch_mvn_stream(const psvi_plan& p, const MvnUpdate& r, const MvnRoute& rt, hipStream_t st) {
    StrArgs b{};
    fill_update(p, r, b);
    fill_tiled(p, r, p.str_part.dev, b);
    b.ranges = p.str.dev;
    for (int l = 0; l < p.L; ++l) {
        b.xcol[l] = p.xcol_l[p.rank][l];
        b.nb[l] = p.lay[l].nb;
    }
    const dim3 sg(p.str.n());
    const bool higher = b.adam.kind == PSVI_ADAM_HIGHER;
    if (rt.kernel == MvnRoute::STREAM_BF) {
        b.stamps = g_diag.bf_stamps;
        b.ep = r.eps_planes;
        b.enp = r.next.planes;
        b.pl = p.eps_planes.pl;
        for (int l = 0; l < p.L; ++l) {
            b.ppoff[l] = p.eps_planes.poff[l];
            b.npad[l] = p.eps_planes.npad[l];
        }
        b.rbs = p.sfrb.dev;
        b.bcnt = p.str_cnt.dev;
        b.bms = p.str_bms.dev;
        b.x = r.next.x;
        b.ldx = p.rows_tot[p.rank];
        if (higher) launch_stream_bf<PSVI_ADAM_HIGHER>(b.stamps, rt.fold, sg, st, b);
        else launch_stream_bf<PSVI_ADAM_HYPERGRAD>(b.stamps, rt.fold, sg, st, b);
    } else {
        const bool diag = b.stamps && b.S == 128;
        if (higher) launch_stream_f32<PSVI_ADAM_HIGHER>(diag, r.padded, sg, st, b);
        else launch_stream_f32<PSVI_ADAM_HYPERGRAD>(diag, r.padded, sg, st, b);
    }
    return hipGetLastError();
}

}  // namespace psvi
