// kernels_mvn_fwd.hip -- the full-covariance sample x = mean + L eps: the item
// grid and its reduce, the segmented sample (fp32 and bf16 pieces), and the
// next-step reduce behind the fused updates (see mvn_common.hpp).
#include "mvn_common.hpp"

namespace psvi {

constexpr int FBK = 64;    // k (columns of L) per LDS stage
constexpr int FST = 128;   // samples per pass: 4 waves x 32
constexpr int FLD = FBK + 4;  // LDS row stride: 16-byte rows (float4 stores, ds_read_b128)

struct FwdArgs {
    const FwdItem* items;
    const float* params;
    const float* eps;
    float* part;      // split-K partial slots [n_items][S][32]
    int ldx, S;
    int64_t e_total;  // floats in eps (load guards)
    const float* diag_of;  // HVP tangent sample: params is the direction vec, and the
                           // diagonal is sigmoid(diag_of's sd) vec_sd (nullptr: softplus(sd))
    // pair launches (launch_mvn_fwd_pair, blockIdx.y / .z = 1): the second
    // sample's parameters, split-K slots and diagonal source
    const float* params2;
    float* part2;
    const float* diag_of2;
    int abl;                     // diagnostics ablation mask (0 in production):
                                 // 1 loads, 2 MFMAs, 4 x atomics
    unsigned long long* stamps;  // diagnostics: 16 slots per workgroup
    // segmented sample (mvn_fwd_seg_kernel): segments, per-workgroup offsets,
    // parameter count (buffer range), sample rows per slot (0: S, one slot spans
    // all samples -- the item grid and the fused updates' slots)
    const FsSeg* segs;
    const int* seg_off;
    int64_t pcount;
    int slot_rows;
    int slot_frag;  // slots in MFMA fragment order (the segmented sample)
    int seg_nrun;  // runs in seg_off (one per workgroup)
    MvnLayerArgs lay[kMaxL];
};

// One item: rows [r0, r1) (<= kFwdRows) of L against columns [k0, k1) for all
// samples: D[s][r] = sum_c eps[s][c] L[r][c] on v_mfma_f32_32x32x2_f32; wave w
// owns 32 samples x all kFwdRows rows (FT = kFwdRows/32 accumulators), so one
// eps fragment feeds FT MFMAs and the eps block (L2-resident, shared by every
// item of the column range) is read once per kFwdRows rows.  Stages of 64 columns:
// L rows (packed triangle, 256-byte runs) and eps rows go global -> registers
// (float4) -> LDS, the next stage's loads in flight during this stage's
// MFMAs.  k-permuted operand feed: one ds_read_b128 per operand per 4 MFMAs.
// Each item stores its partial sums in its own slot; mvn_fwd_reduce_kernel
// adds a row block's slots and mean + softplus(sd) eps into x (split-K
// without atomics; float atomics from the k-chunks of a row block contend on
// the same addresses).
__global__ __launch_bounds__(256, 2) void mvn_fwd_kernel(FwdArgs a) {
    __shared__ __attribute__((aligned(16))) float Es[FST * FLD];       // eps  [s][k]
    __shared__ __attribute__((aligned(16))) float Ls[kFwdRows * FLD];  // corr [r][k]
    MVN_STAMP(0, __builtin_amdgcn_s_memtime());
    MVN_STAMP(6, __builtin_amdgcn_s_memrealtime());  // chip-wide 100 MHz clock
    MVN_STAMP(4, (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4));
    MVN_STAMP(5, (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20));
    const FwdItem it = a.items[blockIdx.x];
    const int n = a.lay[it.layer].n;
    const bool second = blockIdx.y == 1;  // pair launch: the second sample
    const float* corr = (second ? a.params2 : a.params) + a.lay[it.layer].poff + 2 * n;
    float* const part = second ? a.part2 : a.part;
    const int corr_len = (int)((int64_t)(n - 1) * (n - 2) / 2);
    const int eoff = (int)a.lay[it.layer].eoff;
    const rsrc_t re = make_rsrc(a.eps, 4 * a.e_total);
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id(), h = lane >> 5, l32 = lane & 31;
    const int col4 = tid & 15, srow = tid >> 4;
    constexpr int FT = kFwdRows / 32, LJ = kFwdRows / 16;
    // this thread's staged L rows
    int lrp[LJ];
#pragma unroll
    for (int j = 0; j < LJ; ++j) {
        const int r = it.r0 + srow + 16 * j;
        lrp[j] = r >= 1 ? (int)((int64_t)r * (r - 1) / 2) : 0;
    }
    const int klast = it.k0 + ((it.k1 - it.k0 - 1) / FBK) * FBK;  // last stage start

    // sample blocks: gridDim.z workgroups share an item's FST-sample passes
    // (launch_mvn_fwd spreads them when the items alone leave CUs idle)
    for (int sb = blockIdx.z * FST; sb < a.S; sb += FST * gridDim.z) {
        floatx16 acc[FT];
#pragma unroll
        for (int t = 0; t < FT; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
        const bool wave_live = sb + 32 * wv < a.S;
        float4 lreg[LJ], ereg[8];
        // eps through buffer loads: the per-dword range check returns 0 past
        // the buffer's end, and rows past S go to offset kOOB (zeros) -- no
        // clamp, fix-up or select at staging
        auto eofs = [&](int j, int kb) {
            const int sr = sb + srow + 16 * j;
            return sr < a.S ? (uint32_t)(eoff + sr * n + kb + 4 * col4) * 4u : kOOB;
        };
        auto fetch = [&](int kb) {
#pragma unroll
            for (int j = 0; j < LJ; ++j)
                lreg[j] = ld4u(corr, (a.abl & 1) ? 0 : lrp[j] + kb + 4 * col4, 0, corr_len);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                ereg[j] = __builtin_bit_cast(
                    float4, __builtin_amdgcn_raw_buffer_load_b128(re, (a.abl & 1) ? 0u : eofs(j, kb), 0, 0));
        };
        auto stage = [&](int kb) {
            const int c = kb + 4 * col4;
#pragma unroll
            for (int j = 0; j < LJ; ++j) {
                // entries outside the item / triangle / column range are 0
                const int r = it.r0 + srow + 16 * j;
                const float4 v = fix4(lreg[j], lrp[j] + c, 0, corr_len);
                const bool rok = r < it.r1 && r <= n - 2;
                float4 o;
                o.x = rok && c + 0 < r && c + 0 < it.k1 ? v.x : 0.f;
                o.y = rok && c + 1 < r && c + 1 < it.k1 ? v.y : 0.f;
                o.z = rok && c + 2 < r && c + 2 < it.k1 ? v.z : 0.f;
                o.w = rok && c + 3 < r && c + 3 < it.k1 ? v.w : 0.f;
                *reinterpret_cast<float4*>(&Ls[(srow + 16 * j) * FLD + 4 * col4]) = o;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) *reinterpret_cast<float4*>(&Es[(srow + 16 * j) * FLD + 4 * col4]) = ereg[j];
        };
        if (it.k0 < it.k1) fetch(it.k0);
        for (int kb = it.k0; kb < it.k1; kb += FBK) {
            __syncthreads();  // previous stage's MFMAs done with the LDS
            stage(kb);
            __syncthreads();
            fetch(min(kb + FBK, klast));  // unconditional: keeps the vmcnt bookkeeping exact
            if (kb == it.k0 && sb == 0) MVN_STAMP(1, __builtin_amdgcn_s_memtime());
            if (wave_live && !(a.abl & 2)) {
                // k permutation: per 8 columns, lane half h feeds k = kk + 4h + j to
                // MFMA j (j = 0..3) for BOTH operands -- the same sum over k
                const float* Ea = Es + (32 * wv + l32) * FLD + 4 * h;
                const float* Lb = Ls + l32 * FLD + 4 * h;
#pragma unroll
                for (int kk = 0; kk < FBK; kk += 8) {
                    const float4 av = *reinterpret_cast<const float4*>(Ea + kk);
                    float4 bv[FT];
#pragma unroll
                    for (int t = 0; t < FT; ++t)
                        bv[t] = *reinterpret_cast<const float4*>(Lb + 32 * t * FLD + kk);
#pragma unroll
                    for (int t = 0; t < FT; ++t) {
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv[t].x, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv[t].y, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv[t].z, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv[t].w, acc[t], 0, 0, 0);
                    }
                }
            }
        }
        MVN_STAMP(2, __builtin_amdgcn_s_memtime());
        // D[i = s][j = r]: j = lane&31, i = (q&3) + 8(q>>2) + 4h
        if (wave_live && !(a.abl & 4)) {
#pragma unroll
            for (int t = 0; t < FT; ++t) {
                if (it.r0 + 32 * t + l32 >= it.r1) continue;
                float* slot = part + (size_t)it.slot * a.S * kFwdRows + 32 * t + l32;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int s = sb + 32 * wv + (q & 3) + 8 * (q >> 2) + 4 * h;
                    if (s < a.S) slot[(size_t)s * kFwdRows] = acc[t][q];
                }
            }
        }
    }
    MVN_STAMP(3, __builtin_amdgcn_s_memtime());
    MVN_STAMP(7, __builtin_amdgcn_s_memrealtime());
}

// x[s][xcol + rr] = mean[r] + softplus(sd[r]) eps[s][r] + sum over the row
// block's slots (r = r0 + rr); one workgroup per (row block, 256/kFwdRows
// samples), coalesced along the rows.
// Two samples per thread (s and s + 4 of the block's 8): the row block's
// descriptor, mean and softplus(sd) serve both, and twice the loads are in
// flight.
constexpr int kRedSpb = 2 * 256 / kFwdRows;  // samples per reduce block
__global__ __launch_bounds__(256) void mvn_fwd_reduce_kernel(const FwdRowBlock* rbs,
                                                             const float* part, FwdArgs a,
                                                             float* x, float* x2 = nullptr) {
    const FwdRowBlock rb = rbs[blockIdx.x];
    // pair launch: the second sample (locals -- writing into the by-value
    // argument copies the whole struct to scratch)
    const bool second = blockIdx.z == 1;
    if (second) {
        part = a.part2;
        x = x2;
    }
    const float* const prm = second ? a.params2 : a.params;
    const float* const dof = second ? a.diag_of2 : a.diag_of;
    const int rr = threadIdx.x & (kFwdRows - 1);
    // slots of slot_rows samples from sample rb.s0 (0 / S: one slot spans all)
    const int srows = a.slot_rows > 0 ? a.slot_rows : a.S;
    const int l0 = blockIdx.y * kRedSpb + threadIdx.x / kFwdRows, l1 = l0 + kRedSpb / 2;
    const int s0 = rb.s0 + l0, s1 = rb.s0 + l1, s_end = min(a.S, rb.s0 + srows);
    if (s0 >= s_end || rr >= rb.R) return;
    const bool two = s1 < s_end;
    const int n = a.lay[rb.layer].n, r = rb.r0 + rr;
    const float* mean = prm + a.lay[rb.layer].poff;
    const float* eps = a.eps + a.lay[rb.layer].eoff + r;
    const float e0 = eps[(int64_t)s0 * n], e1 = eps[(int64_t)(two ? s1 : s0) * n];
    const float mu = mean[r], sdr = mean[n + r];
    const size_t st = (size_t)srows * kFwdRows;
    // slot element (sample l, row rr): row-major [l][rr], or (a.slot_frag, the
    // segmented sample) the MFMA fragment order of mvn_fwd_seg_kernel
    auto so = [&](int l) -> size_t {
        if (!a.slot_frag) return (size_t)l * kFwdRows + rr;
        const int i = l & 31, hh = (i >> 2) & 1, q = (i & 3) + 4 * (i >> 3);
        return ((size_t)((l >> 5) * (kFwdRows / 32) + (rr >> 5)) * 16 + q) * 64 + (rr & 31) + 32 * hh;
    };
    const float* p0 = part + (size_t)rb.slot0 * st + so(l0);
    const float* p1 = part + (size_t)rb.slot0 * st + so(two ? l1 : l0);
    // The first 8 slots as unconditional loads at clamped indices (all in
    // flight at once; a row block of C3's streaming update has 1-10 slots),
    // any further ones 4 at a time.  Partial sums s4[k % 4] in slot order k =
    // 0, 1, ..., so the result does not depend on the unroll.
    float a4[4] = {0.f, 0.f, 0.f, 0.f}, b4[4] = {0.f, 0.f, 0.f, 0.f};
    {
        float va[8], vb[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const size_t o = (size_t)max(min(i, rb.nk - 1), 0) * st;
            va[i] = p0[o];
            vb[i] = p1[o];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            a4[i & 3] += i < rb.nk ? va[i] : 0.f;
            b4[i & 3] += i < rb.nk ? vb[i] : 0.f;
        }
    }
    int k = 8;
    for (; k + 4 <= rb.nk; k += 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a4[i] += p0[(k + i) * st];
            b4[i] += p1[(k + i) * st];
        }
    }
    for (int i = 0; k + i < rb.nk; ++i) {
        a4[i] += p0[(k + i) * st];
        b4[i] += p1[(k + i) * st];
    }
    const float dg = dof ? sigmoid_f(dof[a.lay[rb.layer].poff + n + r]) * sdr
                               : softplus_f(sdr);
    // mean + (softplus(sd) eps, rounded) + the slots: the product never fused
    // into an fma, here and in the streaming update's in-kernel combine, so
    // the two give the same bits
    x[(int64_t)s0 * a.ldx + rb.xcol + rr] = (mu + mul_unfused(dg, e0)) + ((a4[0] + a4[1]) + (a4[2] + a4[3]));
    if (two)
        x[(int64_t)s1 * a.ldx + rb.xcol + rr] = (mu + mul_unfused(dg, e1)) + ((b4[0] + b4[1]) + (b4[2] + b4[3]));
}

// Segmented sample (K = S > 128): one persistent workgroup run of the
// (row block, pass, column block) unit list (build_fseg), two per CU.  Per
// segment -- consecutive column blocks of one (row block, 128-sample pass) --
// D[s][r] = sum_c eps[s][c] L[r][c] accumulates over its column blocks as in
// mvn_fwd_kernel (64-column LDS stages, k-permuted ds_read_b128 feed, wave w
// = 32 samples x 64 rows), then goes to the segment's slot ([128][64]); the
// reduce adds a (row block, pass)'s slots.  The next stage -- the next
// segment's first after a segment's last -- is loaded behind the MFMAs.  corr
// and eps through buffer loads: the range check returns 0 past the end (rows
// past S to offset kOOB); the triangle / row masks are applied at staging.
__global__ __launch_bounds__(256, 2) void mvn_fwd_seg_kernel(FwdArgs a) {
    __shared__ __attribute__((aligned(16))) float Es[FST * FLD];       // eps  [s][k]
    __shared__ __attribute__((aligned(16))) float Ls[kFwdRows * FLD];  // corr [r][k]
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id(), h = lane >> 5, l32 = lane & 31;
    const int col4 = tid & 15, srow = tid >> 4;
    constexpr int FT = kFwdRows / 32, LJ = kFwdRows / 16;
    const rsrc_t re = make_rsrc(a.eps, 4 * a.e_total);
    const rsrc_t rp = make_rsrc(a.params, 4 * a.pcount);
    const int sbeg = a.seg_off[blockIdx.x], send = a.seg_off[blockIdx.x + 1];
    if (sbeg >= send) return;  // uniform, before any barrier
    struct D {
        int n, corr, eoff, r0, r1, s0;
    };
    auto desc = [&](const FsSeg& g) __attribute__((always_inline)) {
        D d;
        int poff = (int)a.lay[0].poff;
        d.n = a.lay[0].n;
        d.eoff = (int)a.lay[0].eoff;
#pragma unroll
        for (int l = 1; l < kMaxL; ++l)  // select: a dynamic index into the arguments goes to scratch
            if (g.layer == l) {
                d.n = a.lay[l].n;
                d.eoff = (int)a.lay[l].eoff;
                poff = (int)a.lay[l].poff;
            }
        d.corr = poff + 2 * d.n;
        d.r0 = g.r0;
        d.r1 = g.r1;
        d.s0 = g.pass * FST;
        return d;
    };
    float4 lreg[LJ], ereg[8];
    auto fetch = [&](const D& d, int kb) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < LJ; ++j) {
            const int r = d.r0 + srow + 16 * j;
            const int ro = r >= 1 ? (int)((int64_t)r * (r - 1) / 2) : 0;
            lreg[j] = __builtin_bit_cast(
                float4, __builtin_amdgcn_raw_buffer_load_b128(rp, (uint32_t)(d.corr + ro + kb + 4 * col4) * 4u, 0, 0));
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int sr = d.s0 + srow + 16 * j;
            const uint32_t eo = sr < a.S ? (uint32_t)(d.eoff + sr * d.n + kb + 4 * col4) * 4u : kOOB;
            ereg[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(re, eo, 0, 0));
        }
    };
    auto stage = [&](const D& d, int kb) __attribute__((always_inline)) {
        const int c = kb + 4 * col4;
#pragma unroll
        for (int j = 0; j < LJ; ++j) {
            // entries outside the block's rows / the strict lower triangle are 0
            const int r = d.r0 + srow + 16 * j;
            const bool rok = r < d.r1 && r <= d.n - 2;
            const float4 v = lreg[j];
            float4 o;
            o.x = rok && c + 0 < r ? v.x : 0.f;
            o.y = rok && c + 1 < r ? v.y : 0.f;
            o.z = rok && c + 2 < r ? v.z : 0.f;
            o.w = rok && c + 3 < r ? v.w : 0.f;
            *reinterpret_cast<float4*>(&Ls[(srow + 16 * j) * FLD + 4 * col4]) = o;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) *reinterpret_cast<float4*>(&Es[(srow + 16 * j) * FLD + 4 * col4]) = ereg[j];
    };
    // diagnostics (a.stamps): shader clocks -- 1 until the first stage is in
    // LDS, 2 stages + MFMAs, 3 slot writes (summed over segments); 6 stages;
    // 0 / 12 start / end, 13 / 14 the 100 MHz clock at start / end
    const bool dgn = a.stamps != nullptr;
    unsigned long long ph[4] = {0ull, 0ull, 0ull, 0ull}, tprev = dgn ? __builtin_amdgcn_s_memtime() : 0ull;
    const unsigned long long t_start = tprev, rt_start = dgn ? __builtin_amdgcn_s_memrealtime() : 0ull;
    int nst = 0;
    auto mark = [&](int q) __attribute__((always_inline)) {
        if (dgn) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            ph[q] += t - tprev;
            tprev = t;
        }
    };
    FsSeg gn = a.segs[sbeg];
    D dn = desc(gn);
    fetch(dn, gn.k0);
    for (int si = sbeg; si < send; ++si) {  // uniform
        const FsSeg g = gn;
        const D d = dn;
        const bool more = si + 1 < send;
        if (more) {
            gn = a.segs[si + 1];
            dn = desc(gn);
        }
        floatx16 acc[FT];
#pragma unroll
        for (int t = 0; t < FT; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
        const bool wave_live = d.s0 + 32 * wv < a.S;
        for (int kb = g.k0; kb < g.k1; kb += FBK) {  // uniform
            __syncthreads();  // previous stage's MFMAs done with the LDS
            stage(d, kb);
            __syncthreads();
            if (si == sbeg && kb == g.k0) mark(1);
            ++nst;
            {
                const bool inseg = kb + FBK < g.k1;
                if (inseg || more) fetch(inseg ? d : dn, inseg ? kb + FBK : gn.k0);
            }
            if (wave_live) {
                // k permutation: per 8 columns, lane half h feeds k = kk + 4h + j to
                // MFMA j (j = 0..3) for BOTH operands -- the same sum over k
                const float* Ea = Es + (32 * wv + l32) * FLD + 4 * h;
                const float* Lb = Ls + l32 * FLD + 4 * h;
#pragma unroll
                for (int kk = 0; kk < FBK; kk += 8) {
                    const float4 av = *reinterpret_cast<const float4*>(Ea + kk);
                    float4 bv[FT];
#pragma unroll
                    for (int t = 0; t < FT; ++t) bv[t] = *reinterpret_cast<const float4*>(Lb + 32 * t * FLD + kk);
#pragma unroll
                    for (int t = 0; t < FT; ++t) {
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv[t].x, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv[t].y, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv[t].z, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv[t].w, acc[t], 0, 0, 0);
                    }
                }
            }
        }
        mark(2);
        // the accumulators in fragment order ((wave FT + t) 16 + q) 64 + lane: every
        // store a contiguous 256-byte wave run (the reduce reads the order back)
        if (wave_live) {
            float* slot = a.part + (size_t)g.slot * FST * kFwdRows + (size_t)wv * FT * 16 * 64 + lane;
#pragma unroll
            for (int t = 0; t < FT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) slot[(t * 16 + q) * 64] = acc[t][q];
        }
        mark(3);
    }
    if (dgn && threadIdx.x == 0) {
        unsigned long long* o = a.stamps + (size_t)blockIdx.x * 16;
        o[0] = t_start;
        for (int q = 1; q < 4; ++q) o[q] = ph[q];
        o[6] = (unsigned long long)nst;
        o[12] = __builtin_amdgcn_s_memtime();
        o[13] = rt_start;
        o[14] = __builtin_amdgcn_s_memrealtime();
    }
}

// mvn_fwd_seg_bf_kernel: mvn_fwd_seg_kernel with the GEMM on the bf16 matrix
// cores, fp32-faithful (the pieces of mvn_stream_bf2_kernel): each stage's eps
// block [128 s][64 k] and masked L block [64 r][64 k] are split at staging
// into three bf16 planes each, stored as row images (128-byte rows, 16-byte
// chunk c of row s at c ^ ((s >> 1) & 7)), and both operands read with one
// ds_read_b128 per plane: lane (l32, h) of K-step t takes k = 16 t + 8 h ..
// + 7 of row l32 -- the same k order for A (eps, M = samples) and B (L, N =
// rows), so the accumulators, slots and reduce are mvn_fwd_seg_kernel's.
// 72 KB of LDS: two workgroups per CU, as the fp32 kernel.
//
// PAIR (psvi_hvp's sample pair, launch_mvn_fwd_pair): x = L eps and the
// tangent x2 = Lv eps in one launch on the same segments.  Eight waves: wave
// group g = wv >> 2 stages and multiplies group g's matrix (g 0: params, 1:
// params2) into its own L image and writes its own slots (part / part2); the
// eps stage is shared, each group staging half of its rows.  96 KB of LDS, one
// workgroup per CU (the same eight waves per CU as two single workgroups).
constexpr int kSegEImg = FST * 128;       // bytes per eps plane image
constexpr int kSegLImg = kFwdRows * 128;  // bytes per L plane image
__device__ __forceinline__ int seg_img(int s, int chunk) {
    return s * 128 + ((chunk ^ ((s >> 1) & 7)) << 4);
}
template <bool PAIR>
__global__ __launch_bounds__(PAIR ? 512 : 256, PAIR ? 1 : 2) void mvn_fwd_seg_bf_kernel(FwdArgs a) {
    constexpr int NG = PAIR ? 2 : 1;  // matrices (wave groups)
    __shared__ __attribute__((aligned(16))) uint8_t smb[3 * kSegEImg + NG * 3 * kSegLImg];
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l32 = lane & 31;
    const int gw = PAIR ? __builtin_amdgcn_readfirstlane(wave_id() >> 2) : 0;  // wave group
    const int wv = wave_id() & 3, tl = tid & 255;
    const int col4 = tl & 15, srow = tl >> 4;
    uint8_t* const Eb = smb;
    uint8_t* const Lb = smb + 3 * kSegEImg + gw * 3 * kSegLImg;
    constexpr int FT = kFwdRows / 32, LJ = kFwdRows / 16;
    constexpr int EJ = 8 / NG;  // eps rows staged per thread: rows srow + 16 (EJ gw + j)
    const rsrc_t re = make_rsrc(a.eps, 4 * a.e_total);
    const rsrc_t rp = make_rsrc(gw ? a.params2 : a.params, 4 * a.pcount);
    const int sbeg = a.seg_off[blockIdx.x], send = a.seg_off[min((int)blockIdx.x + 1, a.seg_nrun)];
    if (sbeg >= send) return;  // uniform, before any barrier
    // a stage: column block kb of segment si (si == send: past the run's end)
    struct St {
        int si, kb, n, corr, eoff, r0, r1, s0, k1;
    };
    auto stage_at = [&](int si, int kb) __attribute__((always_inline)) {
        St d;
        d.si = si;
        d.kb = kb;
        if (si >= send) return d;
        const FsSeg g = a.segs[si];
        int poff = (int)a.lay[0].poff;
        d.n = a.lay[0].n;
        d.eoff = (int)a.lay[0].eoff;
#pragma unroll
        for (int l = 1; l < kMaxL; ++l)  // select: a dynamic index into the arguments goes to scratch
            if (g.layer == l) {
                d.n = a.lay[l].n;
                d.eoff = (int)a.lay[l].eoff;
                poff = (int)a.lay[l].poff;
            }
        d.corr = poff + 2 * d.n;
        d.r0 = g.r0;
        d.r1 = g.r1;
        d.s0 = g.pass * FST;
        d.k1 = g.k1;
        if (kb < 0) d.kb = g.k0;
        return d;
    };
    auto next = [&](const St& d) __attribute__((always_inline)) {
        return d.kb + FBK < d.k1 ? stage_at(d.si, d.kb + FBK) : stage_at(d.si + 1, -1);
    };
    // two register sets: stage i + 2 is loaded behind stage i's MFMAs
    float4 lreg[2][LJ], ereg[2][EJ];
    auto fetch = [&](const St& d, float4 (&lr)[LJ], float4 (&er)[EJ]) __attribute__((always_inline)) {
        if (d.si >= send) return;  // uniform
#pragma unroll
        for (int j = 0; j < LJ; ++j) {
            const int r = d.r0 + srow + 16 * j;
            const int ro = r >= 1 ? (int)((int64_t)r * (r - 1) / 2) : 0;
            lr[j] = __builtin_bit_cast(
                float4, __builtin_amdgcn_raw_buffer_load_b128(rp, (uint32_t)(d.corr + ro + d.kb + 4 * col4) * 4u, 0, 0));
        }
#pragma unroll
        for (int j = 0; j < EJ; ++j) {
            const int sr = d.s0 + srow + 16 * (EJ * gw + j);
            const uint32_t eo = sr < a.S ? (uint32_t)(d.eoff + sr * d.n + d.kb + 4 * col4) * 4u : kOOB;
            er[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(re, eo, 0, 0));
        }
    };
    // a thread's 4 columns 4 col4 .. + 3: half (col4 & 1) of chunk col4 >> 1
    const int cw = (col4 & 1) * 8;
    auto put = [&](uint8_t* img, int pbytes, int row, float4 v) __attribute__((always_inline)) {
        uint32_t x0[2], x1[2], x2[2];
        split3_pk(f32x2{v.x, v.y}, x0[0], x1[0], x2[0]);
        split3_pk(f32x2{v.z, v.w}, x0[1], x1[1], x2[1]);
        uint8_t* q = img + seg_img(row, col4 >> 1) + cw;
        *reinterpret_cast<u32x2*>(q) = u32x2{x0[0], x0[1]};
        *reinterpret_cast<u32x2*>(q + pbytes) = u32x2{x1[0], x1[1]};
        *reinterpret_cast<u32x2*>(q + 2 * pbytes) = u32x2{x2[0], x2[1]};
    };
    auto stage = [&](const St& d, const float4 (&lr)[LJ], const float4 (&er)[EJ]) __attribute__((always_inline)) {
        const int c = d.kb + 4 * col4;
#pragma unroll
        for (int j = 0; j < LJ; ++j) {
            // entries outside the block's rows / the strict lower triangle are 0
            const int r = d.r0 + srow + 16 * j;
            const bool rok = r < d.r1 && r <= d.n - 2;
            const float4 v = lr[j];
            float4 o;
            o.x = rok && c + 0 < r ? v.x : 0.f;
            o.y = rok && c + 1 < r ? v.y : 0.f;
            o.z = rok && c + 2 < r ? v.z : 0.f;
            o.w = rok && c + 3 < r ? v.w : 0.f;
            put(Lb, kSegLImg, srow + 16 * j, o);
        }
#pragma unroll
        for (int j = 0; j < EJ; ++j) put(Eb, kSegEImg, srow + 16 * (EJ * gw + j), er[j]);
    };
    // operand bases: A row 32 wv + l32 of the eps image, B rows 32 t + l32 of
    // the L image; K-step t, half h -> chunk 2 t + h (the swizzle of row s
    // depends on s alone: (s >> 1) & 7 = (l32 >> 1) & 7 for both)
    const int sw = (l32 >> 1) & 7;
    const uint8_t* const ra = Eb + (32 * wv + l32) * 128;
    const uint8_t* const rb = Lb + l32 * 128;
    floatx16 acc[FT];
#pragma unroll
    for (int t = 0; t < FT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
    St cur = stage_at(sbeg, -1);
    St nx1 = next(cur);
    fetch(cur, lreg[0], ereg[0]);
    fetch(nx1, lreg[1], ereg[1]);
    // one stage with register set P: stage, load the stage after next into P,
    // the MFMAs; at a segment's last stage its slot is written
    auto body = [&](auto P_c) __attribute__((always_inline)) {
        constexpr int P = decltype(P_c)::value;
        __syncthreads();  // previous stage's MFMAs done with the LDS
        stage(cur, lreg[P], ereg[P]);
        __syncthreads();
        const St nx2 = next(nx1);
        fetch(nx2, lreg[P], ereg[P]);
        const bool wave_live = cur.s0 + 32 * wv < a.S;
        if (wave_live) {
#pragma unroll
            for (int t = 0; t < FBK / 16; ++t) {
                const int co = ((2 * t + h) ^ sw) << 4;
                bf8v av[3], bv[FT][3];
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    av[p] = *reinterpret_cast<const bf8v*>(ra + p * kSegEImg + co);
#pragma unroll
                    for (int u = 0; u < FT; ++u)
                        bv[u][p] = *reinterpret_cast<const bf8v*>(rb + p * kSegLImg + 32 * 128 * u + co);
                }
#pragma unroll
                for (int u = 0; u < FT; ++u) acc[u] = mfma6(av, bv[u], acc[u]);
            }
        }
        if (nx1.si != cur.si) {  // uniform: the segment's last stage
            // the accumulators in fragment order, as mvn_fwd_seg_kernel
            if (wave_live) {
                const FsSeg g = a.segs[cur.si];
                float* slot = (gw ? a.part2 : a.part) + (size_t)g.slot * FST * kFwdRows + (size_t)wv * FT * 16 * 64 + lane;
#pragma unroll
                for (int t = 0; t < FT; ++t)
#pragma unroll
                    for (int q = 0; q < 16; ++q) slot[(t * 16 + q) * 64] = acc[t][q];
            }
#pragma unroll
            for (int t = 0; t < FT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
        }
        cur = nx1;
        nx1 = nx2;
    };
    for (;;) {  // uniform
        body(std::integral_constant<int, 0>{});
        if (cur.si >= send) break;
        body(std::integral_constant<int, 1>{});
        if (cur.si >= send) break;
    }
}

// Workgroups per forward item along the samples: the items (row blocks x
// column chunks of the rank's rows) run their FST-sample passes in parallel
// when they alone would leave the chip's 2 x 256 workgroup slots idle -- the
// K = S >> 128 shapes (a rank's rows for all S = 1024 samples at 8 ranks, C4
// on one GPU); every (item, sample) partial still has one writer.
static int fwd_sample_blocks(const psvi_plan& p, int pairs = 1) {
    const int nsb = (p.d.S + FST - 1) / FST;
    const int want = (512 + p.fwd.n() * pairs - 1) / (p.fwd.n() * pairs);
    return std::max(1, std::min(nsb, want));
}

hipError_t launch_mvn_fwd(const psvi_plan& p, const float* eps, const float* params,
                          float* x_shard, hipStream_t st, const float* diag_of) {
    FwdArgs a{};
    a.diag_of = diag_of;
    a.items = p.fwd.dev;
    a.params = params;
    a.eps = eps;
    a.part = p.fwd_part.dev;
    a.ldx = p.rows_tot[p.rank];
    a.S = p.d.S;
    a.e_total = p.Peps;
    a.abl = g_diag.fwd_ablation;
    a.stamps = g_diag.fwd_stamps;
    fill_layers(p, a.lay);
    if (p.n_fswg() > 0 && !g_diag.fs_off) {
        // K = S > 128: the segmented sample, then the (row block, pass) reduce
        a.segs = p.fs_segs.dev;
        a.seg_off = p.fs_off.dev;
        a.pcount = p.P;
        a.part = p.fs_part.dev;
        a.slot_rows = FST;
        a.slot_frag = 1;
        a.seg_nrun = p.n_fswg();
        a.abl = 0;
        if (g_diag.fs_bf_off || a.stamps)
            hipLaunchKernelGGL(mvn_fwd_seg_kernel, dim3(p.n_fswg()), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL(mvn_fwd_seg_bf_kernel<false>, dim3(p.n_fswg()), dim3(256), 0, st, a);
        hipLaunchKernelGGL(mvn_fwd_reduce_kernel, dim3(p.fs_rb.n(), FST / kRedSpb), dim3(256), 0, st,
                           p.fs_rb.dev, p.fs_part.dev, a, x_shard);
        return hipGetLastError();
    }
    if (p.fwd.n() == 0) return hipSuccess;
    // every x element is written by exactly one reduce thread: no memset
    hipLaunchKernelGGL(mvn_fwd_kernel, dim3(p.fwd.n(), 1, fwd_sample_blocks(p)), dim3(256), 0, st, a);
    constexpr int spb = kRedSpb;  // samples per reduce workgroup
    hipLaunchKernelGGL(mvn_fwd_reduce_kernel, dim3(p.frb.n(), (a.S + spb - 1) / spb), dim3(256), 0,
                       st, p.frb.dev, p.fwd_part.dev, a, x_shard);
    return hipGetLastError();
}

// x = mean + L eps (params) and x2 = its HVP tangent, v_mean + Lv eps with the
// diagonal from params (vec), in one launch of each kernel: the items of the
// two GEMMs share eps through L2 and fill the chip together (psvi_hvp)
hipError_t launch_mvn_fwd_pair(const psvi_plan& p, const float* eps, const float* params,
                               float* x, const float* vec, float* x2, float* part2,
                               hipStream_t st) {
    if (p.n_fpwg() > 0 && !g_diag.fs_off && !g_diag.fs_bf_off && g_diag.fwd_pair_bf) {
        // the segmented sample's units over the pair table (256 workgroups of
        // eight waves), both matrices per unit (the eps stage shared), then the
        // pair reduce over the two slot sets.  Measured at C3: 25.4 + 7.5 us
        // against the fp32 item grid's 39.2 + 7.9 (psvi_hvp 0.120 -> 0.107 ms);
        // the two bf16-piece samples one after the other took 2 x (20.1 + 6.8),
        // the pair on the sample's 512-run table (two runs per workgroup) 29.5 + 9.3
        FwdArgs a{};
        a.params = params;
        a.eps = eps;
        a.params2 = vec;
        a.diag_of2 = params;
        a.part = p.fs_part.dev;
        a.part2 = part2;
        a.ldx = p.rows_tot[p.rank];
        a.S = p.d.S;
        a.e_total = p.Peps;
        a.segs = p.fp_segs.dev;
        a.seg_off = p.fp_off.dev;
        a.pcount = p.P;
        a.slot_rows = FST;
        a.slot_frag = 1;
        a.seg_nrun = p.n_fpwg();
        fill_layers(p, a.lay);
        hipLaunchKernelGGL(mvn_fwd_seg_bf_kernel<true>, dim3(p.n_fpwg()), dim3(512), 0, st, a);
        hipLaunchKernelGGL(mvn_fwd_reduce_kernel, dim3(p.fp_rb.n(), FST / kRedSpb, 2), dim3(256), 0, st, p.fp_rb.dev,
                           p.fs_part.dev, a, x, x2);
        return hipGetLastError();
    }
    FwdArgs a{};
    a.items = p.fwd.dev;
    a.params = params;
    a.eps = eps;
    a.part = p.fwd_part.dev;
    a.params2 = vec;
    a.part2 = part2;
    a.diag_of2 = params;
    a.ldx = p.rows_tot[p.rank];
    a.S = p.d.S;
    a.e_total = p.Peps;
    a.abl = g_diag.fwd_ablation;
    fill_layers(p, a.lay);
    if (p.fwd.n() == 0) return hipSuccess;
    hipLaunchKernelGGL(mvn_fwd_kernel, dim3(p.fwd.n(), 2, fwd_sample_blocks(p, 2)), dim3(256), 0, st, a);
    constexpr int spb = kRedSpb;
    hipLaunchKernelGGL(mvn_fwd_reduce_kernel, dim3(p.frb.n(), (a.S + spb - 1) / spb, 2), dim3(256),
                       0, st, p.frb.dev, p.fwd_part.dev, a, x, x2);
    return hipGetLastError();
}

// x_next = mean' + softplus(sd') eps_next + the sum of each row block's partial slots
hipError_t launch_next_reduce(const psvi_plan& p, const MvnUpdate& r, const FwdRowBlock* rbs,
                              int nrb, const float* part, hipStream_t st) {
    FwdArgs f{};
    f.params = r.params;
    f.eps = r.next.eps;
    f.ldx = p.rows_tot[p.rank];
    f.S = p.d.S;
    fill_layers(p, f.lay);
    constexpr int spb = kRedSpb;
    hipLaunchKernelGGL(mvn_fwd_reduce_kernel, dim3(nrb, (f.S + spb - 1) / spb), dim3(256), 0, st,
                       rbs, part, f, r.next.x);
    return hipGetLastError();
}

}  // namespace psvi
