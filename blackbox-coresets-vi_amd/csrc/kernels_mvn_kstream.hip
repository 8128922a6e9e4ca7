// kernels_mvn_kstream.hip -- the K-split streaming update (see mvn_common.hpp).
#include <type_traits>

#include "mvn_common.hpp"

namespace psvi {

// The full-cov Adam update at K = S > 128 (every rank of the row-sharded step,
// where a rank's rows take all S samples; C4 on one GPU): the rank's 64 x 64
// tiles with their K cut in 128-sample passes, units (tile, pass) dealt as
// equal contiguous runs to persistent workgroups (two per CU; build_kstream).
// Per pass: the band's G rows and the tile's eps column block staged into LDS
// (register prefetch of the next pass during the MFMAs), dL^T[c][r] +=
// sum_s eps[s][c] G[s][r] on v_mfma_f32_32x32x2_f32 (4 waves = 2 x 2 of 32 x
// 32), the diagonal tile also sum_s G and sum_s G eps per row.  A tile whose
// passes all sit in one run goes straight to the Adam epilogue (the chunked
// kernel's packed epilogue: accumulators transposed through LDS, corr / m / v
// as 256-byte row runs).  A split tile's contributors write their partials to
// their slots with write-through (sc1) stores, drain them (vmcnt 0), and one
// lane adds to the tile's counter (relaxed, agent scope); the contributor that
// draws the last ticket reads every partial with sc1 loads, adds them in pass
// order (the result does not depend on who arrives last) and runs the
// epilogue -- the in-launch split-K combine of cdna_hip_programming.md (§6
// Guideline 16, counter form), correct for any placement of the contributors.
// No workgroup ever waits on another: the kernel cannot hang on the hand-off.
// The ticket stays relaxed on purpose: sc1 stores + the vmcnt(0) drain before
// the add is the first row of MI355X_MICROARCH.md's hand-off table (release by
// drain, acquire by sc1 loads); an acq_rel atomic would add an L2 writeback /
// invalidate per contributor (1.7 - 3.5 us per launch at C4 W = 8) for no
// ordering the drain does not give.  The last arriver resets the counter in
// the same launch; an aborted launch ends the process, so no half-counted
// ticket reaches a later launch.
struct KsArgs : MvnUpdCommon, MvnUpdGrad {
    const KsTile* tiles;
    const KsSeg* segs;
    const int* seg_off;
    float* slots;
    int* cnt;
    int64_t slot_bytes;
    const float* g2;  // GRAD: a second G slot added at staging (slot 0 + slot 1, as slot_sum_kernel)
};

// G / eps / corr / m / v through buffer loads whose per-dword range check
// returns 0 past the end (rows past S are sent to offset kOOB): no clamped
// addresses, fix-ups or zero selects at staging.  The first pass of the next
// segment is loaded behind the last pass of this one (its latency overlaps the
// hand-off and the epilogue).
// BF: the dL GEMM on bf16 pieces (fp32-faithful, mvn_stream_bf2_kernel's
// products): a pass's G and eps blocks are split at staging into three bf16
// planes each, in two halves of 64 samples (column images of 8 KB per plane,
// read with ds_read_b64_tr_b16; 48 KB of LDS, two workgroups per CU), each
// half's next loads issued as soon as it is staged.  The diagonal tile's row
// sums come from the planes (their sum is the fp32 value exactly).
constexpr int kKsBfImg = 64 * 128;  // bytes per plane image (64 samples x 64 columns)
struct KsBfShared {
    uint8_t img[6 * kKsBfImg];  // eps planes, then G planes; the epilogue's T tile after the passes
    float red[2 * 4 * 64];
};
template <bool BF, bool GRAD = false>
__global__ __launch_bounds__(256, 2) void mvn_kstream_kernel(KsArgs a) {
    __shared__ __attribute__((aligned(16))) std::conditional_t<BF, KsBfShared, UpdShared<true>> sh;
    static_assert(kKsPass == USB, "one LDS stage per pass");
    static_assert(64 * TLD * 4 <= 6 * kKsBfImg, "the epilogue tile fits the images");
    float* Gs = nullptr;
    float* Es = nullptr;
    if constexpr (!BF) {
        Gs = sh.Gs;
        Es = sh.Es;
    }
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id(), h = lane >> 5, l32 = lane & 31;
    const int wr = wv >> 1, wc = wv & 1;
    const int col4 = tid & 15, srow = tid >> 4;
    const FragPos fp{wr, wc, h, l32};
    const rsrc_t rs = make_rsrc(a.slots, a.slot_bytes);
    const rsrc_t rg = make_rsrc(a.g, 4 * a.g_total), re = make_rsrc(a.eps, 4 * a.e_total);
    const rsrc_t rg2 = make_rsrc(a.g2, GRAD && a.g2 ? 4 * a.g_total : 0);
    // GRAD: m reads kl_vec (0 when none: an empty range), v is not read
    const rsrc_t rpar = make_rsrc(a.params, 4 * a.pcount),
                 rm = make_rsrc(GRAD ? a.kl_vec : a.m, GRAD && !a.kl_vec ? 0 : 4 * a.pcount),
                 rv = make_rsrc(a.v, 4 * a.pcount);
    float klp = 0.f;
    // diagnostics (a.stamps): shader clocks per phase summed over the segments
    // -- 1 first-pass load wait, 2 passes (MFMAs + later loads), 3 hand-off,
    // 4 partial sums, 5 epilogue; 6 segments, 7 combines; 0 / 12 start / end,
    // 13 / 14 the 100 MHz clock at start / end
    const bool dg = a.stamps != nullptr;
    unsigned long long ph[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    unsigned long long tprev = dg ? __builtin_amdgcn_s_memtime() : 0ull;
    const unsigned long long t_start = tprev, rt_start = dg ? __builtin_amdgcn_s_memrealtime() : 0ull;
    int ncomb = 0;
    auto mark = [&](int k) __attribute__((always_inline)) {
        if (dg) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            ph[k] += t - tprev;
            tprev = t;
        }
    };
    // a segment's pass operands: G columns gcol.., eps [S][n] at eoff, columns ecol..
    struct Ld {
        int gcol, eoff, n, ecol;
    };
    auto desc = [&](const KsTile& t) __attribute__((always_inline)) {
        Ld d;
        d.n = a.lay[0].n;
        d.eoff = (int)a.lay[0].eoff;
#pragma unroll
        for (int l = 1; l < kMaxL; ++l)  // select: a dynamic index into the arguments goes to scratch
            if (t.layer == l) {
                d.n = a.lay[l].n;
                d.eoff = (int)a.lay[l].eoff;
            }
        d.gcol = t.xcol + t.r0 + 4 * col4;
        d.ecol = t.k * UB + 4 * col4;
        return d;
    };
    float4 greg[8], ereg[8], greg2[GRAD ? 8 : 1];
    auto load = [&](const Ld& d, int pi) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int s = pi * USB + srow + 16 * j;
            const bool live = s < a.S;
            const uint32_t go = live ? (uint32_t)(s * a.ldg + d.gcol) * 4u : kOOB;
            const uint32_t eo = live ? (uint32_t)(d.eoff + s * d.n + d.ecol) * 4u : kOOB;
            greg[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rg, go, 0, 0));
            ereg[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(re, eo, 0, 0));
        }
    };
    auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int o = (srow + 16 * j) * ULD + 4 * col4;
            *reinterpret_cast<float4*>(&Gs[o]) = greg[j];
            *reinterpret_cast<float4*>(&Es[o]) = ereg[j];
        }
    };
    // BF: half hp of a pass (samples 64 hp + srow + 16 j', registers j = 4 hp + j')
    uint8_t* const Eb = BF ? reinterpret_cast<uint8_t*>(&sh) : nullptr;
    uint8_t* const Gb = BF ? reinterpret_cast<uint8_t*>(&sh) + 3 * kKsBfImg : nullptr;
    auto load_half = [&](const Ld& d, int pi, int hp) __attribute__((always_inline)) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = 4 * hp + jj;
            const int s = pi * USB + srow + 16 * j;
            const bool live = s < a.S;
            const uint32_t go = live ? (uint32_t)(s * a.ldg + d.gcol) * 4u : kOOB;
            const uint32_t eo = live ? (uint32_t)(d.eoff + s * d.n + d.ecol) * 4u : kOOB;
            greg[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rg, go, 0, 0));
            ereg[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(re, eo, 0, 0));
            if (GRAD) greg2[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rg2, go, 0, 0));
        }
    };
    auto stage_half = [&](int hp) __attribute__((always_inline)) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = 4 * hp + jj, sl = srow + 16 * jj;
            if (GRAD && a.g2) {
                greg[j].x += greg2[j].x;
                greg[j].y += greg2[j].y;
                greg[j].z += greg2[j].z;
                greg[j].w += greg2[j].w;
            }
            uint32_t x[3][2], y[3][2];
            split3_pk(f32x2{greg[j].x, greg[j].y}, x[0][0], x[1][0], x[2][0]);
            split3_pk(f32x2{greg[j].z, greg[j].w}, x[0][1], x[1][1], x[2][1]);
            split3_pk(f32x2{ereg[j].x, ereg[j].y}, y[0][0], y[1][0], y[2][0]);
            split3_pk(f32x2{ereg[j].z, ereg[j].w}, y[0][1], y[1][1], y[2][1]);
            const int o = img_col(sl, 4 * col4);
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                *reinterpret_cast<u32x2*>(Gb + p * kKsBfImg + o) = u32x2{x[p][0], x[p][1]};
                *reinterpret_cast<u32x2*>(Eb + p * kKsBfImg + o) = u32x2{y[p][0], y[p][1]};
            }
        }
    };
    // the transposed reads (mvn_stream_bf2_kernel's): lane 4 qq + pp of its
    // 16-lane group takes sample row qq, columns 4 pp .. + 3 of its 16
    const int g16 = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
    const uint8_t* const rda = BF ? Eb + img_col(8 * h + qq, 32 * wc + 16 * (g16 & 1) + 4 * pp) : nullptr;
    const uint8_t* const rdb = BF ? Gb + img_col(8 * h + qq, 32 * wr + 16 * (g16 & 1) + 4 * pp) : nullptr;
    auto read_ab = [&](int t, bf8v (&av)[3], bf8v (&bv)[3]) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            typedef __attribute__((address_space(3))) s4v* lds_s4;
            const int o = p * kKsBfImg + 2048 * t;  // sample rows 16 t + 8 h + qq (+ 4)
            av[p] = cat44(__builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(rda + o)),
                          __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(rda + o + 512)));
            bv[p] = cat44(__builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(rdb + o)),
                          __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(rdb + o + 512)));
        }
    };
    const int sbeg = a.seg_off[blockIdx.x], send = a.seg_off[blockIdx.x + 1];
    KsSeg sg_next = a.segs[sbeg < send ? sbeg : 0];
    if (sbeg < send) {
        if constexpr (BF) {
            load_half(desc(a.tiles[sg_next.tile]), sg_next.p0, 0);
            load_half(desc(a.tiles[sg_next.tile]), sg_next.p0, 1);
        } else {
            load(desc(a.tiles[sg_next.tile]), sg_next.p0);
        }
    }
    for (int si = sbeg; si < send; ++si) {  // uniform
        if (dg) tprev = __builtin_amdgcn_s_memtime();
        const KsSeg sg = sg_next;
        const KsTile tl = a.tiles[sg.tile];
        const Ld cur = desc(tl);
        const int n = cur.n;
        int poff = (int)a.lay[0].poff;
#pragma unroll
        for (int l = 1; l < kMaxL; ++l)
            if (tl.layer == l) poff = (int)a.lay[l].poff;
        const int corr_off = poff + 2 * n;
        // the segment after this one: its first pass loads behind our last
        const bool more = si + 1 < send;
        if (more) sg_next = a.segs[si + 1];
        const Ld nxt = desc(a.tiles[sg_next.tile]);
        // epilogue rows: r_j = r0 + srow + 16 j, columns 64 k + 4 col4 + (0..3)
        int rowp[4];
        bool rown[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = tl.r0 + srow + 16 * j;
            rown[j] = r >= tl.rlo && r < tl.rhi && r >= 1 && r <= n - 2;
            rowp[j] = corr_off + (int)((int64_t)r * (r - 1) / 2);
        }
        float4 pq[4], mq[4], vq[4];
        // the diagonal tile's mean / sd rows (thread tid & 63 -> row r0 + (tid & 63)):
        // value, m, v of both, loaded with corr / m / v (not one round trip each)
        float dmu = 0.f, dsd = 0.f, dmm = 0.f, dmv = 0.f, dsm = 0.f, dsv = 0.f;
        const int pm_d = poff + tl.r0 + (tid & 63), ps_d = pm_d + n;
        auto load_pmv = [&]() {
            if (tl.diag) {  // uniform
                const uint32_t om = (uint32_t)pm_d * 4u, os = (uint32_t)ps_d * 4u;
                dmu = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rpar, om, 0, 0));
                dsd = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rpar, os, 0, 0));
                if (!GRAD) {
                    dmm = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, om, 0, 0));
                    dmv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rv, om, 0, 0));
                    dsm = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, os, 0, 0));
                    dsv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rv, os, 0, 0));
                }
            }
            const int cl = tl.k * UB + 4 * col4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // rows off the band's corr rows load something valid, never stored
                const uint32_t o = (uint32_t)(rowp[j] + cl) * 4u;
                pq[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rpar, o, 0, 0));
                mq[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rm, o, 0, 0));
                if (!GRAD) vq[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rv, o, 0, 0));
            }
        };
        floatx16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        float dgm = 0.f, dgs = 0.f;
        const bool whole = sg.slot < 0;
        for (int pi = sg.p0; pi < sg.p1; ++pi) {  // uniform
            const bool inseg = pi + 1 < sg.p1;
            if constexpr (BF) {
#pragma unroll
                for (int hp = 0; hp < 2; ++hp) {
                    __syncthreads();  // every wave done with the images
                    stage_half(hp);
                    __syncthreads();
                    if (pi == sg.p0 && hp == 0) mark(1);
                    // this half's registers refilled at once: the next pass's
                    // half (after the segment's last pass, the next segment's)
                    if (inseg || more) load_half(inseg ? cur : nxt, inseg ? pi + 1 : sg_next.p0, hp);
                    if (pi * USB + 64 * hp >= a.S) continue;  // uniform: a ragged last pass
                    // one K-step of fragments at a time (the other workgroup on
                    // the CU covers the LDS latency; a second set spills)
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        bf8v fa[3], fb[3];
                        read_ab(t, fa, fb);
                        acc = mfma6(fa, fb, acc);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (tl.diag && wc == wr) {
                        // the diagonal quadrants: lane (c = r, h) reads eps and G of
                        // the same row for its samples -- sum_s G, sum_s G eps
#pragma unroll 1
                        for (int t = 0; t < 4; ++t) {
                            bf8v av[3], bv[3];
                            read_ab(t, av, bv);
#pragma unroll
                            for (int j = 0; j < 8; j += 2) {
                                const f32x2 e = (bf_pair(av[0], j) + bf_pair(av[1], j)) + bf_pair(av[2], j);
                                const f32x2 gg = (bf_pair(bv[0], j) + bf_pair(bv[1], j)) + bf_pair(bv[2], j);
                                dgm += gg[0] + gg[1];
                                dgs = fmaf(gg[1], e[1], fmaf(gg[0], e[0], dgs));
                            }
                        }
                    }
                }
                continue;
            }
            stage();
            __syncthreads();
            if (pi == sg.p0) mark(1);
            // the next pass's operands behind this pass's MFMAs -- after the
            // segment's last pass, the next segment's first (corr / m / v are
            // loaded at the epilogue: prefetched here they keep 48 more
            // registers live across the MFMAs and the kernel takes scratch)
            if (inseg || more) load(inseg ? cur : nxt, inseg ? pi + 1 : sg_next.p0);
            const int kend = min(USB, a.S - pi * USB);
            if (tl.diag) {
                // column j of Es is row r0 + j of the band
                for (int s = 32 * wv; s < 32 * wv + 32 && s < kend; ++s) {
                    const float gv = Gs[s * ULD + lane];
                    dgm += gv;
                    dgs = fmaf(gv, Es[s * ULD + lane], dgs);
                }
            }
            const float* Ea = Es + h * ULD + 32 * wc + l32;
            const float* Gb = Gs + h * ULD + 32 * wr + l32;
            for (int kk = 0; kk < kend; kk += 16) {
                float av[8], bv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    av[u] = Ea[(kk + 2 * u) * ULD];
                    bv[u] = Gb[(kk + 2 * u) * ULD];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
            }
            __syncthreads();  // every wave done with Gs / Es
        }
        if (BF && tl.diag) {
            // the two halves' sums; row 32 wr + l32 of the band kept by wave 0
            // in lanes 0..31 and by wave 3 in lanes 32..63, so that the
            // epilogue's wave sum red[w 64 + j] sees row j once
            dgm += __shfl_xor(dgm, 32, kWave);
            dgs += __shfl_xor(dgs, 32, kWave);
            if (!((wv == 0 && h == 0) || (wv == 3 && h == 1))) dgm = dgs = 0.f;
        }
        mark(2);
        if (!whole) {
            // ---- split tile: publish this contributor's partial (fragment order:
            // float4 (w * 4 + g) * 64 + lane; then 2 floats of diagonal sums per thread)
            const uint32_t sbase = (uint32_t)((sg.slot + sg.ci) * kKsSlotFloats) * 4u;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                BSTORE128(
                    __builtin_bit_cast(u32x4, make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2],
                                                          acc[4 * g + 3])),
                    rs, sbase + (uint32_t)(((wv * 4 + g) * 64 + lane) * 16), 0, 16);
            if (tl.diag)
                __builtin_amdgcn_raw_buffer_store_b64(
                    __builtin_bit_cast(u32x2, f32x2{dgm, dgs}), rs,
                    sbase + (uint32_t)(4096 * 4 + tid * 8), 0, 16);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                const int old = __hip_atomic_fetch_add(a.cnt + tl.cnt, 1, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
                sh.red[0] = __int_as_float(old);
            }
            __syncthreads();
            const int old = __float_as_int(sh.red[0]);
            __syncthreads();  // everyone has read the ticket before red is reused
            mark(3);
            if (old != sg.nc - 1) continue;  // uniform: another contributor finishes the tile
            ++ncomb;
            // the last arriver: every partial, in pass order, through sc1 loads
            if (tid == 0)
                __hip_atomic_store(a.cnt + tl.cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            load_pmv();
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = 0.f;
            dgm = dgs = 0.f;
            // the partials KP at a time (all their loads in flight together),
            // added in pass order; past nc the last one is loaded again, not added
            constexpr int KP = BF ? 2 : 4;  // BF: fewer registers beside the image bases
            for (int c0 = 0; c0 < sg.nc; c0 += KP) {  // uniform
                float4 part[KP][4];
                f32x2 pd[KP];
#pragma unroll
                for (int i = 0; i < KP; ++i) {
                    const int c = min(c0 + i, sg.nc - 1);
                    const uint32_t cb = (uint32_t)((sg.slot + c) * kKsSlotFloats) * 4u;
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        part[i][g] = __builtin_bit_cast(
                            float4, __builtin_amdgcn_raw_buffer_load_b128(
                                        rs, cb + (uint32_t)(((wv * 4 + g) * 64 + lane) * 16), 0, 16));
                    pd[i] = tl.diag ? __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(
                                                                   rs, cb + (uint32_t)(4096 * 4 + tid * 8), 0, 16))
                                    : f32x2{0.f, 0.f};
                }
#pragma unroll
                for (int i = 0; i < KP; ++i) {
                    if (c0 + i >= sg.nc) break;  // uniform
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        acc[4 * g] += part[i][g].x;
                        acc[4 * g + 1] += part[i][g].y;
                        acc[4 * g + 2] += part[i][g].z;
                        acc[4 * g + 3] += part[i][g].w;
                    }
                    dgm += pd[i][0];
                    dgs += pd[i][1];
                }
            }
            mark(4);
        }
        if (whole) load_pmv();
        // ---- Adam epilogue: D[i = c][j = r] (j = lane & 31, i = (q & 3) + 8 (q >> 2) + 4 h)
        // -> T[r][c] in Es, then the rows' 256-byte runs of corr / m / v
        float* T = BF ? reinterpret_cast<float*>(&sh) : Es;
        if constexpr (BF) __syncthreads();  // the images are T now: every wave past its last reads
        store_frag_T(T, fp, acc);
        __syncthreads();
        const int cb = tl.k * UB + 4 * col4;
        float klt = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = tl.r0 + srow + 16 * j;
            if (!rown[j] || cb >= r) continue;
            const int o = rowp[j] + cb;
            const float4 d4 = *reinterpret_cast<const float4*>(&T[(srow + 16 * j) * TLD + 4 * col4]);
            const float4 p4 = pq[j], m4 = mq[j], v4 = GRAD ? float4{} : vq[j];
            float pn[4], mn[4], vn[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float p = f4get(p4, i);
                klt += cb + i < r ? p * p : 0.f;
                float gval = a.include_kl ? f4get(d4, i) + p * a.inv_s0sq : f4get(d4, i);
                if (GRAD) {
                    // the chunked kernel's gradient mode (upd_chunk): + kl_vec / s0^2
                    if (a.kl_vec) gval += f4get(m4, i) * a.inv_s0sq;
                    pn[i] = gval;
                    continue;
                }
                float mm = f4get(m4, i), vv = f4get(v4, i);
                pn[i] = adam_apply_fast(a.adam, p, gval, mm, vv);
                mn[i] = mm;
                vn[i] = vv;
            }
            const float4 pn4 = make_float4(pn[0], pn[1], pn[2], pn[3]);
            if (GRAD)
                store_packed_run<1>({a.grad_out}, {pn4}, o, cb, r);
            else
                store_packed_run<3>({a.params, a.m, a.v},
                                    {pn4, make_float4(mn[0], mn[1], mn[2], mn[3]),
                                     make_float4(vn[0], vn[1], vn[2], vn[3])}, o, cb, r);
        }
        klp += klt * (0.5f * a.inv_s0sq);
        if (tl.diag) {
            // the band's mean / sd from the four waves' row sums, added in wave order
            sh.red[wv * 64 + lane] = dgm;
            sh.red[256 + wv * 64 + lane] = dgs;
            __syncthreads();
            const int rr = tl.r0 + tid;
            if (tid < 64 && rr >= tl.rlo && rr < tl.rhi) {
                const float* red = sh.red;
                const float gm = red[tid] + red[64 + tid] + red[128 + tid] + red[192 + tid];
                const float gs = red[256 + tid] + red[320 + tid] + red[384 + tid] + red[448 + tid];
                const int pm = pm_d, ps = ps_d;  // rr = r0 + tid
                float gmean, gsd;
                diag_head(a, dmu, dsd, gm, gs, gmean, gsd, klp);
                if (GRAD) {
                    a.grad_out[pm] = gmean;
                    a.grad_out[ps] = gsd;
                } else {
                    adam_diag(a.adam, dmu, gmean, dmm, dmv, dsd, gsd, dsm, dsv, dmu, dsd);
                    a.params[pm] = dmu;
                    a.m[pm] = dmm;
                    a.v[pm] = dmv;
                    a.params[ps] = dsd;
                    a.m[ps] = dsm;
                    a.v[ps] = dsv;
                }
            }
        }
        __syncthreads();  // T / red reads done before the next segment stages
        mark(5);
    }
    if (a.kl_out && a.include_kl) {
        const float tot = block_sum(klp, sh.red);
        if (tid == 0) atomicAdd(a.kl_out, (double)tot);
    }
    if (dg && tid == 0) {
        unsigned long long* o = a.stamps + (size_t)blockIdx.x * 16;
        o[0] = t_start;
        for (int k = 1; k < 6; ++k) o[k] = ph[k];
        o[6] = (unsigned long long)(send - sbeg);
        o[7] = (unsigned long long)ncomb;
        o[12] = __builtin_amdgcn_s_memtime();
        o[13] = rt_start;
        o[14] = __builtin_amdgcn_s_memrealtime();
    }
}

// the K-split update (launch_mvn_update: K = S > 128, or gradient mode on the slots)
hipError_t launch_mvn_kstream(const psvi_plan& p, const MvnUpdate& r, const MvnRoute& rt, hipStream_t st) {
    KsArgs k{};
    fill_update(p, r, k);
    fill_grad(p, r, k);
    k.tiles = p.ks_tiles.dev;
    k.segs = p.ks_segs.dev;
    k.seg_off = p.ks_off.dev;
    k.slots = p.ks_slots.dev;
    k.cnt = p.ks_cnt.dev;
    k.slot_bytes = (int64_t)sizeof(float) * std::max(1, p.n_ks_slots) * kKsSlotFloats;
    k.g2 = r.g_shard2;
    const dim3 grid(p.n_kwg()), block(256);
    if (rt.grad)
        hipLaunchKernelGGL((mvn_kstream_kernel<true, true>), grid, block, 0, st, k);
    else if (!rt.bf)
        hipLaunchKernelGGL(mvn_kstream_kernel<false>, grid, block, 0, st, k);
    else
        hipLaunchKernelGGL(mvn_kstream_kernel<true>, grid, block, 0, st, k);
    return hipGetLastError();
}

}  // namespace psvi
