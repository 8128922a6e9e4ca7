// kernels_mvn_update.hip -- the full-covariance update (backward): the chunked
// kernel and its forms, the packed <-> tiled state converter, mvn_route (which
// kernel a request takes) and launch_mvn_update, which switches on it over this
// unit's, the K-split and the streaming launchers (see mvn_common.hpp).
#include "mvn_common.hpp"

namespace psvi {

// FUSE kernels: part holds the partial x_next per chunk slot
struct UpdArgs : MvnUpdCommon, MvnUpdGrad, MvnUpdTiled {
    const UpdChunk* chunks;
    int abl;  // diagnostics ablation mask (0 in production)
};

template <bool GRAD>
__device__ __forceinline__ void upd_elem(const UpdArgs& a, int64_t pidx, float gval) {
    if (GRAD) {
        a.grad_out[pidx] = gval;
    } else {
        float mm = a.m[pidx], vv = a.v[pidx];
        const float pn = adam_apply(a.adam, a.params[pidx], gval, mm, vv);
        a.params[pidx] = pn;
        a.m[pidx] = mm;
        a.v[pidx] = vv;
    }
}

// One chunk: for each of its c-blocks, dL^T[c][r] = sum_s eps[s][c] G[s][r]
// (v_mfma_f32_32x32x2_f32, 4 waves = 2 x 2 sub-tiles of 32 x 32), then
//   corr <- Adam(corr, dL + corr/s0^2)         (or grad_out in GRAD mode).
// The accumulator tile goes through LDS (into the eps stage, free after the
// MFMAs) so the corr / m / v / grad traffic moves in 256-byte row runs, four
// rows per wave instruction.
// Pipeline: after each staging barrier the next step's operand loads (eps,
// and G when S > 128; clamped to the last step rather than skipped) and, on a
// c-block's last sample pass, its corr/m/v loads are issued; the MFMAs run
// while they land.  Every global load is unconditional: a load under a
// branch makes the compiler's vmcnt bookkeeping fall back to vmcnt(0).
// The diagonal c-block (columns = the band's rows) also yields sum_s G and
// sum_s G*eps per row: the mean / sd update.
// MODE: 0 = S <= 64 (one eps half), 1 = S <= 128 (two halves), 2 = S > 128.
// FUSE (Adam, MODE < 2): also the next step's sample from the updated L --
// per c-block, x_next[s][r] += sum_c eps_next[s][c] L_new[r][c] on a second
// MFMA GEMM (L_new tile through the LDS tile region, eps_next fragments
// straight from L2 into registers), partial sums to the chunk's slot.
// PKO (tiled state, no fused sample: an inner loop's last step): corr / m / v
// read from the tiled state, written back to the packed arrays
template <bool GRAD, int MODE, bool FUSE, bool TILED, bool PKO = false>
__device__ __forceinline__ void upd_chunk(const UpdArgs& a, const UpdChunk& ch,
                                          UpdShared<MODE == 2>& sh) {
    constexpr bool MULTI = MODE == 2, TWOH = MODE == 1;
    static_assert(!FUSE || (!GRAD && !MULTI), "fused sample: Adam mode, S <= 128");
    static_assert(!TILED || (!GRAD && !MULTI), "tiled state: Adam mode, S <= 128");
    float* Gs = sh.Gs;
    float* Es = sh.Es;
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id(), h = lane >> 5, l32 = lane & 31;
    const int wr = wv >> 1, wc = wv & 1;
    const FragPos fp{wr, wc, h, l32};
    const int n = a.lay[ch.layer].n;
    const int eoff = (int)a.lay[ch.layer].eoff;
    const float* E = a.eps + eoff;  // [S][n]; the whole eps buffer is [-eoff, e_rem)
    const int e_rem = (int)a.e_total - eoff;
    const int g_total = (int)a.g_total, pcount = (int)a.pcount;
    const int poff = (int)a.lay[ch.layer].poff, corr_off = poff + 2 * n;
    const int np = MULTI ? (a.S + USB - 1) / USB : 1;
    const int nt = ch.k1 - ch.k0;
    const int kd = ch.diag ? ch.r0 / UB - ch.k0 : -1;  // diagonal c-block index in the chunk

    // staging / epilogue map: 16 lanes x float4 = one 64-column row, rows srow + 16 j
    const int col4 = tid & 15, srow = tid >> 4;
    const int gcol = ch.xcol + ch.r0 + 4 * col4;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 greg[8], ereg[8];
    // sample row s is clamped to S-1 (rows >= S are zeroed at the LDS write)
    // (ablation 1: every G / eps load from one cached address)
    const int ab1 = (a.abl & 1) ? 0 : 1;
    auto goff = [&](int s) { return ab1 * (min(s, a.S - 1) * a.ldg + gcol); };
    auto eofs = [&](int s, int ti) {
        return ab1 * (min(s, a.S - 1) * n + (ch.k0 + ti) * UB + 4 * col4);
    };
    auto load_G = [&](int pi) {
#pragma unroll
        for (int j = 0; j < 8; ++j) greg[j] = ld4u(a.g, goff(pi * USB + srow + 16 * j), 0, g_total);
    };
    auto load_E = [&](int ti, int pi) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            ereg[j] = ld4u(E, eofs(pi * USB + srow + 16 * j, ti), -eoff, e_rem);
    };
    auto stage = [&](bool withG, int ti, int pi) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int o = (srow + 16 * j) * ULD + 4 * col4;
            const int sr = pi * USB + srow + 16 * j;
            const bool live = sr < a.S && !(a.abl & 1);
            if (withG)
                *reinterpret_cast<float4*>(&Gs[o]) = live ? fix4(greg[j], goff(sr), 0, g_total) : z4;
            *reinterpret_cast<float4*>(&Es[o]) =
                live ? fix4(ereg[j], eofs(sr, ti), -eoff, e_rem) : z4;
        }
    };

    // S <= 128: eps halves of UEH samples (4 float4 per thread)
    float4 ehreg[4];
    auto load_Eh = [&](int ti, int hh) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            ehreg[j] = ld4u(E, eofs(hh * UEH + srow + 16 * j, ti), -eoff, e_rem);
    };
    auto stage_Eh = [&](int ti, int hh) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int sr = hh * UEH + srow + 16 * j;
            const bool live = sr < a.S && !(a.abl & 1);
            *reinterpret_cast<float4*>(&Es[(srow + 16 * j) * ULD + 4 * col4]) =
                live ? fix4(ehreg[j], eofs(sr, ti), -eoff, e_rem) : z4;
        }
    };

    // epilogue rows: r_j = r0 + srow + 16 j, columns c0 + 4 col4 + (0..3)
    int rowp[4];
    bool rown[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = ch.r0 + srow + 16 * j;
        rown[j] = r >= ch.rlo && r < ch.rhi && r >= 1 && r <= n - 2;
        rowp[j] = corr_off + (int)((int64_t)r * (r - 1) / 2);
    }
    float4 pq[4], mq[4], vq[4];
    // tiled state: this lane's 4 fragment float4s of a tile (contiguous per wave)
    auto tile_off = [&](int ti, int g) {
        return tile_index(a.lay[ch.layer], ch.r0 / UB, ch.k0 + ti) * 4096 +
               (int64_t)((wv * 4 + g) * 64 + lane) * 4;
    };
    const int64_t ab4 = (a.abl & 4) ? 0 : 1;  // ablation 4: corr/m/v loads from one address
    auto load_pmv = [&](int ti) {
        if (TILED) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t o = ab4 * tile_off(ti, g);
                pq[g] = *reinterpret_cast<const float4*>(a.tp + o);
                mq[g] = *reinterpret_cast<const float4*>(a.tm + o);
                vq[g] = *reinterpret_cast<const float4*>(a.tv + o);
            }
            return;
        }
        const int cl = (ch.k0 + ti) * UB + 4 * col4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // rows off the band's corr rows load something valid, never stored
            pq[j] = ld4u(a.params, rowp[j] + cl, 0, pcount);
            if (!GRAD) {
                mq[j] = ld4u(a.m, rowp[j] + cl, 0, pcount);
                vq[j] = ld4u(a.v, rowp[j] + cl, 0, pcount);
            }
        }
    };

    floatx16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    float dgm = 0.f, dgs = 0.f, klp = 0.f;

    // ---- fused next-step sample state
    floatx16 acc2[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc2[t][q] = 0.f;
    float4 enreg[FUSE ? 8 : 1];
    const bool wave_s = 32 * wv < a.S;  // this wave owns samples of the fused GEMM
    const int es = min(32 * wv + l32, a.S - 1);
    const int ab32 = (a.abl & 32) ? 0 : 1;  // ablation 32: eps_next loads from one address
    auto enofs = [&](int ti, int g) { return ab32 * (es * n + (ch.k0 + ti) * UB + 8 * g + 4 * h); };
    auto load_En = [&](int ti) {
        if (FUSE) {
#pragma unroll
            for (int g = 0; g < 8; ++g) enreg[g] = ld4u(a.eps_next + eoff, enofs(ti, g), -eoff, e_rem);
        }
    };
    // x_next partial over one c-block: A = eps_next[s][c] (registers, k-permuted:
    // lane half h holds c = 8g + 4h + j for MFMA j), B = L_new[r][c] from the tile
    auto gemm2 = [&](int ti) {
        if (FUSE && wave_s && !(a.abl & 16)) {
            const float* Lb = Es + l32 * TLD + 4 * h;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const float4 av = fix4(enreg[g], enofs(ti, g), -eoff, e_rem);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const float4 bv = *reinterpret_cast<const float4*>(Lb + 32 * t * TLD + 8 * g);
                    acc2[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc2[t], 0, 0, 0);
                    acc2[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc2[t], 0, 0, 0);
                    acc2[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc2[t], 0, 0, 0);
                    acc2[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc2[t], 0, 0, 0);
                }
            }
        }
    };

    auto compute = [&](int ti, int pi) {
        const int kend = (a.abl & 2) ? 0 : min(USB, a.S - pi * USB);
        if (ti == kd) {
            // diagonal c-block: column j of Es is row r0 + j of the band
            for (int s = 32 * wv; s < 32 * wv + 32 && s < kend; ++s) {
                const float gv = Gs[s * ULD + lane];
                dgm += gv;
                dgs = fmaf(gv, Es[s * ULD + lane], dgs);
            }
        }
        // 16 samples per group (rows past S are staged as zeros up to USB)
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
    };

    // one eps half against the resident G (rows hh*UEH ..)
    auto compute_h = [&](int ti, int hh) {
        const int kend = (a.abl & 2) ? 0 : min(UEH, a.S - hh * UEH);
        if (ti == kd) {
            for (int s = 16 * wv; s < 16 * wv + 16 && s < kend; ++s) {
                const float gv = Gs[(hh * UEH + s) * ULD + lane];
                dgm += gv;
                dgs = fmaf(gv, Es[s * ULD + lane], dgs);
            }
        }
        const float* Ea = Es + h * ULD + 32 * wc + l32;
        const float* Gb = Gs + (hh * UEH + h) * ULD + 32 * wr + l32;
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
    };

    // call after a barrier that ends every wave's reads of Es
    auto epilogue = [&](int ti) {
        if (TILED) {
            // D[i = c][j = r] (j = lane & 31, i = (q&3) + 8(q>>2) + 4h) is already the
            // tile's fragment order: Adam on the accumulators, float4 in / out
            static_assert(!PKO || !FUSE, "packed-out: the last step samples nothing");
            const int r = ch.r0 + 32 * wr + l32;
            const bool rv = r >= 1 && r <= n - 2 && !(a.abl & 8);
            float kp[PKO ? 16 : 1], km[PKO ? 16 : 1], kv[PKO ? 16 : 1];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int cb = (ch.k0 + ti) * UB + 32 * wc + 8 * g + 4 * h;
                const int64_t o = tile_off(ti, g);
                float pn[4], mn[4], vn[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    // entries outside the strict lower part stay exactly 0: zero
                    // gradient, zero state (both Adam variants keep p = 0)
                    const float p = f4get(pq[g], i);
                    klp += p * p;
                    const bool ok = rv && cb + i < r;
                    const float gval = ok ? (a.include_kl ? acc[4 * g + i] + p * a.inv_s0sq
                                                          : acc[4 * g + i])
                                          : 0.f;
                    float mm = f4get(mq[g], i), vv = f4get(vq[g], i);
                    pn[i] = (a.abl & 64) ? p + gval + mm + vv
                                         : adam_apply_fast(a.adam, p, gval, mm, vv);
                    mn[i] = mm;
                    vn[i] = vv;
                }
                if (PKO) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        kp[4 * g + i] = pn[i];
                        km[4 * g + i] = mn[i];
                        kv[4 * g + i] = vn[i];
                    }
                } else if (!(a.abl & 8)) {
                    // write-through (sc1): the state leaves the XCD's L2, which keeps
                    // the eps / G blocks other chunks re-read (as the stream kernel)
                    const rsrc_t rs_t = make_rsrc(a.tp, 0x7fffffff);
                    const int tmb = __builtin_amdgcn_readfirstlane((int)((a.tm - a.tp) * 4));
                    const int tvb = __builtin_amdgcn_readfirstlane((int)((a.tv - a.tp) * 4));
                    const uint32_t ob = (uint32_t)(o * 4);
                    BSTORE128(
                        __builtin_bit_cast(u32x4, make_float4(pn[0], pn[1], pn[2], pn[3])), rs_t, ob, 0, 16);
                    BSTORE128(
                        __builtin_bit_cast(u32x4, make_float4(mn[0], mn[1], mn[2], mn[3])), rs_t, ob, tmb, 16);
                    BSTORE128(
                        __builtin_bit_cast(u32x4, make_float4(vn[0], vn[1], vn[2], vn[3])), rs_t, ob, tvb, 16);
                }
                if (FUSE)  // L_new fragment -> the [r][c] tile for the sample GEMM
                    frag_T(Es, fp, g) = make_float4(pn[0], pn[1], pn[2], pn[3]);
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = 0.f;
            if (PKO) {
                // fragment -> [r][c] through LDS, then the rows' float4 segments
                // to the packed triangle (as the packed epilogue below)
                float* T = Es;
                const int cb = (ch.k0 + ti) * UB + 4 * col4;
#pragma unroll
                for (int ai = 0; ai < 3; ++ai) {
                    store_frag_T(T, fp, ai == 0 ? kp : ai == 1 ? km : kv);
                    __syncthreads();
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int rr = ch.r0 + srow + 16 * j;
                        if (!rown[j] || cb >= rr) continue;
                        store_packed_run<1>({ai == 0 ? a.params : ai == 1 ? a.m : a.v},
                                            {*reinterpret_cast<const float4*>(&T[(srow + 16 * j) * TLD + 4 * col4])},
                                            rowp[j] + cb, cb, rr);
                    }
                    __syncthreads();
                }
            }
            return;
        }
        // D[i = c][j = r]: j = lane & 31, i = (q & 3) + 8 (q >> 2) + 4 h  ->  T[r][c] in Es
        float* T = Es;
        store_frag_T(T, fp, acc);
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        __syncthreads();
        const int cb = (ch.k0 + ti) * UB + 4 * col4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = ch.r0 + srow + 16 * j;
            if (!rown[j] || cb >= r || (a.abl & 8)) {
                if (FUSE)  // no L entries here: zeros for the fused sample GEMM
                    *reinterpret_cast<float4*>(&T[(srow + 16 * j) * TLD + 4 * col4]) = z4;
                continue;
            }
            const int o = rowp[j] + cb;
            const float4 d4 = *reinterpret_cast<const float4*>(&T[(srow + 16 * j) * TLD + 4 * col4]);
            const float4 p4 = (a.abl & 4) ? z4 : fix4(pq[j], o, 0, pcount);
            const float4 kv4 = (GRAD && a.kl_vec) ? fix4(ld4u(a.kl_vec, o, 0, pcount), o, 0, pcount) : z4;
            float4 m4 = z4, v4 = z4;
            if (!GRAD) {
                m4 = (a.abl & 4) ? z4 : fix4(mq[j], o, 0, pcount);
                v4 = (a.abl & 4) ? z4 : fix4(vq[j], o, 0, pcount);
            }
            float pn[4], mn[4], vn[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float p = f4get(p4, i);
                klp += cb + i < r ? p * p : 0.f;
                float gval = a.include_kl ? f4get(d4, i) + p * a.inv_s0sq : f4get(d4, i);
                if (GRAD && a.kl_vec) gval += f4get(kv4, i) * a.inv_s0sq;
                if (GRAD) {
                    pn[i] = gval;
                } else {
                    float mm = f4get(m4, i), vv = f4get(v4, i);
                    pn[i] = adam_apply_fast(a.adam, p, gval, mm, vv);
                    mn[i] = mm;
                    vn[i] = vv;
                }
            }
            if (FUSE) {  // L_new row segment (strict lower part only)
                float4 lv;
                lv.x = cb + 0 < r ? pn[0] : 0.f;
                lv.y = cb + 1 < r ? pn[1] : 0.f;
                lv.z = cb + 2 < r ? pn[2] : 0.f;
                lv.w = cb + 3 < r ? pn[3] : 0.f;
                *reinterpret_cast<float4*>(&T[(srow + 16 * j) * TLD + 4 * col4]) = lv;
            }
            float* dp = GRAD ? a.grad_out : a.params;
            if (cb + 3 < r) {
                *reinterpret_cast<float4*>(dp + o) = make_float4(pn[0], pn[1], pn[2], pn[3]);
                if (!GRAD) {
                    *reinterpret_cast<float4*>(a.m + o) = make_float4(mn[0], mn[1], mn[2], mn[3]);
                    *reinterpret_cast<float4*>(a.v + o) = make_float4(vn[0], vn[1], vn[2], vn[3]);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (cb + i < r) {
                        dp[o + i] = pn[i];
                        if (!GRAD) {
                            a.m[o + i] = mn[i];
                            a.v[o + i] = vn[i];
                        }
                    }
                }
            }
        }
    };

    if (!MULTI) {
        // all samples in one pass: the band's G slice stays in LDS, eps
        // comes in halves.  Loads are issued in the order they are consumed
        // (vmcnt retires in order): second eps half, this c-block's corr/m/v,
        // next c-block's first eps half -- the corr/m/v get both MFMA halves
        // to land.
        load_G(0);
        load_Eh(0, 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {  // G slice once (its registers die here)
            const int sr = srow + 16 * j;
            *reinterpret_cast<float4*>(&Gs[sr * ULD + 4 * col4]) =
                sr < a.S && !(a.abl & 1) ? fix4(greg[j], goff(sr), 0, g_total) : z4;
        }
        // diagnostics: shader-clock time per loop phase, summed over c-blocks
        // (slots 6..11: stage 1, MFMA half 1, stage 2, MFMA half 2, epilogue, gemm2)
        unsigned long long tph[6] = {0, 0, 0, 0, 0, 0}, tlast = 0;
        auto ph = [&](int k) {
            if (a.stamps && tid == 0) {
                const unsigned long long t = __builtin_amdgcn_s_memtime();
                if (k >= 0) tph[k] += t - tlast;
                tlast = t;
            }
        };
        ph(-1);
        for (int ti = 0; ti < nt; ++ti) {
            stage_Eh(ti, 0);
            __syncthreads();
            if (ti == 0) MVN_STAMP(1, __builtin_amdgcn_s_memtime());
            ph(0);
            if (TWOH) {
                load_Eh(ti, 1);
                load_pmv(ti);
                load_En(ti);
                compute_h(ti, 0);
                __syncthreads();
                ph(1);
                stage_Eh(ti, 1);
                __syncthreads();
                ph(2);
                load_Eh(min(ti + 1, nt - 1), 0);
                compute_h(ti, 1);
            } else {
                load_pmv(ti);
                load_En(ti);
                load_Eh(min(ti + 1, nt - 1), 0);
                compute_h(ti, 0);
            }
            __syncthreads();  // every wave done with Es: it takes the accumulator tile
            ph(3);
            epilogue(ti);
            if (FUSE) {
                __syncthreads();  // L_new tile complete
                ph(4);
                gemm2(ti);
            }
            __syncthreads();  // tile read before the next staging overwrites Es
            ph(FUSE ? 5 : 4);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) MVN_STAMP(6 + k, tph[k]);
    } else {
        load_G(0);
        load_E(0, 0);
        for (int ti = 0; ti < nt; ++ti) {
            for (int pi = 0; pi < np - 1; ++pi) {
                stage(true, ti, pi);
                __syncthreads();
                load_G(pi + 1);
                load_E(ti, pi + 1);
                compute(ti, pi);
                __syncthreads();
            }
            stage(true, ti, np - 1);
            __syncthreads();
            load_G(0);
            load_E(min(ti + 1, nt - 1), 0);
            load_pmv(ti);
            compute(ti, np - 1);
            __syncthreads();
            epilogue(ti);
            __syncthreads();
        }
    }
    MVN_STAMP(2, __builtin_amdgcn_s_memtime());
    if (FUSE && wave_s && ch.slot >= 0) {
        // D2[i = s][j = r]: j = lane & 31, i = (q & 3) + 8 (q >> 2) + 4 h
        float* slot = a.part + (size_t)ch.slot * a.S * 64 + l32;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int s = 32 * wv + (q & 3) + 8 * (q >> 2) + 4 * h;
                if (s < a.S) slot[(size_t)s * 64 + 32 * t] = acc2[t][q];
            }
    }
    klp *= 0.5f * a.inv_s0sq;
    if (ch.diag) {
        sh.red[wv * 64 + lane] = dgm;
        sh.red[256 + wv * 64 + lane] = dgs;
        __syncthreads();
        const int rr = ch.r0 + tid;
        if (tid < 64 && rr >= ch.rlo && rr < ch.rhi && rr < n) {
            const float* red = sh.red;
            const float gm = red[tid] + red[64 + tid] + red[128 + tid] + red[192 + tid];
            const float gs = red[256 + tid] + red[320 + tid] + red[384 + tid] + red[448 + tid];
            const int pm = poff + rr, ps = pm + n;
            float gmean, gsd;
            diag_head(a, a.params[pm], a.params[ps], gm, gs, gmean, gsd, klp);
            upd_elem<GRAD>(a, pm, gmean);
            upd_elem<GRAD>(a, ps, gsd);
        }
        __syncthreads();
    }
    if (a.kl_out && a.include_kl) {
        const float tot = block_sum(klp, sh.red);
        if (tid == 0) atomicAdd(a.kl_out, (double)tot);
    }
}

template <bool GRAD, int MODE, bool FUSE = false, bool TILED = false, bool PKO = false>
__global__ __launch_bounds__(256, MODE == 2 || FUSE ? 2 : 3) void mvn_update_kernel(UpdArgs a) {
    __shared__ __attribute__((aligned(16))) UpdShared<MODE == 2> sh;
    MVN_STAMP(0, __builtin_amdgcn_s_memtime());
    MVN_STAMP(12, __builtin_amdgcn_s_memrealtime());  // chip-wide 100 MHz clock
    MVN_STAMP(4, (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4));
    MVN_STAMP(5, (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20));
    const UpdChunk ch = a.chunks[blockIdx.x];
    if (ch.k1 > ch.k0) upd_chunk<GRAD, MODE, FUSE, TILED, PKO>(a, ch, sh);  // XCD padding chunks are empty
    MVN_STAMP(3, __builtin_amdgcn_s_memtime());
    MVN_STAMP(13, __builtin_amdgcn_s_memrealtime());
}

// packed <-> tiled corr / m / v: one workgroup per 64 x 64 tile.  The tile's
// 64 row segments are contiguous in the packed triangle (row r from poff + 2n +
// r (r - 1) / 2, columns c < r): they go through LDS (row stride 65) between
// row-major packed accesses and float4 fragment-order tiled accesses
// (fragment float4 q = (w * 4 + g) * 64 + lane holds row 32 (w >> 1) + (lane
// & 31), columns 32 (w & 1) + 8 g + 4 (lane >> 5) + 0..3).  Entries outside
// the triangle (or rows 0, n - 1) are zero in the tiled copy.
struct ConvArgs {
    float* pad[3];      // nullable: 64 floats to zero each (the inner loop's eps / G pads)
    float* params;
    float* m;
    float* v;
    float* tstate;      // [3][tiles_total * 4096]: p, m, v
    int64_t tfloats;    // tiles_total * 4096
    int L;
    MvnLayerArgs lay[kMaxL];
};

template <bool TO_TILED>
__global__ __launch_bounds__(256) void mvn_tile_convert_kernel(ConvArgs c) {
    __shared__ float T[64 * 65];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    if (TO_TILED && tile == 0 && tid < 192 && c.pad[tid >> 6]) c.pad[tid >> 6][tid & 63] = 0.f;
    int l = 0;
#pragma unroll
    for (int j = 1; j < kMaxL; ++j)
        if (j < c.L && tile >= c.lay[j].tbase) l = j;
    int n = c.lay[0].n;
    int64_t poff = c.lay[0].poff, tbase = c.lay[0].tbase;
#pragma unroll
    for (int j = 1; j < kMaxL; ++j)
        if (j == l) {
            n = c.lay[j].n;
            poff = c.lay[j].poff;
            tbase = c.lay[j].tbase;
        }
    const int64_t tb = tile - tbase;
    int b = (int)((sqrtf(8.f * (float)tb + 1.f) - 1.f) * 0.5f);
    while ((int64_t)(b + 1) * (b + 2) / 2 <= tb) ++b;
    while ((int64_t)b * (b + 1) / 2 > tb) --b;
    const int k = (int)(tb - (int64_t)b * (b + 1) / 2);
    // row-major side: thread -> (row 16 pass + tid / 16, columns 4 (tid % 16) + 0..3)
    const int cq = 4 * (tid & 15);
    // fragment side: thread -> float4 q = tid + 256 j
    float* arr[3] = {c.params, c.m, c.v};
#pragma unroll 1
    for (int ai = 0; ai < 3; ++ai) {
        float* A = arr[ai];
        float4* tt = reinterpret_cast<float4*>(c.tstate + ai * c.tfloats + tile * 4096);
        if (TO_TILED) {
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) {
                const int i = 16 * ps + (tid >> 4), r = 64 * b + i;
                const bool rv = r >= 1 && r <= n - 2;
                const int64_t rowp = poff + 2 * (int64_t)n + (int64_t)r * (r - 1) / 2 + 64 * k;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int cc = 64 * k + cq + e;
                    T[i * 65 + cq + e] = rv && cc < r ? A[rowp + cq + e] : 0.f;
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = tid + 256 * j, w = q >> 8, g = (q >> 6) & 3, lane = q & 63;
                const int i = 32 * (w >> 1) + (lane & 31), c0 = 32 * (w & 1) + 8 * g + 4 * (lane >> 5);
                tt[q] = make_float4(T[i * 65 + c0], T[i * 65 + c0 + 1], T[i * 65 + c0 + 2],
                                    T[i * 65 + c0 + 3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = tid + 256 * j, w = q >> 8, g = (q >> 6) & 3, lane = q & 63;
                const int i = 32 * (w >> 1) + (lane & 31), c0 = 32 * (w & 1) + 8 * g + 4 * (lane >> 5);
                const float4 v4 = tt[q];
                T[i * 65 + c0] = v4.x;
                T[i * 65 + c0 + 1] = v4.y;
                T[i * 65 + c0 + 2] = v4.z;
                T[i * 65 + c0 + 3] = v4.w;
            }
            __syncthreads();
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) {
                const int i = 16 * ps + (tid >> 4), r = 64 * b + i;
                const bool rv = r >= 1 && r <= n - 2;
                const int64_t rowp = poff + 2 * (int64_t)n + (int64_t)r * (r - 1) / 2 + 64 * k;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (rv && 64 * k + cq + e < r) A[rowp + cq + e] = T[i * 65 + cq + e];
            }
        }
        __syncthreads();  // T reused by the next array
    }
}

hipError_t launch_mvn_tile_convert(const psvi_plan& p, float* params, float* m, float* v,
                                   float* tstate, bool to_tiled, hipStream_t st, float* const* pads) {
    ConvArgs c{};
    for (int i = 0; i < 3; ++i) c.pad[i] = pads ? pads[i] : nullptr;
    c.params = params;
    c.m = m;
    c.v = v;
    c.tstate = tstate;
    c.tfloats = p.tiles_total * 4096;
    c.L = p.L;
    fill_layers(p, c.lay);
    if (c.tfloats == 0) return hipSuccess;
    const dim3 grid((unsigned)p.tiles_total);
    if (to_tiled)
        hipLaunchKernelGGL(mvn_tile_convert_kernel<true>, grid, dim3(256), 0, st, c);
    else
        hipLaunchKernelGGL(mvn_tile_convert_kernel<false>, grid, dim3(256), 0, st, c);
    return hipGetLastError();
}

// one <GRAD, FUSE, TILED, PKO> form at the request's MODE (samples per LDS
// pass; S > 128 exists for the plain packed forms only)
template <bool GRAD, bool FUSE = false, bool TILED = false, bool PKO = false>
static void launch_chunked(int mode, dim3 grid, hipStream_t st, const UpdArgs& a) {
    const dim3 block(256);
    if constexpr (!FUSE && !TILED) {
        if (mode == 2) {
            hipLaunchKernelGGL((mvn_update_kernel<GRAD, 2>), grid, block, 0, st, a);
            return;
        }
    }
    if (mode == 1) hipLaunchKernelGGL((mvn_update_kernel<GRAD, 1, FUSE, TILED, PKO>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((mvn_update_kernel<GRAD, 0, FUSE, TILED, PKO>), grid, block, 0, st, a);
}

// the streaming kernels exist for the trainers' variants (higher / hypergrad
// Adam) at S = 128 (C3 and the sharded C4 per-GPU count); other S take the
// chunked kernel (the stream kernel's narrower instantiations spilled their
// scalar registers to scratch)
static bool stream_ok(int S, int kind) {
    return S == 128 && (kind == PSVI_ADAM_HIGHER || kind == PSVI_ADAM_HYPERGRAD);
}
// gradient mode (the HVP's J^T G_dot) at any S on the bf16-piece K-split kernel
bool mvn_grad_takes_slots(const psvi_plan& p) {
    return p.n_kwg() > 0 && !g_diag.ks_off && !g_diag.ks_bf_off;
}

// Which kernel a request takes, in which form, and what follows it: decided
// here and nowhere else, at launch time (the request and g_diag's A/B switches).
static MvnRoute mvn_route(const psvi_plan& p, const MvnUpdate& r) {
    MvnRoute t{};
    const int S = p.d.S;
    t.mode = S > USB ? 2 : S > UEH ? 1 : 0;
    if (r.tstate) {
        // tiled state (psvi_inner_loop on a fusable plan): Adam only; with a next
        // step the streaming kernels, else (or switched off) the chunked forms
        t.tiled = true;
        const int kind = r.hp ? r.hp->kind : PSVI_ADAM_HIGHER;
        if (r.next.eps && p.str.n() > 0 && g_diag.stream_off != 1 && stream_ok(S, kind)) {
            const bool bf = r.eps_planes && r.next.planes && p.bf_stream && r.padded && !g_diag.stream_bf_off;
            t.kernel = bf ? MvnRoute::STREAM_BF : MvnRoute::STREAM_F32;
            t.fold = bf && p.str_cnt.dev && p.str_bms.dev && p.str_max_ends <= kFoldMax &&
                     !g_diag.stream_fold_off;
            t.after = t.fold ? MvnRoute::NONE : MvnRoute::REDUCE_SFRB;
            return t;
        }
        t.fuse = r.next.eps != nullptr;
        t.pko = !t.fuse && r.packed_out;
        t.after = t.fuse ? MvnRoute::REDUCE_UFRB : MvnRoute::NONE;
        return t;
    }
    t.grad = r.grad_out != nullptr;
    const bool ks_grad = t.grad && mvn_grad_takes_slots(p);
    if ((t.mode == 2 && !t.grad && p.n_kwg() > 0 && g_diag.ks_off != 1) || ks_grad) {
        // K = S > 128, or gradient mode on the slots; fp32 MFMAs for the A/B and the stamps
        t.kernel = MvnRoute::KSPLIT;
        t.bf = ks_grad || !(g_diag.ks_bf_off || g_diag.upd_stamps);
        t.after = r.next.eps ? MvnRoute::FWD : MvnRoute::NONE;
        return t;
    }
    if (r.next.eps && !t.grad) {
        // the fused sample where the plan has it, else the sample kernel on the new params
        t.fuse = p.fuse_sample && t.mode < 2;
        t.after = t.fuse ? MvnRoute::REDUCE_UFRB : MvnRoute::FWD;
    }
    return t;
}

hipError_t launch_mvn_update(const psvi_plan& p, const MvnUpdate& r, hipStream_t st) {
    if (p.upd.n() == 0) return hipSuccess;
    const MvnRoute t = mvn_route(p, r);
    // a second G slot is the K-split gradient kernel's alone
    if (r.g_shard2 && !r.tstate && !(t.kernel == MvnRoute::KSPLIT && t.grad)) return hipErrorInvalidValue;
    hipError_t e;
    if (t.kernel == MvnRoute::KSPLIT) {
        e = launch_mvn_kstream(p, r, t, st);
    } else if (t.kernel != MvnRoute::CHUNKED) {
        e = launch_mvn_stream(p, r, t, st);
    } else {
        UpdArgs a{};
        fill_update(p, r, a);
        fill_grad(p, r, a);
        fill_tiled(p, r, p.upd_part.dev, a);
        a.chunks = p.upd.dev;
        a.abl = g_diag.upd_ablation;
        const dim3 grid(p.upd.n());
        if (t.grad) launch_chunked<true>(t.mode, grid, st, a);
        else if (t.tiled && t.fuse) launch_chunked<false, true, true>(t.mode, grid, st, a);
        else if (t.tiled && t.pko) launch_chunked<false, false, true, true>(t.mode, grid, st, a);
        else if (t.tiled) launch_chunked<false, false, true>(t.mode, grid, st, a);
        else if (t.fuse) launch_chunked<false, true>(t.mode, grid, st, a);
        else launch_chunked<false>(t.mode, grid, st, a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    switch (t.after) {
    case MvnRoute::REDUCE_UFRB: return launch_next_reduce(p, r, p.ufrb.dev, p.ufrb.n(), p.upd_part.dev, st);
    case MvnRoute::REDUCE_SFRB: return launch_next_reduce(p, r, p.sfrb.dev, p.sfrb.n(), p.str_part.dev, st);
    case MvnRoute::FWD: return launch_mvn_fwd(p, r.next.eps, r.params, r.next.x, st);
    default: return hipSuccess;
    }
}

}  // namespace psvi
