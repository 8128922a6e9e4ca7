// lds_layout.hpp -- the dynamic-LDS layout of every kernel that cuts its
// `extern __shared__` block into regions by shape: the single statement of the
// regions, their order and their extents.  The kernel runs its layout function
// on its LDS base and uses the pointers; the launcher and the shape solver run
// it on a null base for the bytes, so the size a launch asks for and the
// pointers the kernel forms come from the same walk.  The layouts: lap_fit_lds,
// lap_full_lds, giga_lds, mffit_lds, pred_lds, km_lds, and the R-op's
// rop_valu_lds / rop_mfma_lds, which yield float offsets that the plan holds
// and the kernels take as an argument.  (The network kernel likewise carries
// host-computed offsets: net_carve, kernels_net.hip.)
#pragma once
#include <utility>

#include "psvi_internal.hpp"

namespace psvi {

// WsCarve's counterpart for LDS: the regions in order, PACKED -- nothing is
// rounded up, so a layout's bank mapping and size are exactly its extents.
// Alignment is checked, not repaired: every layout takes its doubles first and
// its floats after from a 16-byte aligned base, and tests/cpp/plan_tables_check.cpp
// checks every region's alignment on the host.
// On the device the carve steps a typed pointer from region to region, the
// arithmetic the kernels wrote by hand before (32-bit LDS addressing, no null
// test); the byte count is kept on the host only, where bytes() serves the
// launchers and the shape solvers (on the device it reads 0).
struct LdsCarve {
    char* base;  // host: nullptr for sizes only (every region nullptr); device: the next region
    size_t off;
    __host__ __device__ explicit LdsCarve(void* b) : base(static_cast<char*>(b)), off(0) {}
    template <class T>
    __host__ __device__ T* take(size_t count) {
        static_assert(alignof(T) <= 16, "the base is 16-byte aligned");
#ifdef __HIP_DEVICE_COMPILE__
        T* r = reinterpret_cast<T*>(base);
        base = reinterpret_cast<char*>(r + count);
#else
        T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += sizeof(T) * count;
#endif
        return r;
    }
    __host__ __device__ size_t bytes() const { return off; }
};

// ------------------------------------------------------ kernels_laplace.hip
// laplace_fit_kernel<XLDS>; ds: the odd row stride of the staged x
struct LapFitLds {
    double *th, *part, *r;
    float* xs;
    size_t bytes;
};
__host__ __device__ inline LapFitLds lap_fit_lds(void* base, int Nu, int ds, bool xlds) {
    LdsCarve c(base);
    LapFitLds l;
    l.th = c.take<double>(2 * kLapMaxD);                        // [2][kLapMaxD]: theta, double-buffered
    l.part = c.take<double>(kLapThreads);                       // [kLapThreads]: the row owners' objective shares
    l.r = c.take<double>((size_t)Nu);                           // [Nu]: the per-row terms
    l.xs = c.take<float>(xlds ? (size_t)Nu * ds : 0);           // [Nu][ds]: x, XLDS only
    l.bytes = c.bytes();
    return l;
}
// x is staged when it fits beside the rest
inline bool lap_fit_xlds(int Nu, int ds) { return lap_fit_lds(nullptr, Nu, ds, true).bytes <= kLapLds; }

// laplace_sample_full_kernel; nb: the sample columns of the work area
struct LapFullLds {
    double *th, *P, *work;
    size_t bytes;
};
__host__ __device__ inline LapFullLds lap_full_lds(void* base, int Nu, int d, int nb) {
    LdsCarve c(base);
    LapFullLds l;
    l.th = c.take<double>((size_t)d);                           // [d]
    l.P = c.take<double>((size_t)d * (d + 1) / 2);              // [tri(d)]: P, then A, packed by rows
    l.work = c.take<double>((size_t)(Nu > nb * d ? Nu : nb * d));  // [max(Nu, nb * d)]: r, then y[i][column]
    l.bytes = c.bytes();
    return l;
}
// the sample columns that fit beside theta and the factor, one thread each
inline int lap_full_cols(int d, int S) {
    const size_t fixed = lap_full_lds(nullptr, 0, d, 0).bytes;
    const size_t col = lap_full_lds(nullptr, 0, d, 1).bytes - fixed;
    return std::min(std::min(kLapThreads, (int)((kLapLds - fixed) / col)), S);
}

// giga_step_kernel (its opt-in cap: the layout at kLapMaxRows, kSelMaxS)
struct GigaLds {
    double *mean, *inv, *b, *ell, *dd;
    size_t bytes;
};
__host__ __device__ inline GigaLds giga_lds(void* base, int N, int S) {
    LdsCarve c(base);
    GigaLds l;
    l.mean = c.take<double>((size_t)N);  // [N]: column means
    l.inv = c.take<double>((size_t)N);   // [N]: 1 / max(|cll_.n|, 1e-12)
    l.b = c.take<double>((size_t)N);     // [N]: ell_n . lw
    l.ell = c.take<double>((size_t)S);   // [S]
    l.dd = c.take<double>((size_t)S);    // [S]: d, then ell*
    l.bytes = c.bytes();
    return l;
}

// ----------------------------------------------------- kernels_mfvi_fit.hip
// mfvi_fit_kernel<LDS> at RB rows per chunk.  lds: the accumulators, the state
// and the batch live here (else in the workspace / the caller's arrays: null)
struct MfFitLds {
    double* red;
    float *Wb, *eb, *gmu, *grho, *sp, *sm, *sv, *xl, *h, *dA, *dB;
    size_t bytes;
};
__host__ __device__ inline MfFitLds mffit_lds(void* base, bool lds, int L, int B, int n_tot, int hs,
                                              int xs, int RB) {
    LdsCarve c(base);
    const size_t n = (size_t)n_tot, rows = (size_t)RB * hs;
    MfFitLds l;
    l.red = c.take<double>(kMfFitThreads);            // [kMfFitThreads]: the loss tree
    l.Wb = c.take<float>(n);                          // [n_tot]: W_s
    l.eb = c.take<float>(n);                          // [n_tot]: eps_s
    l.gmu = c.take<float>(lds ? n : 0);               // [n_tot]: sum_s dW_s
    l.grho = c.take<float>(lds ? n : 0);              // [n_tot]: sum_s dW_s eps_s
    l.sp = c.take<float>(lds ? 2 * n : 0);            // [2 n_tot]: params
    l.sm = c.take<float>(lds ? 2 * n : 0);            // [2 n_tot]: Adam m
    l.sv = c.take<float>(lds ? 2 * n : 0);            // [2 n_tot]: Adam v
    l.xl = c.take<float>(lds ? (size_t)B * xs : 0);   // [B][xs]: the batch
    l.h = c.take<float>((size_t)(L - 1) * rows);      // [L - 1][RB][hs]: activations
    l.dA = c.take<float>(rows);                       // [RB][hs]: a layer's delta
    l.dB = c.take<float>(rows);                       // [RB][hs]: the previous layer's
    if (!lds) l.gmu = l.grho = l.sp = l.sm = l.sv = l.xl = nullptr;
    l.bytes = c.bytes();
    return l;
}
inline size_t mffit_lds_bytes(const MfviFitShape& s, bool lds, int RB) {
    return mffit_lds(nullptr, lds, s.L, s.B, s.n_tot, s.hs, s.xs, RB).bytes;
}

// ------------------------------------------------------ kernels_predict.hip
// predict_scores_kernel at RG rows per group and a W tile of wcap floats
struct PredLds {
    double* red;
    float *Wt, *xin, *hA, *hB, *lg;
    size_t bytes;
};
__host__ __device__ inline PredLds pred_lds(void* base, int RG, int wcap, int xs, int hs, int C) {
    LdsCarve c(base);
    PredLds l;
    l.red = c.take<double>(2 * kPredThreads);         // [2][kPredThreads]: the statistics' tree
    l.Wt = c.take<float>((size_t)wcap);               // [wcap]: a tile's W_s rows, then its biases
    l.xin = c.take<float>((size_t)RG * xs);           // [RG][xs]: the group's rows
    l.hA = c.take<float>((size_t)RG * hs);            // [RG][hs]
    l.hB = c.take<float>((size_t)RG * hs);            // [RG][hs]
    l.lg = c.take<float>((size_t)RG * C);             // [RG][C]: sum over s of the logits
    l.bytes = c.bytes();
    return l;
}
inline size_t pred_lds_bytes(const PredictShape& s, int RG, int wcap) {
    return pred_lds(nullptr, RG, wcap, s.xs, s.hs, s.C).bytes;
}

// ------------------------------------------------------- kernels_kmeans.hip
// km_assign_kernel (rows: with its row tile) and km_sums_kernel (the centre
// tile alone, as the accumulators of km_accumulate)
struct KmLds {
    double* sC;
    float* sX;
    size_t bytes;
};
__host__ __device__ inline KmLds km_lds(void* base, int K, int DT, int XS, bool rows) {
    LdsCarve c(base);
    KmLds l;
    l.sC = c.take<double>((size_t)K * DT);                              // [K][DT]: centres / cluster sums
    l.sX = c.take<float>(rows ? (size_t)kKmRows * XS : 0);              // [kKmRows][XS]: a row tile
    l.bytes = c.bytes();
    return l;
}
// Columns of a tile: the largest DT <= D whose layout fits kKmLds.  With
// bytes(DT, XS) = DT c + XS x (c: a column of the centres, x: a column of the
// row tile) and XS = DT | 1 <= DT + 1, bytes <= DT (c + x) + x; so DT =
// (kKmLds - x) / (c + x) fits whichever way DT | 1 falls.  x = bytes(0, 1) and
// c + x = bytes(1, 1) are read off the walk.
inline int km_tile_cols(int D, int K) {
    const size_t x = km_lds(nullptr, K, 0, 1, true).bytes, cx = km_lds(nullptr, K, 1, 1, true).bytes;
    return (int)std::min<size_t>((size_t)D, (kKmLds - x) / cx);
}

// ---------------------------------------------------------- kernels_rop.hip
// The R-op kernels take their layout as float offsets in a kernel argument
// (RopValuLds, RopMfmaLds: psvi_internal.hpp), walked once per plan on the
// host by rop_geometry; the walk of the offsets is the walk of the bytes.
constexpr size_t kRopLds = 160 * 1024;
struct LdsFloats {
    size_t off = 0;
    int take(size_t nfl) { return (int)std::exchange(off, off + nfl); }
    int take4(size_t nfl) { return take((nfl + 3) & ~size_t(3)); }  // the next region 16-byte aligned
};

// net_rop_kernel at rc rows per chunk; with_g: the G / G_dot accumulators of
// rows in several chunks
inline RopValuLds rop_valu_lds(const psvi_plan& p, int rc, bool with_g) {
    LdsFloats c;
    RopValuLds v{};
    v.rc = rc;
    int maxd = 0, xtot = 0;
    for (int l = 0; l < p.L; ++l) {
        maxd = std::max(maxd, std::max(p.lay[l].din, p.lay[l].dout));
        v.ldw[l] = p.lay[l].din | 1;
        v.xo[l] = xtot;
        xtot += p.lay[l].dout * v.ldw[l] + p.lay[l].dout;
    }
    v.maxd = ((maxd + 3) & ~3) | 1;
    v.lx = c.take4(xtot);                                  // W_l rows, then b_l, layer by layer
    v.lxd = c.take4(xtot);                                 // their tangents
    v.lg = with_g ? c.take4(p.n_tot) : 0;                  // [n_tot]
    v.lgd = with_g ? c.take4(p.n_tot) : 0;                 // [n_tot]
    for (int l = 0; l <= p.L; ++l) {
        const int d = l < p.L ? p.lay[l].din : p.lay[p.L - 1].dout;
        v.lh[l] = c.take4((size_t)rc * d);                 // [rc][d]
        v.lhd[l] = c.take4((size_t)rc * d);                // [rc][d]
    }
    v.ld0 = c.take4((size_t)rc * v.maxd);                  // [rc][maxd] each
    v.ld1 = c.take4((size_t)rc * v.maxd);
    v.ldd0 = c.take4((size_t)rc * v.maxd);
    v.ldd1 = c.take4((size_t)rc * v.maxd);
    v.bytes = sizeof(float) * c.off;
    return v;
}

// net_rop_mfma_kernel for a row block of `rows`.  The activation regions come
// first, so a 16-row tile's over-read past a region's rows stays inside the
// allocation (tail slack when the weights after the last one are shorter than
// that).
inline RopMfmaLds rop_mfma_lds(const psvi_plan& p, int rows) {
    const int L = p.L;
    LdsFloats c;
    RopMfmaLds m{};
    for (int l = 0; l < L; ++l) m.kx[l] = (p.lay[l].din + 15) & ~15;
    m.kx[L] = (p.lay[L - 1].dout + 15) & ~15;
    for (int l = 0; l <= L; ++l) {
        m.ldxm[l] = 2 * m.kx[l] + 8;  // == 8 (mod 16); X_0's tangent half is zero
        m.mxo[l] = c.take((size_t)rows * m.ldxm[l]);       // [rows][ldxm]
    }
    const size_t x_end = c.off;
    for (int l = 0; l < L; ++l) {
        m.ldwm[l] = 2 * m.kx[l] + 8;
        m.mwo[l] = c.take((size_t)m.kx[l + 1] * m.ldwm[l]);  // [kx_{l+1}][ldwm]
    }
    for (int l = 0; l < L; ++l) m.mbo[l] = c.take(2 * (size_t)m.kx[l + 1]);
    const size_t over = (size_t)(((rows + 15) & ~15) - rows) * m.ldxm[L];
    if (c.off - x_end < over) c.off = x_end + over;
    c.off = (c.off + 3) & ~size_t(3);
    m.lstamp = c.take(20);  // 10 uint64 phase clocks (diagnostics)
    m.bytes = sizeof(float) * c.off;
    // the load jobs: a job is one row of up to 64 columns
    int j = 0;
    for (int l = 0; l < L; ++l) {
        m.jw[l] = j;
        j += m.kx[l + 1] * ((m.kx[l] + 63) >> 6);
    }
    m.jb = j;
    for (int l = 0; l < L; ++l) {
        m.jbl[l] = j - m.jb;
        j += (m.kx[l + 1] + 63) >> 6;
    }
    m.ju = j;
    return m;
}

}  // namespace psvi
