// lds_shapes.cpp -- the shape solvers that size their row blocks from the LDS
// layouts (lds_layout.hpp): what is fixed and what a further row costs both
// come from the layout's walk.  Host only: no HIP call.
#include "lds_layout.hpp"

namespace psvi {

int mfvi_fit_shape(const psvi_net_desc& d, MfviFitShape& s) {
    s = MfviFitShape{};
    s.L = d.n_layers;
    s.B = d.M;
    s.S = d.S;
    int hmax = 1;
    for (int l = 0; l < s.L; ++l) {
        s.n_tot += d.dims[l] * d.dims[l + 1] + d.dims[l + 1];
        if (l > 0) hmax = std::max(hmax, d.dims[l]);
    }
    s.hs = hmax | 1;
    s.xs = d.dims[0] | 1;
    s.eps_count = (int64_t)s.S * s.n_tot;
    // the state and the batch stay in LDS when a chunk of min(B, 16) rows still fits beside them
    const int want = std::min(s.B, 16);
    for (int lds = 1; lds >= 0; --lds) {
        const size_t fixed = mffit_lds_bytes(s, lds != 0, 0);
        if (fixed >= kMfFitLds) continue;
        const size_t rows = (kMfFitLds - fixed) / (mffit_lds_bytes(s, lds != 0, 1) - fixed);
        if (rows < (size_t)(lds ? want : 1)) continue;
        s.lds = lds != 0;
        s.RB = (int)std::min<size_t>(rows, (size_t)s.B);
        s.ws_bytes = s.lds ? 0 : sizeof(float) * 2 * (size_t)s.n_tot;  // per member
        return 0;
    }
    return PSVI_EUNSUP;
}

RopGeometry rop_geometry(const psvi_plan& p) {
    RopGeometry g{};
    g.nsplit = rop_splits(p);
    const int rows_per = (p.d.M + g.nsplit - 1) / g.nsplit;
    // the matrix-core form when a row block fits the LDS in one pass, its rows
    // padded to a 16-multiple (the contraction over rows runs to it, over zeros)
    g.mfma_rows = (rows_per + 15) & ~15;
    g.mfma = rop_mfma_lds(p, g.mfma_rows);
    g.mfma_fits = g.mfma.bytes <= kRopLds;
    // VALU: the rows per chunk that fit beside the LDS gradient accumulators (a
    // power of two up to 64; none: unsupported) -- or a workgroup's rows in one
    // chunk when they fit without the accumulators (C3: 50 rows, 146 KB)
    int rc = 0;
    for (int r = 64; r >= 1 && !rc; r >>= 1)
        if (rop_valu_lds(p, r, true).bytes <= kRopLds) rc = r;
    if (!rc) return g;
    g.single = rop_valu_lds(p, rows_per, false).bytes <= kRopLds;
    g.valu = rop_valu_lds(p, g.single ? rows_per : rc, !g.single);
    return g;
}

int predict_shape(const psvi_plan& p, int64_t rpd, PredictShape& s) {
    s = PredictShape{};
    s.L = p.L;
    s.S = p.d.S;
    s.D = p.lay[0].din;
    s.C = p.lay[p.L - 1].dout;
    s.n_tot = p.n_tot;
    s.eps_count = p.Peps;
    int hmax = 1;
    for (int l = 0; l + 1 < p.L; ++l) hmax = std::max(hmax, p.lay[l].dout);
    s.hs = hmax | 1;
    s.xs = s.D | 1;
    // row groups of one eps block: even shares of at most kPredMaxRows rows,
    // halved until a tile of `want` units of every layer fits beside them
    const int64_t groups = (rpd + kPredMaxRows - 1) / kPredMaxRows;
    const int rg0 = (int)((rpd + groups - 1) / groups);
    for (int want : {16, 1})
        for (int rg = rg0;; rg = (rg + 1) / 2) {
            const size_t fixed = pred_lds_bytes(s, rg, 0);
            if (fixed < kPredLds) {
                const size_t cap = (kPredLds - fixed) / (pred_lds_bytes(s, rg, 1) - fixed);
                bool ok = true;
                size_t need = 0;
                for (int l = 0; l < p.L && ok; ++l) {
                    const size_t row = (size_t)p.lay[l].din + 1;
                    size_t ut = std::min<size_t>(cap / row, (size_t)p.lay[l].dout);
                    ok = ut >= (size_t)std::min(want, p.lay[l].dout);
                    // whole groups of four units, unless the tile is the whole layer
                    if (ut >= 4 && ut < (size_t)p.lay[l].dout) ut &= ~size_t(3);
                    s.ut[l] = (int)ut;
                    need = std::max(need, ut * row);
                }
                if (ok) {
                    s.RG = rg;
                    s.wcap = (int)need;
                    return 0;
                }
            }
            if (rg == 1) break;
        }
    return PSVI_EUNSUP;
}

}  // namespace psvi
