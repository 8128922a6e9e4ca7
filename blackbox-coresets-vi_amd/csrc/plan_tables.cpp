// plan_tables.cpp -- what a plan is made of, built on the host: the parameter
// layout, the sample and row shards, and the work lists of the full-cov
// kernels (forward items, update chunks, the streaming run table, the K-split
// and segmented-sample tables).  Launches nothing and calls no HIP API:
// capi_plan.cpp uploads the lists, tests/cpp/plan_tables_check.cpp checks them.
#include <algorithm>
#include <string>
#include <vector>

#include "psvi_internal.hpp"
#include "workspace.hpp"

namespace psvi {

PlanDebug g_plan_dbg;

namespace {

constexpr int kFwdKChunk = 256;  // columns of L per forward work item
constexpr int64_t kLenetRowFloats = 2 * 1176 + 400 * 2 + 120 * 2 + 84 * 2 + 10;  // per (s, m): P1, routed d P1, ...
constexpr int64_t kMaxOff = (int64_t(1) << 31) - 4096;  // the kernels' 32-bit offsets

int fail(std::string& err, int code, const char* msg) {
    err = msg;
    return code;
}

// Units [0, U) with cumulative costs cum[0 .. U] cut into nwg contiguous
// non-empty runs of about equal cost: run w is [cut[w], cut[w + 1]).
std::vector<int64_t> cut_runs(const std::vector<double>& cum, int nwg) {
    const int64_t U = (int64_t)cum.size() - 1;
    std::vector<int64_t> cut(nwg + 1, 0);
    cut[nwg] = U;
    for (int w = 1; w < nwg; ++w) {
        const double target = cum[U] * w / nwg;
        const int64_t t = (int64_t)(std::lower_bound(cum.begin(), cum.end(), target) - cum.begin());
        cut[w] = std::max(cut[w - 1] + 1, std::min(t, U - (nwg - w)));
    }
    return cut;
}

// XCD-aware placement: workgroup w runs on XCD w % 8 (round-robin dispatch),
// so XCD x takes the contiguous eighth [x per, (x + 1) per) of the run list --
// its bands' G slices and the eps columns up to its last band stay in that
// XCD's L2 instead of every XCD touching every band of both layers.  The run
// of workgroup w (a count that is no multiple of 8 keeps the list's order).
int xcd_run(int w, int nwg) { return nwg % 8 == 0 ? (w % 8) * (nwg / 8) + w / 8 : w; }

void shard_samples(psvi_plan& p) {
    const int S = p.d.S;
    for (int q = 0; q < p.world; ++q) {
        const int base = S / p.world, rem = S % p.world;
        p.s_cnt[q] = base + (q < rem ? 1 : 0);
        p.s_off[q] = q * base + std::min(q, rem);
    }
}

// Row shards.  World > 1 full-cov: whole 64-row bands, so that every rank's
// update and sample work is whole 64 x 64 tiles of L (a band split between
// two ranks would be computed by both).  Band b of a layer holds b + 1 tiles
// (its strict-lower triangle); the bands of all layers are dealt largest
// first to the least-loaded rank (ties: the lower rank), which balances the
// tile counts to within one small band (C4 at 8 ranks: 151..153 of 1,215
// tiles; a contiguous nnz split would make a rank compute up to 216 tiles
// because its partial edge bands count whole).  A rank's rows are the union
// of its bands -- runs of consecutive bands -- and its x-shard columns run
// layer-major in row order.  World 1 (and the replicated mean-field / LeNet
// rows): one run per layer.
void assign_rows(psvi_plan& p) {
    for (int q = 0; q < p.world; ++q) {
        p.rows_tot[q] = 0;
        p.runs[q].clear();
    }
    p.band_owner.clear();
    p.band_coloff.clear();
    int nbt = 0;
    for (int l = 0; l < p.L; ++l) {
        p.band_base[l] = nbt;
        nbt += (p.lay[l].n - 1) / 64 + 1;
    }
    p.band_base[p.L] = nbt;
    const bool banded = p.family == PSVI_FAMILY_FULLCOV && p.world > 1;
    std::vector<int> owner(nbt, 0);
    if (banded) {
        std::vector<int> order(nbt);
        std::vector<double> cost(nbt);
        for (int l = 0; l < p.L; ++l)
            for (int b = 0; b < p.band_base[l + 1] - p.band_base[l]; ++b)
                cost[p.band_base[l] + b] = b + 1.0;
        for (int i = 0; i < nbt; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
        std::vector<double> load(p.world, 0.0);
        for (int i : order) {
            const int q = (int)(std::min_element(load.begin(), load.end()) - load.begin());
            owner[i] = q;
            load[q] += cost[i];
        }
    }
    p.band_coloff.assign(nbt, 0);
    for (int q = 0; q < p.world; ++q)
        for (int l = 0; l < p.L; ++l) {
            const int n = p.lay[l].n;
            p.xcol_l[q][l] = p.rows_tot[q];
            for (int b = 0; 64 * b < n; ++b) {
                const int gb = p.band_base[l] + b;
                if (banded && owner[gb] != q) continue;
                const int r0 = 64 * b, r1 = std::min(n, r0 + 64);
                std::vector<ShardRun>& rv = p.runs[q];
                if (!rv.empty() && rv.back().layer == l && rv.back().hi == r0)
                    rv.back().hi = r1;
                else
                    rv.push_back(ShardRun{l, r0, r1, p.rows_tot[q]});
                p.band_coloff[gb] = p.rows_tot[q] - r0;
                p.rows_tot[q] += r1 - r0;
            }
        }
    p.band_owner = owner;
}

// Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8), each with
// its own L2.  Keep every band's chunks on one XCD (its G slice and the eps
// blocks it shares with neighbouring bands then stay in that L2): bands go
// greedily, largest first, to the least-loaded XCD; each XCD's chunks run
// largest first; the per-XCD queues are interleaved at stride 8 and padded
// with empty chunks (k0 == k1, no work).
std::vector<UpdChunk> xcd_order(const std::vector<UpdChunk>& in) {
    constexpr int kXcd = 8;
    auto work = [](const UpdChunk& c) { return (c.k1 - c.k0) + c.diag; };
    std::vector<std::vector<UpdChunk>> band;  // chunks of one (layer, r0)
    for (const UpdChunk& c : in) {
        if (band.empty() || band.back()[0].layer != c.layer || band.back()[0].r0 != c.r0)
            band.emplace_back();
        band.back().push_back(c);
    }
    std::vector<int> bw(band.size());
    for (size_t i = 0; i < band.size(); ++i)
        for (const UpdChunk& c : band[i]) bw[i] += work(c);
    std::vector<size_t> idx(band.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return bw[a] > bw[b]; });
    std::vector<std::vector<UpdChunk>> q(kXcd);
    std::vector<long> load(kXcd, 0);
    for (size_t i : idx) {
        const int x = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        load[x] += bw[i];
        q[x].insert(q[x].end(), band[i].begin(), band[i].end());
    }
    size_t len = 0;
    for (auto& v : q) {
        std::stable_sort(v.begin(), v.end(),
                         [&](const UpdChunk& a, const UpdChunk& b) { return work(a) > work(b); });
        len = std::max(len, v.size());
    }
    std::vector<UpdChunk> out;
    out.reserve(len * kXcd);
    const UpdChunk empty{0, 0, 0, 0, 0, 0, 0, 0, -1};
    for (size_t j = 0; j < len; ++j)
        for (int x = 0; x < kXcd; ++x) out.push_back(j < q[x].size() ? q[x][j] : empty);
    return out;
}

// Forward items, their row blocks, and the update chunks of the rank's rows.
void build_fwd_upd(psvi_plan& p) {
    const int r = p.rank;
    std::vector<FwdItem>& fwd = p.fwd.host;
    std::vector<UpdChunk> upd;
    int nslots = 0;
    // c-blocks per update chunk: about one chunk per workgroup slot
    // (256 CUs x 3 resident update workgroups), at least one
    int tiles = 0;
    for (const ShardRun& run : p.runs[r])
        for (int b = run.lo / 64; 64 * b < run.hi; ++b) tiles += b + 1;
    const int ch = g_plan_dbg.upd_chunk_tiles > 0 ? g_plan_dbg.upd_chunk_tiles
                                                  : std::max(1, (tiles + 511) / 512);
    for (const ShardRun& run : p.runs[r]) {
        const int l = run.layer, n = p.lay[l].n, lo = run.lo, hi = run.hi;
        const int xc = run.col;
        for (int r0 = lo; r0 < hi; r0 += kFwdRows) {
            const int r1 = std::min(r0 + kFwdRows, hi);
            const int kmax = std::max(0, std::min(r1 - 1, n - 2));
            const int nit = std::max(1, (kmax + kFwdKChunk - 1) / kFwdKChunk);
            // even split, multiples of 64 columns (the kernel's LDS stage)
            const int steps = (kmax + 63) / 64;
            const int slot0 = (int)fwd.size();
            for (int i = 0; i < nit; ++i) {
                const int k0 = std::min(kmax, 64 * (int)((int64_t)steps * i / nit));
                const int k1 = std::min(kmax, 64 * (int)((int64_t)steps * (i + 1) / nit));
                if (i > 0 && k0 >= k1) continue;
                fwd.push_back(FwdItem{l, r0, r1, k0, k1, xc + (r0 - lo), (int)fwd.size()});
            }
            p.frb.host.push_back(
                FwdRowBlock{slot0, (int)fwd.size() - slot0, r1 - r0, xc + (r0 - lo), l, r0});
        }
        // bands of 64 absolute rows; c-blocks 0..b, the last one diagonal.
        // Each band is also a row block of the fused next-step sample: its
        // chunks' partial slots are consecutive.
        for (int b = lo / 64; 64 * b < hi; ++b) {
            const int slot0 = nslots;
            for (int k0 = 0; k0 <= b; k0 += ch) {
                const int k1 = std::min(b + 1, k0 + ch);
                upd.push_back(UpdChunk{l, 64 * b, k0, k1, lo, hi, xc - lo, k1 == b + 1, nslots++});
            }
            const int r0 = std::max(64 * b, lo), r1 = std::min(64 * b + 64, hi);
            p.ufrb.host.push_back(FwdRowBlock{slot0, nslots - slot0, r1 - r0, xc + (r0 - lo), l, r0});
        }
    }
    // longest forward items first
    std::stable_sort(fwd.begin(), fwd.end(), [](const FwdItem& a, const FwdItem& b) {
        return (a.k1 - a.k0) > (b.k1 - b.k0);
    });
    p.upd.host = xcd_order(upd);
    p.n_uslots = nslots;
    p.upd_tiles = tiles;
}

// Streaming fused update: the tile list (layer-major, band-major, the
// diagonal tile last in its band) cut into equal contiguous runs, one
// per workgroup (one workgroup per CU)
void build_stream(psvi_plan& p) {
    const int r = p.rank;
    std::vector<uint32_t> tmap;
    std::vector<int> tband;  // band id per tile
    int nband = 0;
    for (int l = 0; l < p.L; ++l)
        for (int b = 0; b < p.lay[l].nb; ++b, ++nband)
            for (int k = 0; k <= b; ++k) {
                tmap.push_back((uint32_t)l << 28 | (uint32_t)b << 14 | (uint32_t)k);
                tband.push_back(nband);
            }
    const int T = (int)tmap.size();
    const int nwg = std::max(1, std::min(g_plan_dbg.stream_wgs > 0 ? g_plan_dbg.stream_wgs : 256, T));
    // equal-cost runs: a band's diagonal (last) tile also updates the
    // band's mean / sd, flushes its slot, drains and takes the band's
    // ticket (and, for the last arriver, the combine after the walk); a
    // band's first tile follows a G reload and split.  Weights 1.5 and
    // 1.0 of a plain tile: the fastest of a sweep at C3
    // (tools/stream_cost_sweep.py: 55.7 - 56.3 us per step against 58.4
    // at the round-5 weights 0.35 / 0.4, which predate the in-kernel
    // combine); workgroup stamps (tools/bf_stamps.py) show the slowest
    // workgroups are the ones with band boundaries
    const int cost = g_plan_dbg.stream_cost;
    std::vector<double> cum(T + 1, 0.0);
    for (int t = 0; t < T; ++t) {
        const uint32_t k = tmap[t] & 0x3fff, b = (tmap[t] >> 14) & 0x3fff;
        const double wd = cost >= 0 ? (cost / 1000) * 0.01 : 1.5;
        const double wf = cost >= 0 ? (cost % 1000) * 0.01 : 1.0;
        cum[t + 1] = cum[t] + 1.0 + (k == b ? wd : 0.0) + (k == 0 ? wf : 0.0);
    }
    const std::vector<int64_t> cut = cut_runs(cum, nwg);
    std::vector<StreamRange> runs;
    std::vector<std::vector<int>> band_slots(nband);
    int ns = 0;
    for (int w = 0; w < nwg; ++w) {
        const int t0 = (int)cut[w], t1 = (int)cut[w + 1];
        runs.push_back(StreamRange{t0, t1, ns, t0 < T ? tmap[t0] : 0u});
        int ends = 0;
        for (int t = t0; t < t1; ++t)
            if (t == t0 || tband[t] != tband[t - 1]) {
                band_slots[tband[t]].push_back(ns++);
                ++ends;
            }
        p.str_max_ends = std::max(p.str_max_ends, ends);
    }
    int bid = 0;
    for (int l = 0; l < p.L; ++l)
        for (int b = 0; b < p.lay[l].nb; ++b, ++bid) {
            const int r0 = 64 * b, R = std::min(64, p.lay[l].n - r0);
            const auto& sl = band_slots[bid];
            p.sfrb.host.push_back(
                FwdRowBlock{sl.front(), (int)sl.size(), R, p.xcol_l[r][l] + r0, l, r0});
        }
    // workgroup w takes run xcd_run(w)
    for (int w = 0; w < nwg; ++w)
        p.str.host.push_back(runs[g_plan_dbg.stream_rr ? w : xcd_run(w, nwg)]);
    p.n_sslots = ns;
}

// K-split streaming update tables (S > 128): the rank's tiles band-major
// (the diagonal tile last in its band), units (tile, 128-sample pass) cut
// into equal-cost contiguous runs -- a tile's last unit also carries its
// Adam epilogue (about half a pass) -- one run per workgroup, two workgroups
// per CU.  XCD-aware placement as the stream kernel: workgroup w runs on XCD
// w % 8, so XCD x takes a contiguous eighth of the run list (its bands' G
// slices and eps column blocks stay in that XCD's L2).
void build_kstream(psvi_plan& p) {
    const int r = p.rank, np = (p.d.S + kKsPass - 1) / kKsPass;
    std::vector<KsTile>& tiles = p.ks_tiles.host;
    tiles.clear();
    for (const ShardRun& run : p.runs[r])
        for (int b = run.lo / 64; 64 * b < run.hi; ++b)
            for (int k = 0; k <= b; ++k)
                tiles.push_back(KsTile{run.layer, 64 * b, k, k == b, 64 * b,
                                       std::min(64 * b + 64, p.lay[run.layer].n), run.col - run.lo, -1});
    const int T = (int)tiles.size();
    std::vector<KsSeg>& segs = p.ks_segs.host;
    std::vector<int>& off = p.ks_off.host;
    segs.clear();
    off.clear();
    p.n_ks_slots = p.n_ks_cnt = 0;
    if (T == 0) return;
    const int64_t U = (int64_t)T * np;
    int nwg = (int)std::min<int64_t>(U, g_plan_dbg.ks_wgs > 0 ? g_plan_dbg.ks_wgs : 512);
    if (nwg >= 8) nwg -= nwg % 8;
    // unit cost: 1 per pass, + 0.5 on a tile's last pass (its epilogue)
    std::vector<double> cum(U + 1, 0.0);
    for (int64_t u = 0; u < U; ++u) cum[u + 1] = cum[u] + 1.0 + (u % np == np - 1 ? 0.5 : 0.0);
    const std::vector<int64_t> cut = cut_runs(cum, nwg);
    // contributors per tile
    std::vector<int> ncon(T, 0);
    for (int w = 0; w < nwg; ++w)
        for (int64_t u = cut[w]; u < cut[w + 1];) {
            const int t = (int)(u / np);
            ++ncon[t];
            u = std::min<int64_t>(cut[w + 1], (int64_t)(t + 1) * np);
        }
    std::vector<int> slot0(T, -1), seen(T, 0);
    for (int t = 0; t < T; ++t)
        if (ncon[t] > 1) {
            slot0[t] = p.n_ks_slots;
            p.n_ks_slots += ncon[t];
            tiles[t].cnt = p.n_ks_cnt++;
        }
    std::vector<std::vector<KsSeg>> per(nwg);
    for (int w = 0; w < nwg; ++w)
        for (int64_t u = cut[w]; u < cut[w + 1];) {
            const int t = (int)(u / np);
            const int64_t ue = std::min<int64_t>(cut[w + 1], (int64_t)(t + 1) * np);
            per[w].push_back(KsSeg{t, (int)(u - (int64_t)t * np), (int)(ue - (int64_t)t * np),
                                   slot0[t], ncon[t], seen[t]++});
            u = ue;
        }
    off.push_back(0);
    for (int w = 0; w < nwg; ++w) {
        const auto& v = per[xcd_run(w, nwg)];
        segs.insert(segs.end(), v.begin(), v.end());
        off.push_back((int)segs.size());
    }
}

// Segmented sample tables (S > 128): units (row block of 64, 128-sample pass,
// 64-column block of L) ordered row block-major, then pass, then column block
// (a run accumulates x over consecutive column blocks of one (row block,
// pass)); equal-count contiguous runs, one per workgroup, two workgroups per
// CU; a run's piece of one (row block, pass) is a segment writing its own
// slot, and the reduce adds a (row block, pass)'s slots in segment order.
// XCD placement as the K-split update: workgroup w -> run xcd_run(w).
// One table for nwg_max workgroups (into segs / off / rbs and the slot count).
void build_fseg_table(const psvi_plan& p, int nwg_max, std::vector<FsSeg>& segs,
                      std::vector<int>& off, std::vector<FwdRowBlock>& rbs, int& n_slots) {
    const int r = p.rank, np = (p.d.S + kKsPass - 1) / kKsPass;
    struct Blk {
        int layer, r0, r1, xcol, nkb;
    };
    std::vector<Blk> blks;
    for (const ShardRun& run : p.runs[r]) {
        const int n = p.lay[run.layer].n;
        for (int r0 = run.lo; r0 < run.hi; r0 += kFwdRows) {
            const int r1 = std::min(r0 + kFwdRows, run.hi);
            const int kmax = std::max(0, std::min(r1 - 1, n - 2));
            blks.push_back(Blk{run.layer, r0, r1, run.col + (r0 - run.lo), (kmax + 63) / 64});
        }
    }
    segs.clear();
    off.clear();
    rbs.clear();
    n_slots = 0;
    const int B = (int)blks.size();
    std::vector<int64_t> ub(B + 1, 0);
    for (int b = 0; b < B; ++b) ub[b + 1] = ub[b] + (int64_t)blks[b].nkb * np;
    const int64_t U = ub[B];
    if (U == 0) return;
    int nwg = (int)std::min<int64_t>(U, nwg_max);
    if (nwg >= 8) nwg -= nwg % 8;
    std::vector<int64_t> cut(nwg + 1);
    for (int w = 0; w <= nwg; ++w) cut[w] = U * w / nwg;
    // segments per workgroup; group g = b * np + pass
    struct Piece {
        int b, pass, kb0, kb1;
    };
    std::vector<std::vector<Piece>> per(nwg);
    std::vector<int> nseg((size_t)B * np, 0);
    for (int w = 0; w < nwg; ++w) {
        int b = (int)(std::upper_bound(ub.begin(), ub.end(), cut[w]) - ub.begin()) - 1;
        for (int64_t u = cut[w]; u < cut[w + 1];) {
            while (u >= ub[b + 1]) ++b;
            const int nkb = blks[b].nkb;
            const int pass = (int)((u - ub[b]) / nkb), kb = (int)((u - ub[b]) % nkb);
            const int64_t ue = std::min<int64_t>(cut[w + 1], ub[b] + (int64_t)(pass + 1) * nkb);
            per[w].push_back(Piece{b, pass, kb, kb + (int)(ue - u)});
            ++nseg[(size_t)b * np + pass];
            u = ue;
        }
    }
    std::vector<int> slot0((size_t)B * np), seen((size_t)B * np, 0);
    for (int b = 0; b < B; ++b)
        for (int q = 0; q < np; ++q) {
            const size_t g = (size_t)b * np + q;
            slot0[g] = n_slots;
            n_slots += nseg[g];
            rbs.push_back(FwdRowBlock{nseg[g] > 0 ? slot0[g] : 0, nseg[g], blks[b].r1 - blks[b].r0,
                                            blks[b].xcol, blks[b].layer, blks[b].r0, kKsPass * q});
        }
    off.push_back(0);
    for (int w = 0; w < nwg; ++w) {
        for (const Piece& pc : per[xcd_run(w, nwg)]) {
            const Blk& bk = blks[pc.b];
            const size_t g = (size_t)pc.b * np + pc.pass;
            segs.push_back(FsSeg{bk.layer, bk.r0, bk.r1, pc.pass, 64 * pc.kb0, 64 * pc.kb1,
                                 slot0[g] + seen[g]++, 0});
        }
        off.push_back((int)segs.size());
    }
}

// The sample's table over 512 workgroups (two per CU), and the HVP pair's over
// 256 (one eight-wave workgroup per CU: runs twice as long, fewer slots).
void build_fseg(psvi_plan& p) {
    build_fseg_table(p, 512, p.fs_segs.host, p.fs_off.host, p.fs_rb.host, p.n_fs_slots);
    build_fseg_table(p, 256, p.fp_segs.host, p.fp_off.host, p.fp_rb.host, p.n_fp_slots);
}

// The bf16 planes of a draw (EpsPlanes): rows padded to 64-column
// multiples, layers back to back -- the streaming update's operands
// (bf_stream: the plans that run it), and for every plan the layout
// of the diagnostics planes (PSVI_DBG_NET_DRAW_PLANES)
void layout_eps_planes(psvi_plan& p) {
    EpsPlanes& E = p.eps_planes;
    E.L = p.L;
    int64_t po = 0, eo = 0;
    for (int l = 0; l < p.L; ++l) {
        const int n = p.lay[l].n;
        E.eoff[l] = eo;
        E.n[l] = n;
        E.npad[l] = (n + 63) / 64 * 64;
        E.poff[l] = po;
        eo += (int64_t)p.d.S * n;
        po += (int64_t)p.d.S * E.npad[l];
    }
    E.eoff[p.L] = eo;
    E.pl = (po + 63) / 64 * 64;
    p.eps_planes_ok = eo == p.Peps;
    p.bf_stream = p.eps_planes_ok && p.fuse_sample && p.tiles_total > 0 && p.str.n() > 0 &&
                  p.d.S == 128;
}

// make_lenet (neural_net.py:334-359): five mean-field-style layers, the first
// two convolutions ("din" = in_channels * 25), the last one a single shared
// sample.  Samples are sharded like the mean-field family.
int build_lenet_plan(psvi_plan& p, std::string& err) {
    static const int din[5] = {25, 150, 400, 120, 84}, dout[5] = {6, 16, 120, 84, 10};
    const int S = p.d.S;
    p.d.n_layers = 5;
    p.d.dims[0] = 784;
    for (int l = 0; l < 5; ++l) p.d.dims[l + 1] = dout[l];
    p.L = 5;
    int64_t po = 0, eo = 0;
    int wo = 0;
    for (int l = 0; l < 5; ++l) {
        LayerInfo& li = p.lay[l];
        li.din = din[l];
        li.dout = dout[l];
        li.n = din[l] * dout[l] + dout[l];
        li.nc = 0;
        li.poff = po;
        li.eoff = eo;
        li.woff = wo;
        po += 2 * (int64_t)li.n;
        eo += (l < 4 ? (int64_t)S : 1) * li.n;
        wo += li.n;
    }
    p.P = po;
    p.Peps = eo;
    p.n_tot = wo;
    shard_samples(p);
    for (int q = 0; q < p.world; ++q) p.rows_tot[q] = 0;
    p.acc_count = 2 * (int64_t)p.n_tot;
    p.ws_bytes = step_ws(p, nullptr).bytes;
    if (p.Peps > kMaxOff || (int64_t)p.s_cnt[p.rank] * p.d.M * kLenetRowFloats > kMaxOff * 4)
        return fail(err, PSVI_EUNSUP, "LeNet scratch beyond the supported size");
    return 0;
}

// Layer offsets in the parameter, eps and weight spaces, the tiled layout's
// tile bases, and the sample and row shards.
void layout_plan(psvi_plan& p) {
    const psvi_net_desc& d = p.d;
    p.L = d.n_layers;
    int64_t po = 0, eo = 0;
    int wo = 0;
    for (int l = 0; l < p.L; ++l) {
        LayerInfo& li = p.lay[l];
        li.din = d.dims[l];
        li.dout = d.dims[l + 1];
        li.n = li.din * li.dout + li.dout;
        li.nc = (int64_t)(li.n - 1) * (li.n - 2) / 2;
        li.poff = po;
        li.eoff = eo;
        li.woff = wo;
        po += p.family == PSVI_FAMILY_MEANFIELD ? 2 * (int64_t)li.n : 2 * (int64_t)li.n + li.nc;
        eo += (int64_t)d.S * li.n;
        wo += li.n;
    }
    p.P = po;
    p.Peps = eo;
    int64_t tb = 0;
    for (int l = 0; l < p.L; ++l) {
        LayerInfo& li = p.lay[l];
        li.nb = p.family == PSVI_FAMILY_FULLCOV ? (li.n - 1) / 64 + 1 : 0;
        li.tbase = tb;
        tb += (int64_t)li.nb * (li.nb + 1) / 2;
    }
    p.tiles_total = tb;
    p.n_tot = wo;
    shard_samples(p);
    assign_rows(p);
    p.acc_count = 2 * (int64_t)p.n_tot;
}

// the kernels address parameters, eps and the x / g shards with 32-bit offsets
bool sizes_ok(const psvi_plan& p) {
    int rows_max = 0;
    for (int q = 0; q < p.world; ++q) rows_max = std::max(rows_max, p.rows_tot[q]);
    return !(p.P > kMaxOff || p.Peps > kMaxOff || (int64_t)p.d.S * rows_max > kMaxOff ||
             (int64_t)p.d.S * p.n_tot > kMaxOff);
}

}  // namespace

int build_plan(psvi_plan& p, std::string& err) {
    if (p.family == PSVI_FAMILY_LENET) return build_lenet_plan(p, err);
    layout_plan(p);
    net_plan_geometry(p);
    if (p.net_lds > 160 * 1024)
        return fail(err, PSVI_EUNSUP, "layer too wide for the per-sample LDS network kernel");
    if (!sizes_ok(p)) return fail(err, PSVI_EUNSUP, "buffers beyond 2^31 floats are not supported");
    p.ws_bytes = step_ws(p, nullptr).bytes;
    p.rop = rop_geometry(p);
    if (p.family != PSVI_FAMILY_FULLCOV) return 0;
    const int S = p.d.S;
    build_fwd_upd(p);
    // fusion needs band-aligned row blocks (rank row ranges start at 0) and
    // one LDS pass of samples
    p.fuse_sample = p.world == 1 && S <= 128;
    if (p.fuse_sample && S % 32 == 0) build_stream(p);
    // the K-split tables at every S: the Adam update at S > 128, the
    // gradient mode (the HVP's reparameterised backward) at any S
    build_kstream(p);
    // the segmented sample at every S (x_0 of a loop, the HVP's tangent
    // sample, the sharded step): equal runs over 512 workgroups
    build_fseg(p);
    if (p.world == 1) layout_eps_planes(p);
    return 0;
}

}  // namespace psvi
