// plan_tables_check.cpp -- stand-alone check of the work lists plan_tables.cpp
// builds (no GPU use): every plan of a list of shapes is built on the host and
// its tables are checked against what the kernels assume of them; every
// workspace layout (workspace.hpp) is carved on a buffer of exactly the size it
// reports and its regions are checked to lie inside, apart and aligned; every
// kernel's dynamic-LDS layout (lds_layout.hpp) is held to the byte count it had
// before that header and walked on a buffer of exactly that size; the R-op's
// geometry (psvi_plan::rop) is held to the recorded fixture given as the one
// argument and its two layouts are walked likewise.  Built with
// the host sanitizers by `make check-tables`; exit status 0 when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "lds_layout.hpp"
#include "workspace.hpp"

using namespace psvi;

// Stand-in for the network kernel's LDS geometry (kernels_net.hip): one chunk
// of all M pseudopoints, no LDS demand.  No table depends on it.
namespace psvi {
size_t net_plan_geometry(psvi_plan& p) {
    p.net_roles = 1;
    p.mchunks = 1;
    p.mc = p.d.M;
    p.net_threads = 256;
    p.net_mloop = false;
    p.net_lds = 0;
    return 0;
}
}  // namespace psvi

namespace {

int g_failed = 0;
std::string g_what;  // the plan under check

#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            if (++g_failed <= 50)                                                         \
                std::fprintf(stderr, "%s:%d: [%s] %s\n", __FILE__, __LINE__, g_what.c_str(), #cond); \
            return;                                                                       \
        }                                                                                 \
    } while (0)

// the run of workgroup w, as the tables place them on the XCDs
int xcd_run(int w, int nwg) { return nwg % 8 == 0 ? (w % 8) * (nwg / 8) + w / 8 : w; }

struct Band {
    int layer, b;
};
// the rank's 64-row bands, in run order
std::vector<Band> rank_bands(const psvi_plan& p) {
    std::vector<Band> v;
    for (const ShardRun& run : p.runs[p.rank])
        for (int b = run.lo / 64; 64 * b < run.hi; ++b) v.push_back(Band{run.layer, b});
    return v;
}
// column of absolute row r of a layer in the rank's x shard (-1: not the rank's)
int xcol_of(const psvi_plan& p, int layer, int r) {
    for (const ShardRun& run : p.runs[p.rank])
        if (run.layer == layer && r >= run.lo && r < run.hi) return run.col + (r - run.lo);
    return -1;
}

bool all_fullcov_tables_empty(const psvi_plan& p) {
    return p.fwd.n() == 0 && p.frb.n() == 0 && p.upd.n() == 0 && p.ufrb.n() == 0 && p.str.n() == 0 &&
           p.sfrb.n() == 0 && p.ks_tiles.n() == 0 && p.ks_segs.n() == 0 && p.ks_off.n() == 0 &&
           p.fs_segs.n() == 0 && p.fs_off.n() == 0 && p.fs_rb.n() == 0 && p.fp_segs.n() == 0 &&
           p.fp_off.n() == 0 && p.fp_rb.n() == 0 && p.n_uslots == 0 && p.n_sslots == 0 &&
           p.n_ks_slots == 0 && p.n_ks_cnt == 0 && p.n_fs_slots == 0 && p.n_fp_slots == 0 &&
           p.str_max_ends == 0 && p.upd_tiles == 0 && p.n_kwg() == 0 && p.n_fswg() == 0 &&
           p.n_fpwg() == 0 && !p.fuse_sample && !p.bf_stream && !p.eps_planes_ok;
}

// ---------------------------------------------------------- streaming table
void check_stream(const psvi_plan& p, bool rr) {
    const bool expect = p.world == 1 && p.d.S <= 128 && p.d.S % 32 == 0;
    if (!expect) {
        CHECK(p.str.n() == 0 && p.sfrb.n() == 0 && p.n_sslots == 0 && p.str_max_ends == 0);
        return;
    }
    // the tile list: layer-major, band-major, the diagonal tile last
    std::vector<uint32_t> lbk;
    std::vector<int> tband;
    std::vector<Band> bands;
    for (int l = 0; l < p.L; ++l)
        for (int b = 0; b < p.lay[l].nb; ++b) {
            for (int k = 0; k <= b; ++k) {
                lbk.push_back((uint32_t)l << 28 | (uint32_t)b << 14 | (uint32_t)k);
                tband.push_back((int)bands.size());
            }
            bands.push_back(Band{l, b});
        }
    const int T = (int)lbk.size(), nwg = p.str.n();
    CHECK(T == p.tiles_total && nwg >= 1 && nwg <= T);
    // the XCD order undone
    std::vector<StreamRange> runs(nwg);
    std::vector<bool> set(nwg, false);
    for (int w = 0; w < nwg; ++w) {
        const int i = rr ? w : xcd_run(w, nwg);
        CHECK(i >= 0 && i < nwg && !set[i]);
        set[i] = true;
        runs[i] = p.str.host[w];
    }
    // non-empty, disjoint, covering [0, T); slots consecutive, one per band touched
    std::vector<std::vector<int>> band_slots(bands.size());
    int t = 0, slot = 0, max_ends = 0;
    for (const StreamRange& r : runs) {
        CHECK(r.t0 == t && r.t1 > r.t0 && r.t1 <= T);
        CHECK(r.lbk0 == lbk[r.t0]);
        CHECK(r.slot0 == slot);
        const int touched = tband[r.t1 - 1] - tband[r.t0] + 1;
        for (int j = 0; j < touched; ++j) band_slots[tband[r.t0] + j].push_back(r.slot0 + j);
        slot += touched;
        max_ends = std::max(max_ends, touched);
        t = r.t1;
    }
    CHECK(t == T);
    CHECK(slot == p.n_sslots);
    CHECK(max_ends == p.str_max_ends);
    // band row blocks: nk = the runs touching the band, on consecutive slots
    CHECK(p.sfrb.n() == (int)bands.size());
    int nk_sum = 0;
    for (size_t i = 0; i < bands.size(); ++i) {
        const FwdRowBlock& rb = p.sfrb.host[i];
        const std::vector<int>& sl = band_slots[i];
        CHECK(rb.nk == (int)sl.size() && rb.nk >= 1);
        for (int j = 0; j < rb.nk; ++j) CHECK(sl[j] == rb.slot0 + j);
        CHECK(rb.layer == bands[i].layer && rb.r0 == 64 * bands[i].b);
        CHECK(rb.R == std::min(64, p.lay[rb.layer].n - rb.r0) && rb.R >= 1);
        CHECK(rb.xcol == xcol_of(p, rb.layer, rb.r0) && rb.s0 == 0);
        nk_sum += rb.nk;
    }
    CHECK(nk_sum == p.n_sslots);
}

// ------------------------------------------------------------ K-split table
void check_kstream(const psvi_plan& p) {
    const int np = (p.d.S + kKsPass - 1) / kKsPass;
    const std::vector<Band> bands = rank_bands(p);
    // the rank's tiles, band-major, the diagonal tile last
    size_t T = 0;
    for (const Band& bd : bands) T += bd.b + 1;
    CHECK((size_t)p.ks_tiles.n() == T);
    {
        size_t t = 0;
        for (const Band& bd : bands)
            for (int k = 0; k <= bd.b; ++k, ++t) {
                const KsTile& kt = p.ks_tiles.host[t];
                CHECK(kt.layer == bd.layer && kt.r0 == 64 * bd.b && kt.k == k && kt.diag == (k == bd.b));
                CHECK(kt.rlo == kt.r0 && kt.rhi == std::min(kt.r0 + 64, p.lay[kt.layer].n));
                CHECK(kt.xcol + kt.r0 == xcol_of(p, kt.layer, kt.r0));
            }
    }
    if (T == 0) {
        CHECK(p.ks_segs.n() == 0 && p.ks_off.n() == 0 && p.n_ks_slots == 0 && p.n_ks_cnt == 0);
        return;
    }
    const int nwg = p.n_kwg();
    CHECK(nwg >= 1 && p.ks_off.n() == nwg + 1);
    CHECK(p.ks_off.host[0] == 0 && p.ks_off.host[nwg] == p.ks_segs.n());
    // the XCD order undone: run i's segments
    std::vector<std::pair<int, int>> run(nwg, {-1, -1});
    for (int w = 0; w < nwg; ++w) {
        const int i = xcd_run(w, nwg);
        CHECK(i >= 0 && i < nwg && run[i].first < 0);
        CHECK(p.ks_off.host[w] < p.ks_off.host[w + 1]);  // no empty run
        run[i] = {p.ks_off.host[w], p.ks_off.host[w + 1]};
    }
    // every (tile, pass) unit in exactly one segment: the runs in order walk
    // the units in order
    std::vector<std::vector<KsSeg>> of_tile(T);
    int64_t u = 0;
    for (int i = 0; i < nwg; ++i) {
        int last_tile = -1;
        for (int s = run[i].first; s < run[i].second; ++s) {
            const KsSeg& sg = p.ks_segs.host[s];
            CHECK(sg.tile >= 0 && (size_t)sg.tile < T && sg.p0 >= 0 && sg.p0 < sg.p1 && sg.p1 <= np);
            CHECK((int64_t)sg.tile * np + sg.p0 == u);
            CHECK(sg.tile != last_tile);  // a run's passes of one tile are one segment
            last_tile = sg.tile;
            u = (int64_t)sg.tile * np + sg.p1;
            of_tile[sg.tile].push_back(sg);
        }
    }
    CHECK(u == (int64_t)T * np);
    // split tiles: a counter, nc contributors ci = 0 .. nc - 1 in pass order on
    // slots slot .. slot + nc - 1
    std::set<int> cnts;
    int slot = 0;
    for (size_t t = 0; t < T; ++t) {
        const std::vector<KsSeg>& v = of_tile[t];
        const int nc = (int)v.size();
        CHECK(nc >= 1);
        CHECK((p.ks_tiles.host[t].cnt >= 0) == (nc > 1));
        if (nc == 1) {
            CHECK(v[0].slot == -1 && v[0].nc == 1 && v[0].ci == 0 && p.ks_tiles.host[t].cnt == -1);
            continue;
        }
        CHECK(cnts.insert(p.ks_tiles.host[t].cnt).second);
        for (int j = 0; j < nc; ++j)  // of_tile is in pass order (the walk above)
            CHECK(v[j].nc == nc && v[j].ci == j && v[j].slot == slot);
        slot += nc;
    }
    CHECK(slot == p.n_ks_slots);
    CHECK((int)cnts.size() == p.n_ks_cnt);
    CHECK(cnts.empty() || (*cnts.begin() == 0 && *cnts.rbegin() == p.n_ks_cnt - 1));
}

// --------------------------------------------------------- segmented tables
void check_fseg(const psvi_plan& p, int nwg_max, const DevTable<FsSeg>& segs, const DevTable<int>& off,
                const DevTable<FwdRowBlock>& rbs, int n_slots) {
    const int np = (p.d.S + kKsPass - 1) / kKsPass;
    struct Blk {
        int layer, r0, r1, xcol, nkb;
    };
    std::vector<Blk> blks;
    std::map<std::pair<int, int>, int> blk_of;  // (layer, r0) -> block
    int64_t U = 0;
    for (const ShardRun& run : p.runs[p.rank])
        for (int r0 = run.lo; r0 < run.hi; r0 += kFwdRows) {
            const int r1 = std::min(r0 + kFwdRows, run.hi);
            const int kmax = std::max(0, std::min(r1 - 1, p.lay[run.layer].n - 2));
            blk_of[{run.layer, r0}] = (int)blks.size();
            blks.push_back(Blk{run.layer, r0, r1, run.col + (r0 - run.lo), (kmax + 63) / 64});
            U += (int64_t)blks.back().nkb * np;
        }
    if (U == 0) {
        CHECK(segs.n() == 0 && off.n() == 0 && rbs.n() == 0 && n_slots == 0);
        return;
    }
    const int B = (int)blks.size(), nwg = off.n() - 1;
    CHECK(nwg >= 1 && nwg <= nwg_max && off.host[0] == 0 && off.host[nwg] == segs.n());
    for (int w = 0; w < nwg; ++w) CHECK(off.host[w] < off.host[w + 1]);
    // every (row block, pass, 64-column block) unit in exactly one segment
    std::vector<std::vector<char>> hit((size_t)B * np);
    for (int b = 0; b < B; ++b)
        for (int q = 0; q < np; ++q) hit[(size_t)b * np + q].assign(blks[b].nkb, 0);
    std::vector<std::vector<int>> grp((size_t)B * np);  // the slots of a (row block, pass)
    std::set<int> slots;
    for (const FsSeg& sg : segs.host) {
        const auto it = blk_of.find({sg.layer, sg.r0});
        CHECK(it != blk_of.end());
        const Blk& bk = blks[it->second];
        CHECK(sg.r1 == bk.r1 && sg.pass >= 0 && sg.pass < np && sg.pad == 0);
        CHECK(sg.k0 % 64 == 0 && sg.k1 % 64 == 0 && sg.k0 >= 0 && sg.k0 < sg.k1 && sg.k1 / 64 <= bk.nkb);
        std::vector<char>& h = hit[(size_t)it->second * np + sg.pass];
        for (int kb = sg.k0 / 64; kb < sg.k1 / 64; ++kb) {
            CHECK(!h[kb]);
            h[kb] = 1;
        }
        CHECK(sg.slot >= 0 && sg.slot < n_slots && slots.insert(sg.slot).second);
        grp[(size_t)it->second * np + sg.pass].push_back(sg.slot);
    }
    for (const auto& h : hit)
        for (char c : h) CHECK(c);
    CHECK((int)slots.size() == n_slots);
    // a workgroup's segments, XCD order undone, continue each other
    {
        std::vector<int> w_of(nwg, -1);
        for (int w = 0; w < nwg; ++w) {
            const int i = xcd_run(w, nwg);
            CHECK(i >= 0 && i < nwg && w_of[i] < 0);
            w_of[i] = w;
        }
        int64_t u = 0;
        std::vector<int64_t> ub(B + 1, 0);
        for (int b = 0; b < B; ++b) ub[b + 1] = ub[b] + (int64_t)blks[b].nkb * np;
        for (int i = 0; i < nwg; ++i)
            for (int s = off.host[w_of[i]]; s < off.host[w_of[i] + 1]; ++s) {
                const FsSeg& sg = segs.host[s];
                const int b = blk_of[{sg.layer, sg.r0}];
                CHECK(ub[b] + (int64_t)sg.pass * blks[b].nkb + sg.k0 / 64 == u);
                u += (sg.k1 - sg.k0) / 64;
            }
        CHECK(u == U);
    }
    // reduce blocks: one per (row block, pass), its slots consecutive; nk sums
    // to the slot count
    CHECK(rbs.n() == B * np);
    int nk_sum = 0;
    for (int b = 0; b < B; ++b)
        for (int q = 0; q < np; ++q) {
            const FwdRowBlock& rb = rbs.host[(size_t)b * np + q];
            auto g = grp[(size_t)b * np + q];
            std::sort(g.begin(), g.end());
            CHECK(rb.nk == (int)g.size());
            for (int j = 0; j < rb.nk; ++j) CHECK(g[j] == rb.slot0 + j);
            if (rb.nk == 0) CHECK(rb.slot0 == 0);
            CHECK(rb.layer == blks[b].layer && rb.r0 == blks[b].r0 && rb.R == blks[b].r1 - blks[b].r0);
            CHECK(rb.xcol == blks[b].xcol && rb.s0 == kKsPass * q);
            nk_sum += rb.nk;
        }
    CHECK(nk_sum == n_slots);
}

// ------------------------------------------- forward items and update chunks
void check_fwd(const psvi_plan& p) {
    int nrb = 0, items = 0;
    std::set<int> slots;
    for (const ShardRun& run : p.runs[p.rank])
        for (int r0 = run.lo; r0 < run.hi; r0 += kFwdRows, ++nrb) {
            CHECK(nrb < p.frb.n());
            const FwdRowBlock& rb = p.frb.host[nrb];
            const int r1 = std::min(r0 + kFwdRows, run.hi);
            const int kmax = std::max(0, std::min(r1 - 1, p.lay[run.layer].n - 2));
            CHECK(rb.layer == run.layer && rb.r0 == r0 && rb.R == r1 - r0 && rb.s0 == 0);
            CHECK(rb.xcol == run.col + (r0 - run.lo) && rb.nk >= 1);
            // the row block's items tile [0, kmax) on its slots
            std::vector<std::pair<int, int>> ks;
            for (const FwdItem& it : p.fwd.host)
                if (it.layer == run.layer && it.r0 == r0) {
                    CHECK(it.r1 == r1 && it.xcol == rb.xcol);
                    CHECK(it.slot >= rb.slot0 && it.slot < rb.slot0 + rb.nk && slots.insert(it.slot).second);
                    ks.push_back({it.k0, it.k1});
                }
            std::sort(ks.begin(), ks.end());
            CHECK((int)ks.size() == rb.nk);
            int k = 0;
            for (const auto& kk : ks) {
                CHECK(kk.first == k && (kk.second > kk.first || kmax == 0));
                k = kk.second;
            }
            CHECK(k == kmax);
            items += rb.nk;
        }
    CHECK(nrb == p.frb.n() && items == p.fwd.n());
    for (int i = 0; i + 1 < p.fwd.n(); ++i) {  // longest first
        const FwdItem &a = p.fwd.host[i], &b = p.fwd.host[i + 1];
        CHECK(a.k1 - a.k0 >= b.k1 - b.k0);
    }
}

void check_upd(const psvi_plan& p) {
    const std::vector<Band> bands = rank_bands(p);
    CHECK(p.ufrb.n() == (int)bands.size());
    CHECK(p.upd.n() % 8 == 0);
    // the pads: empty chunks and nothing else
    std::map<std::pair<int, int>, std::vector<UpdChunk>> of_band;
    for (const UpdChunk& c : p.upd.host) {
        if (c.k0 == c.k1) {
            CHECK(c.layer == 0 && c.r0 == 0 && c.k0 == 0 && c.rlo == 0 && c.rhi == 0 && c.xcol == 0 &&
                  c.diag == 0 && c.slot == -1);
            continue;
        }
        CHECK(c.k0 >= 0 && c.k0 < c.k1);
        of_band[{c.layer, c.r0}].push_back(c);
    }
    CHECK(of_band.size() == bands.size());
    int slot = 0, tiles = 0;
    for (size_t i = 0; i < bands.size(); ++i) {
        const int l = bands[i].layer, b = bands[i].b;
        auto v = of_band[{l, 64 * b}];
        std::sort(v.begin(), v.end(), [](const UpdChunk& x, const UpdChunk& y) { return x.k0 < y.k0; });
        CHECK(!v.empty());
        // the band's chunks tile c-blocks 0 .. b, the last one diagonal, on
        // consecutive slots
        const FwdRowBlock& rb = p.ufrb.host[i];
        CHECK(rb.slot0 == slot && rb.nk == (int)v.size());
        int k = 0, ndiag = 0;
        for (const UpdChunk& c : v) {
            CHECK(c.k0 == k && c.slot == slot++);
            CHECK(c.diag == (c.k1 == b + 1));
            CHECK(c.r0 == 64 * b && c.rlo < c.rhi && c.rhi > 64 * b && c.rlo < 64 * b + 64);
            CHECK(c.xcol + std::max(64 * b, c.rlo) == xcol_of(p, l, std::max(64 * b, c.rlo)));
            ndiag += c.diag;
            k = c.k1;
        }
        CHECK(k == b + 1 && ndiag == 1);
        tiles += b + 1;
        CHECK(rb.layer == l && rb.r0 == std::max(64 * b, v[0].rlo));
        CHECK(rb.R == std::min(64 * b + 64, v[0].rhi) - rb.r0 && rb.R >= 1);
        CHECK(rb.xcol == xcol_of(p, l, rb.r0) && rb.s0 == 0);
    }
    CHECK(slot == p.n_uslots);
    CHECK(tiles == p.upd_tiles);
}

// ------------------------------------------------------- workspace layouts
struct Buf {
    char* p;
    size_t n;
    explicit Buf(size_t bytes) : p(static_cast<char*>(std::malloc(bytes))), n(bytes) {}
    Buf(const Buf&) = delete;
    ~Buf() { std::free(p); }
};

// One region of a layout carved on a buffer of exactly the reported size.
struct Region {
    const char* name;
    const void* ptr;  // nullptr: the plan has no such region
    size_t bytes;     // what the entry point may touch from ptr on
};

// Every region 256-aligned, in increasing order, none overlapping the one
// before, all inside [base, base + bytes); the sizes-only pass reports the
// same bytes.
void check_regions(const char* layout, const char* base, size_t bytes, size_t bytes_null,
                   const std::vector<Region>& regions) {
    CHECK(bytes == bytes_null);
    const char* end = base;
    for (const Region& r : regions) {
        if (!r.ptr) continue;
        const char* q = static_cast<const char*>(r.ptr);
        if (q < end || (q - base) % 256 != 0 || q + r.bytes > base + bytes) {
            if (++g_failed <= 50)
                std::fprintf(stderr, "[%s] %s.%s: offset %td size %zu, previous end %td, total %zu\n",
                             g_what.c_str(), layout, r.name, q - base, r.bytes, end - base, bytes);
            return;
        }
        end = q + r.bytes;
    }
}

std::vector<Region> step_regions(const psvi_plan& p, const StepWs& w) {
    const size_t n = sizeof(float) * (size_t)p.d.S * p.rows_tot[p.rank];
    return {{"x", w.x, n}, {"g", w.g, n + 256}, {"acc", w.acc, sizeof(float) * (size_t)p.acc_count}};
}
void append(std::vector<Region>& v, const std::vector<Region>& more) {
    v.insert(v.end(), more.begin(), more.end());
}
std::vector<Region> outer_regions(const psvi_plan& p, const OuterWs& w) {
    const size_t S = p.d.S, M = p.d.M, D = plan_in_dim(p), f = sizeof(float);
    std::vector<Region> v = step_regions(p, w.step);
    append(v, {{"nll", w.nll, f * S * M}, {"rowcoef", w.rowcoef, f * 2 * S}, {"ck", w.ck, f * S},
               {"sck", w.sck, f}, {"stats", w.stats, sizeof(double) * 2 * S},
               {"du", w.du, f * S * M * D}, {"dz", w.dz, f * S * M}});
    return v;
}

// the five layouts of a non-LeNet plan, each carved on a malloc'd buffer of
// exactly its size (the sanitizer's redzones right behind it)
void check_workspaces(const psvi_plan& p) {
    const size_t S = p.d.S, M = p.d.M, f = sizeof(float);
    CHECK(p.ws_bytes == step_ws(p, nullptr).bytes);
    {
        const Buf buf(step_ws(p, nullptr).bytes);
        const StepWs w = step_ws(p, buf.p);
        check_regions("step", buf.p, buf.n, w.bytes, step_regions(p, w));
        CHECK((p.family == PSVI_FAMILY_FULLCOV) == (w.x != nullptr && w.g != nullptr));
        CHECK((p.family == PSVI_FAMILY_FULLCOV) == (w.acc == nullptr));
        if (w.g) CHECK(w.g_pad == w.g + S * p.rows_tot[p.rank]);
    }
    {
        const Buf buf(loop_ws(p, nullptr).bytes);
        const LoopWs w = loop_ws(p, buf.p);
        const size_t eb = f * ((size_t)eps_stride(p) + 64);
        std::vector<Region> v = step_regions(p, w.step);
        append(v, {{"ebuf0", w.ebuf[0], eb}, {"ebuf1", w.ebuf[1], eb},
                   {"tstate", w.tstate, f * tiled_floats(p)},
                   {"pbuf0", w.pbuf[0], w.pbuf_bytes}, {"pbuf1", w.pbuf[1], w.pbuf_bytes}});
        check_regions("loop", buf.p, buf.n, w.bytes, v);
        CHECK((w.tstate != nullptr) == tiled_ok(p));
        CHECK((w.pbuf[0] != nullptr) == p.bf_stream && (w.pbuf[1] != nullptr) == p.bf_stream);
        if (p.bf_stream) CHECK(w.pbuf_bytes >= 3 * sizeof(uint16_t) * (size_t)p.eps_planes.pl);
        // each pad: 64 floats, inside its owner's region, behind the owner's data
        const float* owner[3] = {w.ebuf[0], w.ebuf[1], w.step.g};
        const size_t data[3] = {(size_t)p.Peps, (size_t)p.Peps, S * p.rows_tot[p.rank]};
        const size_t room[3] = {eb, eb, f * data[2] + 256};
        for (int k = 0; k < 3; ++k) {
            CHECK((w.pads[k] != nullptr) == (owner[k] != nullptr));
            if (!owner[k]) continue;
            CHECK(w.pads[k] == owner[k] + data[k]);
            CHECK((const char*)(w.pads[k] + 64) <= (const char*)owner[k] + room[k]);
        }
    }
    {
        const Buf buf(outer_ws(p, nullptr).bytes);
        const OuterWs w = outer_ws(p, buf.p);
        check_regions("outer", buf.p, buf.n, w.bytes, outer_regions(p, w));
        CHECK((w.dz != nullptr) == (p.lik == PSVI_LIK_GAUSSIAN));
    }
    {
        const Buf buf(eval_ws(p, nullptr).bytes);
        const EvalWs w = eval_ws(p, buf.p);
        std::vector<Region> v = outer_regions(p, w.outer);
        append(v, {{"out", w.out, f * S * M * p.lay[p.L - 1].dout}, {"W", w.W, f * S}});
        check_regions("eval", buf.p, buf.n, w.bytes, v);
    }
    {
        const Buf buf(hvp_ws(p, nullptr).bytes);
        const HvpWs w = hvp_ws(p, buf.p);
        const size_t nt = p.n_tot, ns = rop_splits(p);
        const size_t part2 = f * kFwdRows *
                             std::max({(size_t)p.fwd.n() * S, (size_t)p.n_fp_slots * kKsPass,
                                       (size_t)p.n_fs_slots * kKsPass});
        std::vector<Region> v = step_regions(p, w.step);
        append(v, {{"xd", w.xd, f * S * nt}, {"G", w.G, f * ns * S * nt}, {"Gd", w.Gd, f * ns * S * nt},
                   {"du", w.du, f * S * M * p.lay[0].din}, {"nlld", w.nlld, f * S * M},
                   {"dzd", w.dzd, f * S * M}, {"part2", w.part2, part2}});
        check_regions("hvp", buf.p, buf.n, w.bytes, v);
        CHECK((w.dzd != nullptr) == (p.lik == PSVI_LIK_GAUSSIAN));
        CHECK((w.part2 != nullptr) == (p.family == PSVI_FAMILY_FULLCOV));
    }
}

// ------------------------------------------------------------- LDS layouts
// One region of a kernel's dynamic LDS (lds_layout.hpp) at its documented extent.
struct LdsRegion {
    const char* name;
    void* ptr;
    size_t elem, count;
    bool absent = false;  // the shape has no such region: null
};
#define LDS_R(l, m, count) LdsRegion{#m, (l).m, sizeof(*(l).m), (size_t)(count)}

int g_lds_cases = 0;

// `layout(base)` is a kernel's layout function at one shape, `regions(l)` its
// regions in order.  The null-base bytes are what the closed-form expression
// of the commit before lds_layout.hpp gave (`was`: the layouts are unchanged)
// and, for a shape the launcher accepts, within the kernel's opt-in cap.  On
// a buffer of exactly that many bytes every region is non-null, aligned to its
// type and starts where the one before ends; its first and last element are
// written, the sanitizer's redzone right behind the last region.
template <class Layout, class Regions>
void check_lds(const char* kernel, size_t was, bool accepted, size_t cap, Layout layout, Regions regions) {
    ++g_lds_cases;
    g_what = kernel;
    const auto l0 = layout(nullptr);
    CHECK(l0.bytes == was);
    if (accepted) CHECK(l0.bytes <= cap);
    for (const LdsRegion& r : regions(l0)) CHECK(r.ptr == nullptr);
    const Buf buf(l0.bytes);
    const auto l = layout(buf.p);
    CHECK(l.bytes == l0.bytes);
    char* end = buf.p;
    for (const LdsRegion& r : regions(l)) {
        if (r.absent) {
            CHECK(r.ptr == nullptr && r.count == 0);
            continue;
        }
        char* q = static_cast<char*>(r.ptr);
        if (q != end || (q - buf.p) % r.elem != 0 || q + r.elem * r.count > buf.p + buf.n) {
            if (++g_failed <= 50)
                std::fprintf(stderr, "[%s] %s: offset %td, %zu x %zu bytes, previous end %td, total %zu\n",
                             g_what.c_str(), r.name, q - buf.p, r.count, r.elem, end - buf.p, buf.n);
            return;
        }
        if (r.count) {
            std::memset(q, 0xA5, r.elem);
            std::memset(q + r.elem * (r.count - 1), 0x5A, r.elem);
        }
        end = q + r.elem * r.count;
    }
    CHECK(end == buf.p + buf.n);
}

void check_lds_laplace() {
    const size_t f8 = sizeof(double), f4 = sizeof(float);
    int staged[2] = {0, 0};
    for (int Nu : {0, 1, kLapMaxNu})
        for (int d : {1, 2, 255, kLapMaxD}) {
            const int ds = d | 1;
            const bool was_xlds = f8 * (2 * kLapMaxD + kLapThreads + (size_t)Nu) + f4 * (size_t)Nu * ds <= kLapLds;
            g_what = "laplace_fit";
            CHECK(lap_fit_xlds(Nu, ds) == was_xlds);
            for (bool xlds : {false, true}) {
                const size_t was = f8 * (2 * kLapMaxD + kLapThreads + (size_t)Nu) +
                                   (xlds ? f4 * (size_t)Nu * ds : 0);
                check_lds("laplace_fit", was, xlds == was_xlds, kLapLds,
                          [&](void* b) { return lap_fit_lds(b, Nu, ds, xlds); },
                          [&](const LapFitLds& l) {
                              return std::vector<LdsRegion>{LDS_R(l, th, 2 * kLapMaxD), LDS_R(l, part, kLapThreads),
                                                            LDS_R(l, r, Nu), LDS_R(l, xs, xlds ? Nu * ds : 0)};
                          });
            }
            ++staged[was_xlds];
        }
    g_what = "laplace_fit";
    CHECK(staged[0] > 0 && staged[1] > 0);
    // the GPU suite's two sides (tests/test_hip_laplace.py: the edge shapes; Nu = 700, d = 65)
    CHECK(lap_fit_xlds(65, 65 | 1) && !lap_fit_xlds(700, 65 | 1) && !lap_fit_xlds(4096, 11 | 1));
    for (int d : {2, 127, kLapFullMaxD})
        for (int Nu : {0, 1, kLapMaxNu})
            for (int S : {0, 1, kSelMaxS}) {
                const size_t head = f8 * ((size_t)d + (size_t)d * (d + 1) / 2);
                const int room = (int)((kLapLds - head) / (f8 * d));
                const int nb = std::min(std::min(kLapThreads, room), S);
                g_what = "laplace_sample_full";
                CHECK(lap_full_cols(d, S) == nb);
                check_lds("laplace_sample_full", head + f8 * (size_t)std::max(Nu, nb * d), true, kLapLds,
                          [&](void* b) { return lap_full_lds(b, Nu, d, nb); },
                          [&](const LapFullLds& l) {
                              return std::vector<LdsRegion>{LDS_R(l, th, d), LDS_R(l, P, d * (d + 1) / 2),
                                                            LDS_R(l, work, std::max(Nu, nb * d))};
                          });
            }
    const size_t giga_cap = giga_lds(nullptr, kLapMaxRows, kSelMaxS).bytes;
    g_what = "giga_step";
    CHECK(giga_cap == f8 * (3 * (size_t)kLapMaxRows + 2 * (size_t)kSelMaxS));
    for (int N : {1, kLapMaxRows})
        for (int S : {2, kSelMaxS})
            check_lds("giga_step", f8 * (3 * (size_t)N + 2 * (size_t)S), true, giga_cap,
                      [&](void* b) { return giga_lds(b, N, S); },
                      [&](const GigaLds& l) {
                          return std::vector<LdsRegion>{LDS_R(l, mean, N), LDS_R(l, inv, N), LDS_R(l, b, N),
                                                        LDS_R(l, ell, S), LDS_R(l, dd, S)};
                      });
}

void check_lds_mfvi_fit() {
    const size_t f4 = sizeof(float);
    int placed[2] = {0, 0};
    for (int L : {2, kMfFitMaxL})
        for (int D : {1, kMfFitMaxD})
            for (int H : {1, kMfFitMaxH})
                for (int B : {1, 16, kMfFitMaxB})
                    for (int S : {1, kMfFitMaxS}) {
                        psvi_net_desc d{};
                        d.n_layers = L;
                        d.dims[0] = D;
                        for (int l = 1; l < L; ++l) d.dims[l] = H;
                        d.dims[L] = 1;
                        d.M = B;
                        d.S = S;
                        MfviFitShape s;
                        const int rc = mfvi_fit_shape(d, s);
                        g_what = "mfvi_fit";
                        CHECK(rc == 0 && s.RB >= 1 && s.RB <= B);  // every shape of the ranges fits
                        ++placed[s.lds];
                        auto was = [&](bool lds, int RB) {
                            size_t f = 2 * (size_t)s.n_tot;
                            if (lds) f += 8 * (size_t)s.n_tot + (size_t)s.B * s.xs;
                            f += (size_t)(s.L + 1) * RB * s.hs;
                            return sizeof(double) * kMfFitThreads + f4 * f;
                        };
                        for (bool lds : {false, true}) {
                            // what a further row costs, as the solver takes it from the walk
                            CHECK(mffit_lds_bytes(s, lds, 1) - mffit_lds_bytes(s, lds, 0) ==
                                  f4 * (size_t)(s.L + 1) * s.hs);
                            for (int RB : {0, 1, s.RB}) {
                                const size_t n = s.n_tot, rows = (size_t)RB * s.hs;
                                check_lds("mfvi_fit", was(lds, RB), lds == s.lds && RB == s.RB, kMfFitLds,
                                          [&](void* b) { return mffit_lds(b, lds, s.L, s.B, s.n_tot, s.hs, s.xs, RB); },
                                          [&](const MfFitLds& l) {
                                              std::vector<LdsRegion> v{
                                                  LDS_R(l, red, kMfFitThreads), LDS_R(l, Wb, n), LDS_R(l, eb, n),
                                                  LDS_R(l, gmu, lds ? n : 0), LDS_R(l, grho, lds ? n : 0),
                                                  LDS_R(l, sp, lds ? 2 * n : 0), LDS_R(l, sm, lds ? 2 * n : 0),
                                                  LDS_R(l, sv, lds ? 2 * n : 0),
                                                  LDS_R(l, xl, lds ? (size_t)s.B * s.xs : 0),
                                                  LDS_R(l, h, (s.L - 1) * rows), LDS_R(l, dA, rows), LDS_R(l, dB, rows)};
                                              for (int i = 3; i < 9; ++i) v[i].absent = !lds;
                                              return v;
                                          });
                            }
                        }
                    }
    g_what = "mfvi_fit";
    CHECK(placed[0] > 0 && placed[1] > 0);
}

// the predictive scores' layout at the shapes predict_shape solves for a plan
void check_lds_predict(const psvi_plan& p) {
    const std::string plan = g_what;
    for (int64_t rpd : {1, 63, 64, 65, 1000}) {
        PredictShape s;
        g_what = plan + " predict_scores";
        // every plan built here is small: one row and one unit always fit.  RG,
        // wcap and ut[] have no query to pin them; they follow from the bytes
        // held below and from the cost of a further float, the two things the
        // solver reads off the walk (its body is otherwise as it was)
        CHECK(predict_shape(p, rpd, s) == 0);
        CHECK(s.RG >= 1 && s.RG <= kPredMaxRows && s.wcap >= 1);
        for (int l = 0; l < p.L; ++l)  // a tile of every layer: its W rows and its biases
            CHECK(s.ut[l] >= 1 && (size_t)s.ut[l] * (p.lay[l].din + 1) <= (size_t)s.wcap);
        // what a further float of the W tile costs, as the solver takes it from the walk
        CHECK(pred_lds_bytes(s, s.RG, 1) - pred_lds_bytes(s, s.RG, 0) == sizeof(float));
        const size_t was = sizeof(double) * 2 * kPredThreads +
                           sizeof(float) * ((size_t)s.wcap + (size_t)s.RG * (s.xs + 2 * s.hs + s.C));
        check_lds(g_what.c_str(), was, true, kPredLds,
                  [&](void* b) { return pred_lds(b, s.RG, s.wcap, s.xs, s.hs, s.C); },
                  [&](const PredLds& l) {
                      const size_t R = s.RG;
                      return std::vector<LdsRegion>{LDS_R(l, red, 2 * kPredThreads), LDS_R(l, Wt, s.wcap),
                                                    LDS_R(l, xin, R * s.xs), LDS_R(l, hA, R * s.hs),
                                                    LDS_R(l, hB, R * s.hs), LDS_R(l, lg, R * s.C)};
                  });
    }
    g_what = plan;
}

void check_lds_kmeans() {
    for (int K : {1, kKmMaxK})
        for (int D : {1, 784, kKmMaxD}) {
            const int DT = (int)std::min<size_t>((size_t)D, (kKmLds - 256) / ((size_t)K * 8 + 4 * kKmRows));
            const int XS = DT | 1;
            g_what = "kmeans";
            CHECK(km_tile_cols(D, K) == DT && DT >= 1);
            for (bool rows : {true, false}) {
                const size_t was = sizeof(double) * (size_t)K * DT +
                                   (rows ? sizeof(float) * kKmRows * (size_t)XS : 0);
                check_lds(rows ? "km_assign" : "km_sums", was, true, kKmLds,
                          [&](void* b) { return km_lds(b, K, DT, XS, rows); },
                          [&](const KmLds& l) {
                              return std::vector<LdsRegion>{LDS_R(l, sC, (size_t)K * DT),
                                                            LDS_R(l, sX, rows ? kKmRows * XS : 0)};
                          });
            }
        }
}

// ------------------------------------------------------------ R-op geometry
// tests/golden/w3_rop_geometry.json: per plan of a grid, what launch_net_rop
// passed to its kernels before the geometry moved into the plan.  Every list
// is preceded by its length and every record lists its numbers in one fixed
// order, so the reader takes the file as the sequence of its integers outside
// quoted strings.
struct IntStream {
    std::vector<long> v;
    size_t at = 0;
    bool load(const char* path) {
        std::FILE* f = std::fopen(path, "rb");
        if (!f) return false;
        bool quoted = false, num = false, neg = false;
        long x = 0;
        for (int c; (c = std::fgetc(f)) != EOF;) {
            if (quoted) {
                if (c == '\\') (void)std::fgetc(f);
                quoted = c != '"';
                continue;
            }
            if (c >= '0' && c <= '9') {
                x = 10 * x + (c - '0');
                num = true;
                continue;
            }
            if (num) v.push_back(neg ? -x : x);
            num = neg = false;
            x = 0;
            quoted = c == '"';
            neg = c == '-';
        }
        std::fclose(f);
        return true;
    }
    bool over = false;  // read past the end
    bool done() const { return at >= v.size(); }
    long next() {
        if (at < v.size()) return v[at++];
        over = true;
        return -1;
    }
};

// a layout's regions (float offsets and extents) on a buffer of exactly its
// bytes: apart, inside, 16-byte aligned, first and last float written (the
// sanitizer's redzone right behind the buffer)
struct FloatRegion {
    const char* name;
    int off;
    size_t count;
};
void check_float_regions(size_t bytes, std::vector<FloatRegion> r) {
    CHECK(bytes % sizeof(float) == 0);
    const Buf buf(bytes);
    float* base = reinterpret_cast<float*>(buf.p);
    std::sort(r.begin(), r.end(), [](const FloatRegion& a, const FloatRegion& b) { return a.off < b.off; });
    size_t end = 0;
    for (const FloatRegion& q : r) {
        if (q.count == 0) continue;
        if (q.off < 0 || (size_t)q.off < end || q.off % 4 != 0 || (q.off + q.count) * sizeof(float) > bytes) {
            if (++g_failed <= 50)
                std::fprintf(stderr, "[%s] %s: offset %d, %zu floats, previous end %zu, total %zu bytes\n",
                             g_what.c_str(), q.name, q.off, q.count, end, bytes);
            return;
        }
        base[q.off] = 1.f;
        base[q.off + q.count - 1] = 2.f;
        end = q.off + q.count;
    }
}

void check_rop_valu(const psvi_plan& p, const RopValuLds& v, bool with_g) {
    const int L = p.L;
    const size_t rc = v.rc, nt = p.n_tot;
    size_t xtot = 0;
    int wmax = 0;
    for (int l = 0; l < L; ++l) {
        // odd row strides: a lane per output row hits its own bank
        CHECK(v.ldw[l] % 2 == 1 && v.ldw[l] >= p.lay[l].din && v.xo[l] == (int)xtot);
        xtot += (size_t)p.lay[l].dout * v.ldw[l] + p.lay[l].dout;
        wmax = std::max(wmax, std::max(p.lay[l].din, p.lay[l].dout));
    }
    CHECK(v.maxd % 2 == 1 && v.maxd >= wmax);
    std::vector<FloatRegion> r{{"X", v.lx, xtot}, {"XD", v.lxd, xtot}};
    if (with_g) {
        r.push_back({"G", v.lg, nt});
        r.push_back({"GD", v.lgd, nt});
    } else {
        CHECK(v.lg == 0 && v.lgd == 0);
    }
    for (int l = 0; l <= L; ++l) {
        const size_t d = l < L ? p.lay[l].din : p.lay[L - 1].dout;
        r.push_back({"h", v.lh[l], rc * d});
        r.push_back({"hd", v.lhd[l], rc * d});
    }
    for (int o : {v.ld0, v.ld1, v.ldd0, v.ldd1}) r.push_back({"delta", o, rc * v.maxd});
    check_float_regions(v.bytes, r);
}

void check_rop_mfma(const psvi_plan& p, const RopMfmaLds& m, int rows) {
    const int L = p.L;
    const size_t floats = m.bytes / sizeof(float), rows16 = (size_t)((rows + 15) & ~15);
    std::vector<FloatRegion> r;
    for (int l = 0; l <= L; ++l) {
        const int width = l < L ? p.lay[l].din : p.lay[L - 1].dout;
        // [h | h_dot] halves of kx and the stride's 8 floats; the halves are read as float4
        CHECK(m.kx[l] % 16 == 0 && m.kx[l] >= width && m.kx[l] < width + 16);
        CHECK(m.ldxm[l] == 2 * m.kx[l] + 8);
        r.push_back({"X", m.mxo[l], (size_t)rows * m.ldxm[l]});
        // a 16-row tile's reads past the region's rows stay inside the allocation
        CHECK(m.mxo[l] + rows16 * m.ldxm[l] <= floats);
    }
    int jobs = 0;
    for (int l = 0; l < L; ++l) {
        CHECK(m.ldwm[l] == 2 * m.kx[l] + 8);
        r.push_back({"W2", m.mwo[l], (size_t)m.kx[l + 1] * m.ldwm[l]});
        r.push_back({"b", m.mbo[l], 2 * (size_t)m.kx[l + 1]});
        // W2 jobs: a row of up to 64 columns each, layer by layer
        CHECK(m.jw[l] == jobs);
        jobs += m.kx[l + 1] * ((m.kx[l] + 63) / 64);
    }
    CHECK(m.jb == jobs);
    for (int l = 0; l < L; ++l) {
        CHECK(m.jb + m.jbl[l] == jobs);
        jobs += (m.kx[l + 1] + 63) / 64;
    }
    CHECK(m.ju == jobs);
    r.push_back({"stamps", m.lstamp, 20});  // 10 uint64
    check_float_regions(m.bytes, r);
}

int g_rop_plans = 0, g_rop_class[7] = {0, 0, 0, 0, 0, 0, 0};

// The fixture's numbers of one stack: each layout once (matrix-core by its
// padded rows, VALU by rows per chunk and with_g), then what every (M, nsplit)
// of the grid launches, refering to them.
struct RopStack {
    std::vector<int> dims;
    std::map<int, std::vector<long>> mfma;                  // rows -> bytes, offsets, job table
    std::map<std::pair<int, int>, std::vector<long>> valu;  // (rc, with_g) -> bytes, offsets
    std::map<std::pair<int, int>, std::vector<long>> cases; // (M, nsplit) -> form[2], lds[2], fits, rows, rc, single
    bool read(IntStream& in) {
        const int L = (int)in.next();
        if (L < 1 || L > kMaxL) return false;
        for (int i = 0; i <= L; ++i) dims.push_back((int)in.next());
        auto take = [&](std::vector<long>& v, int n) {
            for (int i = 0; i < n; ++i) v.push_back(in.next());
        };
        for (long n = in.next(); n > 0; --n) take(mfma[(int)in.next()], 1 + 3 * (L + 1) + 3 * L + 1 + 2 * L + 2);
        for (long n = in.next(); n > 0; --n) {
            const int rc = (int)in.next(), with_g = (int)in.next();
            take(valu[{rc, with_g}], 6 + 2 * (L + 1) + 4 + 2 * L);
        }
        for (long n = in.next(); n > 0; --n) {
            const int M = (int)in.next(), nsplit = (int)in.next();
            take(cases[{M, nsplit}], 8);
        }
        return !in.over;
    }
};
void put(std::vector<long>& v, const int* a, int n) { v.insert(v.end(), a, a + n); }
std::vector<long> flat(const RopMfmaLds& m, int L) {
    std::vector<long> v{(long)m.bytes};
    put(v, m.mxo, L + 1), put(v, m.ldxm, L + 1), put(v, m.kx, L + 1);
    put(v, m.mwo, L), put(v, m.ldwm, L), put(v, m.mbo, L), v.push_back(m.lstamp);
    put(v, m.jw, L), put(v, m.jbl, L), v.push_back(m.jb), v.push_back(m.ju);
    return v;
}
std::vector<long> flat(const RopValuLds& q, int L) {
    std::vector<long> v{(long)q.bytes, q.maxd, q.lx, q.lxd, q.lg, q.lgd};
    put(v, q.lh, L + 1), put(v, q.lhd, L + 1);
    for (int o : {q.ld0, q.ld1, q.ldd0, q.ldd1}) v.push_back(o);
    put(v, q.ldw, L), put(v, q.xo, L);
    return v;
}

// one plan of the grid against the fixture, then the layouts' structure
void check_rop_plan(const RopStack& st, int family, int S, int M, int nsplit) {
    g_what = "rop family=" + std::to_string(family);
    for (int d : st.dims) g_what += "-" + std::to_string(d);
    g_what += " S=" + std::to_string(S) + " M=" + std::to_string(M);
    std::unique_ptr<psvi_plan> pp(new psvi_plan());
    psvi_plan& p = *pp;
    p.family = family;
    p.d.n_layers = (int)st.dims.size() - 1;
    for (size_t i = 0; i < st.dims.size(); ++i) p.d.dims[i] = st.dims[i];
    p.d.S = S;
    p.d.M = M;
    p.d.prior_sd = 1.f;
    p.world = 1;
    p.rank = 0;
    std::string err;
    CHECK(build_plan(p, err) == 0);
    ++g_rop_plans;
    const RopGeometry& g = p.rop;
    const int L = p.L;
    const RopMfmaLds& m = g.mfma;
    const RopValuLds& v = g.valu;
    // what the launcher does with it under PSVI_DBG_ROP_VALU = 0 and 1
    const bool refused = v.rc == 0;
    const std::vector<long> now{refused ? 2 : g.mfma_fits ? 0 : 1, refused ? 2 : 1,
                                refused ? 0 : (long)(g.mfma_fits ? m.bytes : v.bytes), refused ? 0 : (long)v.bytes,
                                g.mfma_fits, g.mfma_rows, v.rc, g.single};
    CHECK(g.nsplit == nsplit);
    const auto c = st.cases.find({M, nsplit});
    CHECK(c != st.cases.end() && c->second == now);
    const auto fm = st.mfma.find(g.mfma_rows);
    CHECK(fm != st.mfma.end() && fm->second == flat(m, L));
    if (!refused) {
        const auto fv = st.valu.find({v.rc, g.single ? 0 : 1});
        CHECK(fv != st.valu.end() && fv->second == flat(v, L));
    }
    // structure
    const int rows_per = (M + g.nsplit - 1) / g.nsplit;
    CHECK(g.nsplit == rop_splits(p) && g.mfma_rows % 16 == 0 && g.mfma_rows >= rows_per && g.mfma_rows < rows_per + 16);
    CHECK(g.mfma_fits == (m.bytes <= kRopLds));
    check_rop_mfma(p, m, g.mfma_rows);
    // the over-read rule at rows off the 16-multiple (the tail slack)
    for (int rows : {1, 5, 17, rows_per}) check_rop_mfma(p, rop_mfma_lds(p, rows), rows);
    if (refused) {
        CHECK(g.single == 0 && rop_valu_lds(p, 1, true).bytes > kRopLds);
        ++g_rop_class[6];
        return;
    }
    CHECK(v.bytes <= kRopLds);
    if (g.single) {
        CHECK(v.rc == rows_per);
    } else {
        // the largest power of two up to 64 that fits beside the accumulators
        CHECK(v.rc >= 1 && v.rc <= 64 && (v.rc & (v.rc - 1)) == 0);
        CHECK(v.rc == 64 || rop_valu_lds(p, 2 * v.rc, true).bytes > kRopLds);
        CHECK(rop_valu_lds(p, rows_per, false).bytes > kRopLds);
    }
    check_rop_valu(p, v, !g.single);
    if (g.mfma_fits) ++g_rop_class[0];
    if (!g.mfma_fits && g.single) ++g_rop_class[1];
    if (!g.single) ++g_rop_class[v.rc == 64 ? 2 : v.rc == 32 ? 3 : v.rc == 16 ? 4 : 5];
}

void check_rop_geometry(const char* fixture) {
    g_what = fixture;
    IntStream in;
    CHECK(in.load(fixture));
    // the grid: S, M, families, nsplit of every (M, S), then the stacks
    std::vector<long> grid[3];
    for (auto& ax : grid)
        for (long n = in.next(); n > 0 && !in.done(); --n) ax.push_back(in.next());
    const std::vector<long>&Ss = grid[0], &Ms = grid[1], &fams = grid[2];
    std::vector<long> nsplit(Ms.size() * Ss.size());
    for (long& x : nsplit) x = in.next();
    int plans = 0;
    for (long n = in.next(); n > 0; --n) {
        RopStack st;
        g_what = fixture;
        CHECK(st.read(in));
        for (long fam : fams)
            for (size_t i = 0; i < Ms.size(); ++i)
                for (size_t j = 0; j < Ss.size(); ++j, ++plans)
                    check_rop_plan(st, (int)fam, (int)Ss[j], (int)Ms[i], (int)nsplit[i * Ss.size() + j]);
    }
    g_what = fixture;
    CHECK(in.done() && !in.over && plans == g_rop_plans && plans >= 700);
    // the grid holds every class: matrix-core, VALU single without it, VALU
    // chunked at 64, 32, 16 and below, unsupported
    for (int c : g_rop_class) CHECK(c > 0);
}

// ------------------------------------------------------------------- plans
std::unique_ptr<psvi_plan> make_plan(int family, const std::vector<int>& dims, int S, int M, int world,
                                     int rank) {
    std::unique_ptr<psvi_plan> p(new psvi_plan());
    p->family = family;
    p->d.n_layers = (int)dims.size() - 1;
    for (size_t i = 0; i < dims.size(); ++i) p->d.dims[i] = dims[i];
    p->d.S = S;
    p->d.M = M;
    p->d.prior_sd = 1.f;
    p->world = world;
    p->rank = rank;
    std::string err;
    const int rc = build_plan(*p, err);
    if (rc) {
        ++g_failed;
        std::fprintf(stderr, "[%s] build_plan: %d %s\n", g_what.c_str(), rc, err.c_str());
        return nullptr;
    }
    return p;
}

int g_plans = 0;

void check_fullcov(const std::vector<int>& dims, int S, int world, int rank) {
    g_what = "fullcov";
    for (int d : dims) g_what += "-" + std::to_string(d);
    g_what += " S=" + std::to_string(S) + " world=" + std::to_string(world) + " rank=" + std::to_string(rank) +
              " dbg=" + std::to_string(g_plan_dbg.stream_wgs) + "/" + std::to_string(g_plan_dbg.ks_wgs);
    const std::unique_ptr<psvi_plan> p = make_plan(PSVI_FAMILY_FULLCOV, dims, S, 100, world, rank);
    if (!p) return;
    ++g_plans;
    check_stream(*p, g_plan_dbg.stream_rr != 0);
    check_kstream(*p);
    check_fseg(*p, 512, p->fs_segs, p->fs_off, p->fs_rb, p->n_fs_slots);
    check_fseg(*p, 256, p->fp_segs, p->fp_off, p->fp_rb, p->n_fp_slots);
    check_fwd(*p);
    check_upd(*p);
    check_workspaces(*p);
    check_lds_predict(*p);
}

void check_empty(int family, const char* name) {
    g_what = name;
    const std::unique_ptr<psvi_plan> p = make_plan(family, {64, 40, 40, 2}, 128, 100, 1, 0);
    if (!p) return;
    ++g_plans;
    CHECK(all_fullcov_tables_empty(*p));
    if (family == PSVI_FAMILY_LENET) return;  // its HVP scratch is kernels_lenet.hip's
    check_workspaces(*p);
    check_lds_predict(*p);
    g_what += " (gaussian)";  // as psvi_plan_create_lik leaves a Gaussian plan
    p->lik = PSVI_LIK_GAUSSIAN;
    check_workspaces(*p);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: plan_tables_check tests/golden/w3_rop_geometry.json\n");
        return 2;
    }
    const std::vector<int> fn2{64, 40, 40, 2};
    for (int S : {128, 32, 96, 100, 130, 256, 1024}) check_fullcov(fn2, S, 1, 0);
    for (int r = 0; r < 8; ++r) check_fullcov(fn2, 1024, 8, r);
    for (int r = 0; r < 2; ++r) check_fullcov(fn2, 128, 2, r);
    // one layer: n = 2, n = 6 (one tile), n = 64 exactly, n = 65 (a one-row second band)
    for (int S : {128, 256})
        for (const std::vector<int>& dims : {std::vector<int>{1, 1}, {2, 2}, {7, 8}, {12, 5}})
            check_fullcov(dims, S, 1, 0);
    check_fullcov({3, 5, 2}, 64, 1, 0);
    check_empty(PSVI_FAMILY_MEANFIELD, "mean-field");
    check_empty(PSVI_FAMILY_LENET, "lenet");
    // workgroup counts that are no multiple of 8
    g_plan_dbg.stream_wgs = 64;
    check_fullcov(fn2, 128, 1, 0);
    g_plan_dbg.stream_wgs = 100;
    check_fullcov(fn2, 128, 1, 0);
    g_plan_dbg.stream_wgs = 0;
    g_plan_dbg.ks_wgs = 100;
    check_fullcov(fn2, 128, 1, 0);
    g_plan_dbg.ks_wgs = 0;
    check_lds_laplace();
    check_lds_mfvi_fit();
    check_lds_kmeans();
    check_rop_geometry(argv[1]);
    if (g_failed) {
        std::fprintf(stderr, "plan_tables_check: %d failed checks\n", g_failed);
        return 1;
    }
    std::printf("plan_tables_check: %d plans ok, %d LDS layouts ok\n", g_plans, g_lds_cases);
    std::printf("R-op geometry: %d plans ok; matrix-core %d, VALU single without it %d, chunked rc 64: %d, "
                "32: %d, 16: %d, below: %d, unsupported %d\n",
                g_rop_plans, g_rop_class[0], g_rop_class[1], g_rop_class[2], g_rop_class[3], g_rop_class[4],
                g_rop_class[5], g_rop_class[6]);
    return 0;
}
