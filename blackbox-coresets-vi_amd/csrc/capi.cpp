// capi.cpp -- extern "C" boundary of libpsvi_hip.so (declared in include/psvi_hip.h).
//
// Plans hold the immutable geometry of one (family, layer sizes, S, M, world,
// rank) configuration: sample shards, nnz-balanced row shards of every
// full-cov layer, and the device work lists of the packed-triangular kernels
// (built on the host by plan_tables.cpp; uploaded and owned here).
// Steps are pure stream-ordered kernel launches + hipMemsetAsync (graph
// capturable: no allocation, no synchronisation).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "psvi_diag.h"
#include "psvi_internal.hpp"

namespace psvi {
Diag g_diag;
}  // namespace psvi

using namespace psvi;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char* where) {
    g_err = std::string(where) + ": " + hipGetErrorString(e);
    return (int)e;
}

#define HIP_TRY(expr)                                      \
    do {                                                   \
        hipError_t e_ = (expr);                            \
        if (e_ != hipSuccess) return hip_fail(e_, #expr);  \
    } while (0)

template <class T>
int upload(DevTable<T>& t) {
    const char* what = "";
    const hipError_t e = t.upload(&what);
    return e == hipSuccess ? 0 : hip_fail(e, what);
}

int check_desc(const psvi_net_desc* d) {
    if (!d) return fail(PSVI_EINVAL, "null descriptor");
    if (d->n_layers < 1 || d->n_layers > PSVI_MAX_LAYERS)
        return fail(PSVI_EINVAL, "n_layers out of range [1, 8]");
    for (int l = 0; l <= d->n_layers; ++l)
        if (d->dims[l] < 1) return fail(PSVI_EINVAL, "layer dims must be >= 1");
    if (d->S < 1) return fail(PSVI_EINVAL, "S must be >= 1");
    if (d->M < 1) return fail(PSVI_EINVAL, "M must be >= 1");
    if (!(d->prior_sd > 0.f)) return fail(PSVI_EINVAL, "prior_sd must be > 0");
    return 0;
}

// The only device allocations of the library: a plan's immutable work lists
// and its scratch, in a fixed order up to the first failure.
int plan_to_device(psvi_plan& p) {
    const int S = p.d.S;
    const bool fullcov = p.family == PSVI_FAMILY_FULLCOV;
    if (int rc = upload(p.fwd)) return rc;
    if (int rc = upload(p.frb)) return rc;
    if (int rc = upload(p.upd)) return rc;
    // split-K scratch of the sample phase (plan-owned, reused every step)
    if (p.fwd.n() > 0 && !p.fwd_part.alloc(sizeof(float) * (size_t)p.fwd.n() * S * kFwdRows))
        return fail(PSVI_EUNSUP, "cannot allocate the sample-phase scratch");
    if (p.fuse_sample && p.n_uslots > 0) {
        if (int rc = upload(p.ufrb)) return rc;
        if (!p.upd_part.alloc(sizeof(float) * (size_t)p.n_uslots * S * 64))
            return fail(PSVI_EUNSUP, "cannot allocate the fused-sample scratch");
    }
    if (p.str.n() > 0) {
        if (int rc = upload(p.str)) return rc;
        if (int rc = upload(p.sfrb)) return rc;
        const size_t nb = (size_t)std::max(1, p.sfrb.n());
        if (!p.str_part.alloc(sizeof(float) * (size_t)p.n_sslots * S * 64) ||
            !p.str_cnt.alloc(sizeof(int) * nb, true) || !p.str_bms.alloc(sizeof(float) * 128 * nb))
            return fail(PSVI_EUNSUP, "cannot allocate the streaming-update scratch");
    }
    if (p.n_kwg() > 0) {
        if (int rc = upload(p.ks_tiles)) return rc;
        if (int rc = upload(p.ks_segs)) return rc;
        if (int rc = upload(p.ks_off)) return rc;
        if (!p.ks_slots.alloc(sizeof(float) * (size_t)std::max(1, p.n_ks_slots) * kKsSlotFloats) ||
            !p.ks_cnt.alloc(sizeof(int) * std::max(1, p.n_ks_cnt), true))
            return fail(PSVI_EUNSUP, "cannot allocate the K-split update's slots");
    }
    if (p.n_fswg() > 0) {
        if (int rc = upload(p.fs_segs)) return rc;
        if (int rc = upload(p.fs_off)) return rc;
        if (int rc = upload(p.fs_rb)) return rc;
        if (int rc = upload(p.fp_segs)) return rc;
        if (int rc = upload(p.fp_off)) return rc;
        if (int rc = upload(p.fp_rb)) return rc;
        // (the slots serve both tables)
        if (!p.fs_part.alloc(sizeof(float) * (size_t)std::max({1, p.n_fs_slots, p.n_fp_slots}) *
                             kKsPass * kFwdRows))
            return fail(PSVI_EUNSUP, "cannot allocate the segmented sample's slots");
    }
    if (fullcov) {
        net_xmap(p, p.xmap.host, p.net_bands.host);
        if (int rc = upload(p.xmap)) return rc;
        if (int rc = upload(p.net_bands)) return rc;
    }
    if (fullcov && p.mchunks > 1 &&
        !p.net_slots.alloc(sizeof(float) * (size_t)p.mchunks * std::max(1, p.s_cnt[p.rank]) * p.n_tot))
        return fail(PSVI_EUNSUP, "cannot allocate the network's pseudopoint-chunk slots");
    if (p.family == PSVI_FAMILY_MEANFIELD &&
        !p.mf_slots.alloc(sizeof(float) * (size_t)std::max(1, p.s_cnt[p.rank]) * p.mchunks * p.n_tot))
        return fail(PSVI_EUNSUP, "cannot allocate the mean-field gradient slots");
    // (psvi_plan_create_lik releases it again on a Gaussian or Bernoulli plan)
    if (p.family == PSVI_FAMILY_MEANFIELD && p.world == 1 &&
        !p.pred_scratch.alloc(predict_scratch_bytes(p.n_tot)))
        return fail(PSVI_EUNSUP, "cannot allocate the predictive scores' scratch");
    if (fullcov && p.fuse_sample && p.tiles_total > 0 && !p.aux.create())
        return fail(PSVI_EUNSUP, "cannot create the inner loop's conversion stream");
    if (p.eps_planes_ok) {
        p.eps_planes_tab.host.assign(1, p.eps_planes);
        if (int rc = upload(p.eps_planes_tab)) return rc;
    }
    if (p.family == PSVI_FAMILY_LENET && !p.lenet_scratch.alloc(lenet_ws(p, nullptr).bytes))
        return fail(PSVI_EUNSUP, "cannot allocate the LeNet activation scratch");
    return 0;
}

}  // namespace

// The opt-ins made so far: a short list behind a mutex (thread ranks reach it
// together; a handful of kernels on a handful of devices).
hipError_t psvi::allow_dynamic_lds(const void* kernel, size_t bytes) {
    struct Done {
        const void* kernel;
        int dev;
        size_t bytes;
    };
    static std::mutex mu;
    static std::vector<Done> done;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    for (const Done& d : done)
        if (d.kernel == kernel && d.dev == dev && d.bytes >= bytes) return hipSuccess;
    const hipError_t e =
        hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) done.push_back({kernel, dev, bytes});
    return e;
}

namespace {

hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Diagnostics (PSVI_DBG_LOOP_TIMING): HIP events around the network and the
// update launches of every `g_loop_every`-th full-cov inner-loop step.
int g_loop_every = 0;
std::vector<hipEvent_t> g_loop_ev[2];  // [net, update] x (start, end) pairs

void loop_events_clear() {
    for (auto& v : g_loop_ev) {
        for (hipEvent_t e : v) (void)hipEventDestroy(e);
        v.clear();
    }
}

// records the next start or end event of phase k on the stream
hipError_t loop_event(int k, hipStream_t st) {
    hipEvent_t e;
    const hipError_t rc = hipEventCreate(&e);
    if (rc != hipSuccess) return rc;
    g_loop_ev[k].push_back(e);
    return hipEventRecord(e, st);
}

}  // namespace

extern "C" {

const char* psvi_last_error(void) { return g_err.c_str(); }
const char* psvi_version(void) { return "psvi_hip 0.1.0 (gfx950)"; }

int psvi_debug_set(int32_t key, int32_t value) {
    switch (key) {
        case PSVI_DBG_LOOP_TIMING: loop_events_clear(); g_loop_every = value; return 0;
        case PSVI_DBG_NET_ABLATION: g_diag.net_ablation = value; return 0;
        case PSVI_DBG_UPD_ABLATION: g_diag.upd_ablation = value; return 0;
        case PSVI_DBG_NET_SPLIT_BELOW: g_diag.net_split_below = value; return 0;
        case PSVI_DBG_NET_WG_TARGET:
            if (value < 1) return fail(PSVI_EINVAL, "workgroup target must be >= 1");
            g_diag.net_wg_target = value;
            return 0;
        case PSVI_DBG_FWD_ABLATION: g_diag.fwd_ablation = value; return 0;
        case PSVI_DBG_UPD_CHUNK: g_plan_dbg.upd_chunk_tiles = value; return 0;
        case PSVI_DBG_UPD_STREAM_OFF: g_diag.stream_off = value; return 0;
        case PSVI_DBG_STREAM_BF_OFF: g_diag.stream_bf_off = value; return 0;
        case PSVI_DBG_KSTREAM_OFF: g_diag.ks_off = value; return 0;
        case PSVI_DBG_KSTREAM_WGS: g_plan_dbg.ks_wgs = value; return 0;
        case PSVI_DBG_FWD_SEG_OFF: g_diag.fs_off = value; return 0;
        case PSVI_DBG_FWD_SEG_BF_OFF: g_diag.fs_bf_off = value; return 0;
        case PSVI_DBG_FWD_PAIR_BF: g_diag.fwd_pair_bf = value; return 0;
        case PSVI_DBG_STREAM_FOLD_OFF: g_diag.stream_fold_off = value; return 0;
        case PSVI_DBG_KSTREAM_BF_OFF: g_diag.ks_bf_off = value; return 0;
        case PSVI_DBG_ROP_VALU: g_diag.rop_valu = value; return 0;
        case PSVI_DBG_NET_SCALAR_LOADS: g_diag.net_scalar_loads = value; return 0;
        case PSVI_DBG_NET_MLOOP_OFF: g_diag.net_mloop_off = value; return 0;
        case PSVI_DBG_NET_GEO_OFF: g_diag.net_geo_off = value; return 0;
        case PSVI_DBG_NET_DRAW_SPARE_OFF: g_diag.net_draw_spare_off = value; return 0;
        case PSVI_DBG_NET_DRAW_ROLE1:
            if (value < 0 || value > 32) return fail(PSVI_EINVAL, "0..32");
            g_diag.net_draw_role1 = value;
            return 0;
        case PSVI_DBG_STREAM_WGS: g_plan_dbg.stream_wgs = value; return 0;
        case PSVI_DBG_STREAM_COST: g_plan_dbg.stream_cost = value; return 0;
        case PSVI_DBG_STREAM_RR: g_plan_dbg.stream_rr = value; return 0;
        case PSVI_DBG_LENET_ABLATION: g_diag.lenet_abl = value; return 0;
        case PSVI_DBG_NET_THREADS:
            if (value != 0 && value != 256 && value != 512) return fail(PSVI_EINVAL, "256 or 512");
            g_diag.net_threads = value;
            return 0;
        default: return fail(PSVI_EINVAL, "unknown debug key");
    }
}

int psvi_debug_loop_timing(double* out) {
    if (!out) return fail(PSVI_EINVAL, "null out");
    for (int k = 0; k < 2; ++k) {
        double sum = 0.0;
        const auto& v = g_loop_ev[k];
        for (size_t i = 0; i + 1 < v.size(); i += 2) {
            float ms = 0.f;
            HIP_TRY(hipEventSynchronize(v[i + 1]));
            HIP_TRY(hipEventElapsedTime(&ms, v[i], v[i + 1]));
            sum += ms;
        }
        const size_t n = v.size() / 2;
        out[k] = n ? 1e3 * sum / (double)n : 0.0;
        if (k == 0) out[2] = (double)n;
    }
    loop_events_clear();
    return 0;
}

int psvi_debug_set_ptr(int32_t key, void* ptr) {
    switch (key) {
        case PSVI_DBG_NET_STAMPS: g_diag.net_stamps = (unsigned long long*)ptr; return 0;
        case PSVI_DBG_NET_DRAW_PLANES: g_diag.net_draw_planes = (uint16_t*)ptr; return 0;
        case PSVI_DBG_UPD_STAMPS: g_diag.upd_stamps = (unsigned long long*)ptr; return 0;
        case PSVI_DBG_BF_STAMPS: g_diag.bf_stamps = (unsigned long long*)ptr; return 0;
        case PSVI_DBG_ROP_STAMPS: g_diag.rop_stamps = (unsigned long long*)ptr; return 0;
        case PSVI_DBG_FWD_STAMPS: g_diag.fwd_stamps = (unsigned long long*)ptr; return 0;
        default: return fail(PSVI_EINVAL, "unknown debug key");
    }
}

int psvi_plan_create(int32_t family, const psvi_net_desc* d, int32_t world, int32_t rank,
                     psvi_plan** out) {
    if (!out) return fail(PSVI_EINVAL, "null out");
    *out = nullptr;
    if (family != PSVI_FAMILY_MEANFIELD && family != PSVI_FAMILY_FULLCOV &&
        family != PSVI_FAMILY_LENET)
        return fail(PSVI_EINVAL, "unknown family");
    psvi_net_desc dl;
    if (family == PSVI_FAMILY_LENET && d) {  // fixed architecture: dims ignored
        dl = *d;
        dl.n_layers = 5;
        const int dims[6] = {784, 6, 16, 120, 84, 10};
        for (int l = 0; l < 6; ++l) dl.dims[l] = dims[l];
        d = &dl;
    }
    if (int rc = check_desc(d)) return rc;
    if (world < 1 || world > kMaxWorld || rank < 0 || rank >= world)
        return fail(PSVI_EINVAL, "world/rank out of range (world <= 8)");
    int ndev = 0;
    const bool have_dev = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    if (have_dev) {  // on the device the tables go to
        HIP_TRY(net_allow_lds());
        HIP_TRY(rop_allow_lds());
    }
    psvi_plan* p = new psvi_plan();
    p->family = family;
    p->d = *d;
    p->world = world;
    p->rank = rank;
    std::string err;
    int rc = build_plan(*p, err);
    if (rc) rc = fail(rc, err);
    if (!rc && have_dev) {
        rc = plan_to_device(*p);
        p->on_device = rc == 0;
    }
    if (rc) {
        psvi_plan_destroy(p);
        return rc;
    }
    *out = p;
    return 0;
}

int psvi_plan_create_lik(int32_t family, const psvi_net_desc* d, int32_t world, int32_t rank,
                         const psvi_likelihood* lik, psvi_plan** out) {
    if (!lik || lik->kind == PSVI_LIK_CATEGORICAL)
        return psvi_plan_create(family, d, world, rank, out);
    if (!out) return fail(PSVI_EINVAL, "null out");
    *out = nullptr;
    if (lik->kind != PSVI_LIK_GAUSSIAN && lik->kind != PSVI_LIK_BERNOULLI)
        return fail(PSVI_EINVAL, "unknown likelihood kind");
    const bool gauss = lik->kind == PSVI_LIK_GAUSSIAN;
    if (family != PSVI_FAMILY_MEANFIELD && family != PSVI_FAMILY_FULLCOV &&
        family != PSVI_FAMILY_LENET)
        return fail(PSVI_EINVAL, "unknown family");
    if (family != PSVI_FAMILY_MEANFIELD)
        return fail(PSVI_EUNSUP, gauss ? "the Gaussian likelihood runs mean-field plans only"
                                       : "the Bernoulli likelihood runs mean-field plans only");
    if (int rc = check_desc(d)) return rc;
    if (world < 1 || world > kMaxWorld || rank < 0 || rank >= world)
        return fail(PSVI_EINVAL, "world/rank out of range (world <= 8)");
    if (world != 1)
        return fail(PSVI_EUNSUP, gauss ? "the Gaussian likelihood needs world == 1"
                                       : "the Bernoulli likelihood needs world == 1");
    if (d->dims[d->n_layers] != 1)
        return fail(PSVI_EINVAL,
                    gauss ? "the Gaussian likelihood has one output (dims[n_layers] == 1)"
                          : "the Bernoulli likelihood has one output (dims[n_layers] == 1)");
    if (gauss && (!(lik->tau > 0.f) || !std::isfinite(lik->tau)))
        return fail(PSVI_EINVAL, "the Gaussian precision tau must be positive and finite");
    if (int rc = psvi_plan_create(family, d, world, rank, out)) return rc;
    (*out)->lik = lik->kind;
    (*out)->pred_scratch.release();  // psvi_predict_scores runs categorical plans only
    if (gauss) (*out)->lik_tau = lik->tau;
    return 0;
}

int psvi_plan_destroy(psvi_plan* p) {
    delete p;
    return 0;
}

static size_t loop_ws_bytes(const psvi_plan* p);
static size_t tiled_floats(const psvi_plan* p);

// psvi_outer_elbo_grad workspace: the step workspace (x / g or acc), then the
// per-row NLL [S][M], row coefficients [S][2], ck [S], sum ck, per-sample
// stats [S][2] doubles, and the per-sample input gradients [S][M][D]
struct OuterWs {
    float *nll, *rowcoef, *ck, *sck, *du;
    double* stats;
    float* dz;  // Gaussian plans: per-sample target gradients [S][M]
    size_t bytes;
};
static OuterWs outer_ws(const psvi_plan* p, void* ws);

// psvi_hvp workspace: the step workspace (x), x_dot [S][n_tot], G and G_dot
// [splits][S][n_tot], d_u parts [S][M][D], NLL_dot [S][M]
struct HvpWs {
    float *xd, *G, *Gd, *du, *nlld;
    float* dzd;    // Gaussian plans: per-sample target products [S][M]
    float* part2;  // full-cov: split-K slots of the tangent sample (pair launch)
    size_t bytes;
};
static HvpWs hvp_ws(const psvi_plan* p, void* ws) {
    const size_t S = p->d.S, M = p->d.M, D = p->lay[0].din, nt = p->n_tot;
    char* b = (char*)ws;
    HvpWs o{};
    if (p->family == PSVI_FAMILY_LENET) {  // tangent scratch of launch_lenet_hvp
        o.bytes = lenet_tan_ws(*p, nullptr).bytes;
        return o;
    }
    size_t off = align256(p->ws_bytes);
    auto take = [&](size_t bytes) {
        char* r = b ? b + off : nullptr;
        off += align256(bytes);
        return r;
    };
    o.xd = (float*)take(sizeof(float) * S * nt);
    const size_t ns = rop_splits(*p);  // the R-op's row-block slots (summed into slot 0)
    o.G = (float*)take(sizeof(float) * ns * S * nt);
    o.Gd = (float*)take(sizeof(float) * ns * S * nt);
    o.du = (float*)take(sizeof(float) * S * M * D);
    o.nlld = (float*)take(sizeof(float) * S * M);
    if (p->lik == PSVI_LIK_GAUSSIAN) o.dzd = (float*)take(sizeof(float) * S * M);
    if (p->family == PSVI_FAMILY_FULLCOV)
        o.part2 = (float*)take(sizeof(float) *
                               std::max({(size_t)p->fwd.n() * S, (size_t)p->n_fp_slots * kKsPass,
                                         (size_t)p->n_fs_slots * kKsPass}) *
                               kFwdRows);  // item-grid or either segment table's slots
    o.bytes = off;
    return o;
}

static OuterWs outer_ws(const psvi_plan* p, void* ws);

// psvi_evaluate workspace: the outer workspace, then the data rows' softmax
// [S][M][C] (bounded by M rows) and the sample weights [S]
static size_t eval_prob_off(const psvi_plan* p);
static size_t eval_ws_bytes(const psvi_plan* p) {
    const size_t S = p->d.S, M = p->d.M, C = p->lay[p->L - 1].dout;
    return eval_prob_off(p) + align256(sizeof(float) * S * M * C) + align256(sizeof(float) * S);
}

static OuterWs outer_ws(const psvi_plan* p, void* ws) {
    const size_t S = p->d.S, M = p->d.M, D = plan_in_dim(*p);
    char* b = (char*)ws;
    OuterWs o{};
    size_t off = align256(p->ws_bytes);
    auto take = [&](size_t bytes) {
        char* r = b ? b + off : nullptr;
        off += align256(bytes);
        return r;
    };
    o.nll = (float*)take(sizeof(float) * S * M);
    o.rowcoef = (float*)take(sizeof(float) * 2 * S);
    o.ck = (float*)take(sizeof(float) * S);
    o.sck = (float*)take(sizeof(float));
    o.stats = (double*)take(sizeof(double) * 2 * S);
    o.du = (float*)take(sizeof(float) * S * M * D);
    if (p->lik == PSVI_LIK_GAUSSIAN) o.dz = (float*)take(sizeof(float) * S * M);
    o.bytes = off;
    return o;
}

int psvi_plan_query(const psvi_plan* p, int32_t key, int64_t* value) {
    if (!p || !value) return fail(PSVI_EINVAL, "null argument");
    const int r = p->rank;
    switch (key) {
        case PSVI_Q_PARAM_COUNT: *value = p->P; break;
        case PSVI_Q_EPS_COUNT: *value = p->Peps; break;
        case PSVI_Q_WS_BYTES: *value = (int64_t)p->ws_bytes; break;
        case PSVI_Q_S_LOCAL: *value = p->s_cnt[r]; break;
        case PSVI_Q_S_OFFSET: *value = p->s_off[r]; break;
        case PSVI_Q_ACC_COUNT: *value = p->acc_count; break;
        case PSVI_Q_ROWS_LOCAL: *value = p->rows_tot[r]; break;
        case PSVI_Q_XSHARD_COUNT: *value = (int64_t)p->d.S * p->rows_tot[r]; break;
        case PSVI_Q_LOOP_WS_BYTES: *value = (int64_t)loop_ws_bytes(p); break;
        case PSVI_Q_TILED_FLOATS: *value = (int64_t)tiled_floats(p); break;
        case PSVI_Q_XRECV_COUNT: *value = (int64_t)p->s_cnt[r] * p->n_tot; break;
        case PSVI_Q_OUTER_WS_BYTES: *value = (int64_t)outer_ws(p, nullptr).bytes; break;
        case PSVI_Q_HVP_WS_BYTES: *value = (int64_t)hvp_ws(p, nullptr).bytes; break;
        case PSVI_Q_EVAL_WS_BYTES: *value = (int64_t)eval_ws_bytes(p); break;
        case PSVI_Q_NET_PART_OK:
            *value = p->family == PSVI_FAMILY_FULLCOV && !(p->mchunks > 1 && !p->net_mloop);
            break;
        case PSVI_Q_NET_MCHUNKS: *value = p->mchunks; break;
        default: return fail(PSVI_EINVAL, "unknown query key");
    }
    return 0;
}

int psvi_plan_shard_info(const psvi_plan* p, int32_t r, int64_t* out) {
    if (!p || !out) return fail(PSVI_EINVAL, "null argument");
    if (r < 0 || r >= p->world) return fail(PSVI_EINVAL, "rank out of range");
    out[0] = p->s_off[r];
    out[1] = p->s_cnt[r];
    out[2] = p->rows_tot[r];
    for (int l = 0; l < PSVI_MAX_LAYERS; ++l) {
        int cnt = 0, nrun = 0, lo = 0;
        for (const ShardRun& run : p->runs[r])
            if (run.layer == l) {
                if (nrun++ == 0) lo = run.lo;
                cnt += run.hi - run.lo;
            }
        // the first row when the rank's rows of layer l are one run (or none),
        // -1 when they are several (psvi_plan_shard_runs lists them)
        out[3 + l] = nrun <= 1 ? lo : -1;
        out[3 + PSVI_MAX_LAYERS + l] = cnt;
    }
    return 0;
}

int psvi_plan_shard_runs(const psvi_plan* p, int32_t r, int64_t* out, int32_t cap,
                         int32_t* count) {
    if (!p || !count) return fail(PSVI_EINVAL, "null argument");
    if (r < 0 || r >= p->world) return fail(PSVI_EINVAL, "rank out of range");
    const int n = (int)p->runs[r].size();
    *count = n;
    if (!out) return 0;
    if (cap < n) return fail(PSVI_ENOSPC, "run buffer too small");
    for (int i = 0; i < n; ++i) {
        const ShardRun& run = p->runs[r][i];
        out[4 * i] = run.layer;
        out[4 * i + 1] = run.lo;
        out[4 * i + 2] = run.hi - run.lo;
        out[4 * i + 3] = run.col;
    }
    return 0;
}

// Every entry point that runs on a plan, except the loop that takes it up,
// drops the resident state of a PSVI_LOOP_KEEP call: it may have written the
// workspace, the parameters or the Adam state the state stands for.
static void drop_resident(const psvi_plan* p) {
    if (p) p->resident.valid = false;
}

// The entry points' plan check.  families: the allowed PSVI_FAMILY_* as a bit
// mask, with `what` the message for a plan outside it (the phase entry points
// report a null plan the same way); without them a null plan is the error.
constexpr unsigned kFullCov = 1u << PSVI_FAMILY_FULLCOV, kNotFullCov = ~kFullCov;
static int check_plan(const psvi_plan* p, unsigned families = ~0u, const char* what = nullptr) {
    if (!p && !what) return fail(PSVI_EINVAL, "null plan");
    if (!p || !(families >> p->family & 1u)) return fail(PSVI_ESTATE, what);
    if (!p->on_device) return fail(PSVI_ESTATE, "plan was created without a HIP device");
    return 0;
}
static const char kNotMf[] = "not a mean-field plan", kNotFc[] = "not a full-cov plan";

// Bernoulli plans run the inner objective, psvi_sampled_kl_grad and
// psvi_row_loglik only.
static int refuse_bernoulli(const psvi_plan* p, const char* what) {
    if (p && p->lik == PSVI_LIK_BERNOULLI) return fail(PSVI_EUNSUP, what);
    return 0;
}

// The Adam hyper-parameters of an entry point that steps (required; the
// gradient-only calls pass false and may leave hp null).
static int check_adam(const psvi_adam_hp* hp, bool required = true) {
    if (!required) return 0;
    if (hp->step < 1) return fail(PSVI_EINVAL, "adam step must be >= 1");
    if (hp->kind < 0 || hp->kind > 2) return fail(PSVI_EINVAL, "unknown adam kind");
    return 0;
}

// The ABI's `const int32_t* z`: labels, or a Gaussian plan's fp32 targets in
// the same 4-byte slots.
static Targets abi_targets(const psvi_plan* p, const int32_t* z) {
    return p->lik == PSVI_LIK_GAUSSIAN ? Targets::values(reinterpret_cast<const float*>(z))
                                       : Targets::labels(z);
}

static int check_step(const psvi_plan* p, const void* u, const void* z, const void* w,
                      const void* eps, size_t ws_bytes, const void* ws) {
    if (int rc = check_plan(p)) return rc;
    if (p->world != 1) return fail(PSVI_ESTATE, "fused step needs world == 1 (use phases)");
    if (!u || !z || !w || !eps) return fail(PSVI_EINVAL, "null input pointer");
    if (!ws || ws_bytes < p->ws_bytes) return fail(PSVI_ENOSPC, "workspace too small");
    return 0;
}

// the network launch on the rows (u, z, w), its NLL added into nll_out
static NetLaunch net_rows(const float* u, Targets z, const float* w, double* nll_out) {
    NetLaunch n;
    n.u = u; n.targets = z; n.w = w; n.nll_out = nll_out;
    return n;
}

// the full-cov update's Adam step on g_shard, its KL added into kl_out
static MvnUpdate mvn_step(const float* eps, const float* g_shard, float* params, float* m,
                          float* v, const psvi_adam_hp* hp, double* kl_out, int include_kl) {
    MvnUpdate up;
    up.eps = eps; up.g_shard = g_shard; up.params = params; up.m = m; up.v = v; up.hp = hp;
    up.kl_out = kl_out; up.include_kl = include_kl ? 1 : 0;
    return up;
}

static int step_impl(const psvi_plan* p, const float* u, Targets z, const float* w,
                     const float* eps, float* params, float* m, float* v,
                     const psvi_adam_hp* hp, double* elbo_out, float* grad_out,
                     int include_kl, void* ws, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(elbo_out, 0, sizeof(double), st));
    char* wsb = (char*)ws;
    NetLaunch n = net_rows(u, z, w, elbo_out);
    if (p->family != PSVI_FAMILY_FULLCOV) {
        MfUpdate up;
        up.params = params; up.m = m; up.v = v; up.hp = hp;
        up.kl_out = elbo_out; up.grad_out = grad_out; up.include_kl = include_kl;
        if (p->family == PSVI_FAMILY_LENET) {
            float* acc = (float*)wsb;
            HIP_TRY(launch_lenet(*p, u, z.slots(), w, params, eps, acc, elbo_out, p->lenet_scratch.dev, st));
            up.acc = acc;
        } else {
            // per-(sample, chunk) gradient slots, summed in a fixed order by the update
            n.params = params; n.eps = eps; n.mf_slots = p->mf_slots.dev;
            HIP_TRY(launch_net(*p, n, st));
            up.slot_eps = eps;
        }
        HIP_TRY(launch_mf_update(*p, up, st));
    } else {
        const size_t xs = sizeof(float) * (size_t)p->d.S * p->rows_tot[0];
        float* x = (float*)wsb;
        float* g = (float*)(wsb + align256(xs));
        HIP_TRY(launch_mvn_fwd(*p, eps, params, x, st));
        n.xrecv = x; n.gsend = g;
        HIP_TRY(launch_net(*p, n, st));
        MvnUpdate up = mvn_step(eps, g, params, m, v, hp, elbo_out, include_kl);
        up.grad_out = grad_out;
        HIP_TRY(launch_mvn_update(*p, up, st));
    }
    return 0;
}

int psvi_inner_step(const psvi_plan* p, const float* u, const int32_t* z, const float* w,
                    const float* eps, float* params, float* adam_m, float* adam_v,
                    const psvi_adam_hp* hp, double* elbo_out, void* ws, size_t ws_bytes,
                    void* stream) {
    drop_resident(p);
    if (int rc = check_step(p, u, z, w, eps, ws_bytes, ws)) return rc;
    if (!params || !adam_m || !adam_v || !hp || !elbo_out)
        return fail(PSVI_EINVAL, "null state pointer");
    if (int rc = check_adam(hp)) return rc;
    return step_impl(p, u, abi_targets(p, z), w, eps, params, adam_m, adam_v, hp, elbo_out,
                     nullptr, 1, ws, as_stream(stream));
}

int psvi_elbo_grad(const psvi_plan* p, const float* u, const int32_t* z, const float* w,
                   const float* eps, const float* params, int32_t include_kl, double* elbo_out,
                   float* grad_out, void* ws, size_t ws_bytes, void* stream) {
    drop_resident(p);
    if (int rc = check_step(p, u, z, w, eps, ws_bytes, ws)) return rc;
    if (!params || !elbo_out || !grad_out) return fail(PSVI_EINVAL, "null pointer");
    return step_impl(p, u, abi_targets(p, z), w, eps, const_cast<float*>(params), nullptr,
                     nullptr, nullptr, elbo_out, grad_out, include_kl ? 1 : 0, ws,
                     as_stream(stream));
}

int psvi_mf_phase_accumulate(const psvi_plan* p, const float* u, const int32_t* z,
                             const float* w, const float* eps, const float* params, float* acc,
                             double* nll_out, void* stream) {
    drop_resident(p);
    if (int rc = check_plan(p, kNotFullCov, kNotMf)) return rc;
    if (!u || !z || !w || !eps || !params || !acc || !nll_out)
        return fail(PSVI_EINVAL, "null pointer");
    hipStream_t st = as_stream(stream);
    if (p->family == PSVI_FAMILY_LENET) {
        HIP_TRY(launch_lenet(*p, u, z, w, params, eps, acc, nll_out, p->lenet_scratch.dev, st));
        return 0;
    }
    NetLaunch n = net_rows(u, abi_targets(p, z), w, nll_out);
    n.params = params; n.eps = eps; n.mf_slots = p->mf_slots.dev;
    HIP_TRY(launch_net(*p, n, st));
    HIP_TRY(launch_mf_slot_acc(*p, eps, acc, st));
    return 0;
}

int psvi_mf_phase_update(const psvi_plan* p, const float* acc, float* params, float* adam_m,
                         float* adam_v, const psvi_adam_hp* hp, double* kl_out,
                         float* grad_out, int32_t include_kl, void* stream) {
    drop_resident(p);
    if (int rc = check_plan(p, kNotFullCov, kNotMf)) return rc;
    if (!acc || !params) return fail(PSVI_EINVAL, "null pointer");
    if (!grad_out && (!adam_m || !adam_v || !hp)) return fail(PSVI_EINVAL, "null adam state");
    if (int rc = check_adam(hp, !grad_out)) return rc;
    MfUpdate up;
    up.acc = acc; up.params = params; up.m = adam_m; up.v = adam_v; up.hp = hp;
    up.kl_out = kl_out; up.grad_out = grad_out; up.include_kl = include_kl ? 1 : 0;
    HIP_TRY(launch_mf_update(*p, up, as_stream(stream)));
    return 0;
}

int psvi_mvn_phase_sample(const psvi_plan* p, const float* eps, const float* params,
                          float* x_shard, void* stream) {
    drop_resident(p);
    if (int rc = check_plan(p, kFullCov, kNotFc)) return rc;
    // a rank that owns no rows (fewer bands than ranks) has an empty x shard
    if (!eps || !params || (!x_shard && p->rows_tot[p->rank] > 0))
        return fail(PSVI_EINVAL, "null pointer");
    HIP_TRY(launch_mvn_fwd(*p, eps, params, x_shard, as_stream(stream)));
    return 0;
}

int psvi_mvn_phase_net(const psvi_plan* p, const float* u, const int32_t* z, const float* w,
                       const float* x_recv, float* g_send, double* nll_out, void* stream) {
    drop_resident(p);
    if (int rc = check_plan(p, kFullCov, kNotFc)) return rc;
    // a rank without samples (S < world) has empty x / g blocks
    const bool none = p->s_cnt[p->rank] == 0;
    if (!u || !z || !w || (!none && (!x_recv || !g_send)) || !nll_out)
        return fail(PSVI_EINVAL, "null pointer");
    NetLaunch n = net_rows(u, Targets::labels(z), w, nll_out);
    n.xrecv = x_recv; n.gsend = g_send;
    HIP_TRY(launch_net(*p, n, as_stream(stream)));
    return 0;
}

int psvi_mvn_phase_net_draw(const psvi_plan* p, const float* u, const int32_t* z, const float* w,
                            const float* x_recv, float* g_send, double* nll_out, float* eps_out,
                            int64_t n, uint64_t seed, uint64_t offset, void* stream) {
    drop_resident(p);
    if (int rc = check_plan(p, kFullCov, kNotFc)) return rc;
    const bool none = p->s_cnt[p->rank] == 0;  // S < world: empty x / g blocks
    if (!u || !z || !w || (!none && (!x_recv || !g_send)) || !nll_out || !eps_out || n < 0)
        return fail(PSVI_EINVAL, "null pointer or bad count");
    if (offset % 4) return fail(PSVI_EINVAL, "randn offset must be a multiple of 4");
    if (reinterpret_cast<uintptr_t>(eps_out) % 16)
        return fail(PSVI_EINVAL, "eps_out must be 16-byte aligned");
    NetLaunch nl = net_rows(u, Targets::labels(z), w, nll_out);
    nl.xrecv = x_recv; nl.gsend = g_send;
    nl.draw.out = eps_out; nl.draw.n = n; nl.draw.seed = seed; nl.draw.offset = offset;
    HIP_TRY(launch_net(*p, nl, as_stream(stream)));
    return 0;
}

int psvi_mvn_phase_net_part(const psvi_plan* p, const float* u, const int32_t* z, const float* w,
                            const float* x_recv, float* g_send, double* nll_out, int32_t s_begin,
                            int32_t s_count, float* eps_out, int64_t n, uint64_t seed,
                            uint64_t offset, int32_t part, int32_t nparts, void* stream) {
    drop_resident(p);
    if (int rc = check_plan(p, kFullCov, kNotFc)) return rc;
    const int S_loc = p->s_cnt[p->rank];
    if (s_begin < 0 || s_count < 0 || s_begin + s_count > S_loc)
        return fail(PSVI_EINVAL, "sample range outside the rank's samples");
    if (nparts < 1 || part < 0 || part >= nparts) return fail(PSVI_EINVAL, "bad draw part");
    if (!u || !z || !w || (s_count > 0 && (!x_recv || !g_send)) || !nll_out || n < 0 ||
        (n > 0 && !eps_out))
        return fail(PSVI_EINVAL, "null pointer or bad count");
    if (offset % 4) return fail(PSVI_EINVAL, "randn offset must be a multiple of 4");
    if (eps_out && reinterpret_cast<uintptr_t>(eps_out) % 16)
        return fail(PSVI_EINVAL, "eps_out must be 16-byte aligned");
    if (p->mchunks > 1 && !p->net_mloop && (s_begin != 0 || s_count != S_loc))
        return fail(PSVI_EUNSUP, "per-chunk gradient slots: whole sample launches only");
    NetLaunch nl = net_rows(u, Targets::labels(z), w, nll_out);
    nl.xrecv = x_recv; nl.gsend = g_send;
    nl.s_begin = s_begin; nl.s_count = s_count;
    nl.draw.out = n > 0 ? eps_out : nullptr; nl.draw.n = n; nl.draw.seed = seed; nl.draw.offset = offset;
    nl.draw.part = part; nl.draw.nparts = nparts;
    HIP_TRY(launch_net(*p, nl, as_stream(stream)));
    return 0;
}

int psvi_mvn_phase_update(const psvi_plan* p, const float* eps, const float* g_shard,
                          float* params, float* adam_m, float* adam_v, const psvi_adam_hp* hp,
                          double* kl_out, float* grad_out, int32_t include_kl, void* stream) {
    drop_resident(p);
    if (int rc = check_plan(p, kFullCov, kNotFc)) return rc;
    if (!eps || (!g_shard && p->rows_tot[p->rank] > 0) || !params)
        return fail(PSVI_EINVAL, "null pointer");
    if (!grad_out && (!adam_m || !adam_v || !hp)) return fail(PSVI_EINVAL, "null adam state");
    if (int rc = check_adam(hp, !grad_out)) return rc;
    MvnUpdate up = mvn_step(eps, g_shard, params, adam_m, adam_v, hp, kl_out, include_kl);
    up.grad_out = grad_out;
    HIP_TRY(launch_mvn_update(*p, up, as_stream(stream)));
    return 0;
}

int psvi_mvn_phase_update_sample(const psvi_plan* p, const float* eps, const float* g_shard,
                                 float* params, float* adam_m, float* adam_v,
                                 const psvi_adam_hp* hp, double* kl_out, int32_t include_kl,
                                 const float* eps_next, float* x_next, void* stream) {
    drop_resident(p);
    if (int rc = check_plan(p, kFullCov, kNotFc)) return rc;
    const bool rows = p->rows_tot[p->rank] > 0;  // no rows: empty G and x shards
    if (!eps || !params || !eps_next || (rows && (!g_shard || !x_next)))
        return fail(PSVI_EINVAL, "null pointer");
    if (!adam_m || !adam_v || !hp) return fail(PSVI_EINVAL, "null adam state");
    if (int rc = check_adam(hp)) return rc;
    MvnUpdate up = mvn_step(eps, g_shard, params, adam_m, adam_v, hp, kl_out, include_kl);
    up.next.eps = eps_next; up.next.x = x_next;
    HIP_TRY(launch_mvn_update(*p, up, as_stream(stream)));
    return 0;
}

static int64_t eps_stride(const psvi_plan* p) { return (p->Peps + 3) / 4 * 4; }

// tiled corr/m/v state: full-cov, world 1, one LDS pass of samples.  The
// write-through (sc1) stores of the stream kernel and the chunked kernel's
// tiled epilogue address all three arrays through ONE buffer descriptor
// (num_records 0x7fffffff, m / v at 32-bit byte offsets), so the whole state
// must stay below 2^31 bytes; larger plans keep corr / m / v packed (the
// chunked kernel with plain stores) instead of overflowing those offsets.
static bool tiled_ok(const psvi_plan* p) {
    return p->family == PSVI_FAMILY_FULLCOV && p->fuse_sample && p->tiles_total > 0 &&
           3 * p->tiles_total * 4096 * (int64_t)sizeof(float) < 0x7fffffff - 16;
}
static size_t tiled_floats(const psvi_plan* p) {
    return tiled_ok(p) ? 3 * (size_t)p->tiles_total * 4096 : 0;
}

// psvi_inner_loop workspace: the step workspace (x, g, a 256-byte tail), two
// eps buffers each followed by 64 floats of zeros (the streaming update's
// loads past a layer's last column block land there, unclamped), the tiled
// state
static size_t loop_ebuf_bytes(const psvi_plan* p) {
    return align256(sizeof(float) * ((size_t)eps_stride(p) + 64));
}
// the bf16 planes of one draw (three planes of EpsPlanes::pl elements)
static size_t loop_pbuf_bytes(const psvi_plan* p) {
    return p->bf_stream ? align256(3 * sizeof(uint16_t) * (size_t)p->eps_planes.pl) : 0;
}
static size_t loop_ws_bytes(const psvi_plan* p) {
    return align256(p->ws_bytes) + 2 * loop_ebuf_bytes(p) + align256(sizeof(float) * tiled_floats(p)) +
           2 * loop_pbuf_bytes(p);
}

int psvi_mvn_tiled_convert(const psvi_plan* p, float* params, float* adam_m, float* adam_v,
                           float* tstate, int32_t to_tiled, void* stream) {
    drop_resident(p);
    if (!p || !tiled_ok(p)) return fail(PSVI_EUNSUP, "plan has no tiled state (full-cov, world 1, S <= 128)");
    if (!p->on_device) return fail(PSVI_ESTATE, "plan was created without a HIP device");
    if (!params || !adam_m || !adam_v || !tstate) return fail(PSVI_EINVAL, "null pointer");
    HIP_TRY(launch_mvn_tile_convert(*p, params, adam_m, adam_v, tstate, to_tiled != 0,
                                    as_stream(stream)));
    return 0;
}

int psvi_mvn_phase_update_tiled(const psvi_plan* p, const float* eps, const float* g_shard,
                                float* params, float* adam_m, float* adam_v, float* tstate,
                                const psvi_adam_hp* hp, double* kl_out, int32_t include_kl,
                                const float* eps_next, float* x_next, void* stream) {
    drop_resident(p);
    if (!p || !tiled_ok(p)) return fail(PSVI_EUNSUP, "plan has no tiled state (full-cov, world 1, S <= 128)");
    if (!p->on_device) return fail(PSVI_ESTATE, "plan was created without a HIP device");
    if (!eps || !g_shard || !params || !adam_m || !adam_v || !tstate || !hp)
        return fail(PSVI_EINVAL, "null pointer");
    if (!eps_next != !x_next) return fail(PSVI_EINVAL, "eps_next and x_next go together");
    if (int rc = check_adam(hp)) return rc;
    MvnUpdate up = mvn_step(eps, g_shard, params, adam_m, adam_v, hp, kl_out, include_kl);
    up.next.eps = eps_next; up.next.x = x_next; up.tstate = tstate;
    HIP_TRY(launch_mvn_update(*p, up, as_stream(stream)));
    return 0;
}

int psvi_inner_loop(const psvi_plan* p, const float* u, const int32_t* z, const float* w,
                    const float* eps, uint64_t seed, uint64_t offset, int32_t T, float* params,
                    float* adam_m, float* adam_v, const psvi_adam_hp* hp, double* elbo_out,
                    void* ws, size_t ws_bytes, void* stream) {
    return psvi_inner_loop_ex(p, u, z, w, eps, seed, offset, T, params, adam_m, adam_v, hp,
                              elbo_out, ws, ws_bytes, 0, stream);
}

int psvi_inner_loop_ex(const psvi_plan* p, const float* u, const int32_t* z, const float* w,
                       const float* eps, uint64_t seed, uint64_t offset, int32_t T, float* params,
                       float* adam_m, float* adam_v, const psvi_adam_hp* hp, double* elbo_out,
                       void* ws, size_t ws_bytes, int32_t flags, void* stream) {
    if (!p) return fail(PSVI_EINVAL, "null plan");
    if (flags & ~(PSVI_LOOP_KEEP | PSVI_LOOP_RESUME)) return fail(PSVI_EINVAL, "unknown loop flags");
    if (int rc = check_plan(p)) return rc;
    if (p->world != 1) return fail(PSVI_ESTATE, "inner loop needs world == 1 (use phases)");
    if (!u || !z || !w || !params || !adam_m || !adam_v || !hp || !elbo_out)
        return fail(PSVI_EINVAL, "null pointer");
    if (T < 0) return fail(PSVI_EINVAL, "T must be >= 0");
    if (int rc = check_adam(hp)) return rc;
    if (!eps && offset % 4) return fail(PSVI_EINVAL, "randn offset must be a multiple of 4");
    if (!ws || ws_bytes < loop_ws_bytes(p)) return fail(PSVI_ENOSPC, "workspace too small");
    hipStream_t st = as_stream(stream);
    char* wsb = (char*)ws;
    const int64_t es = eps_stride(p);
    const Targets zt = abi_targets(p, z);
    float* ebuf[2] = {(float*)(wsb + align256(p->ws_bytes)),
                      (float*)(wsb + align256(p->ws_bytes) + loop_ebuf_bytes(p))};
    // eps of step t: the caller's [T][EPS_COUNT] array, or Philox (seed, offset + t * stride)
    RandnLaunch rn;  // the draw of one step's eps from the loop's stream
    rn.n = p->Peps; rn.seed = seed;
    auto eps_t = [&](int t) -> const float* {
        if (eps) return eps + (size_t)t * p->Peps;
        RandnLaunch r = rn;
        r.out = ebuf[t & 1]; r.offset = offset + (uint64_t)t * es;
        return launch_randn(r, st) == hipSuccess ? r.out : nullptr;
    };
    // eps of step 0 with the ELBO accumulators cleared: Philox mode folds the
    // clear into the draw's launch
    auto first_eps = [&]() -> const float* {
        if (eps) {
            return hipMemsetAsync(elbo_out, 0, sizeof(double) * (size_t)T, st) == hipSuccess
                       ? eps
                       : nullptr;
        }
        RandnLaunch r = rn;
        r.out = ebuf[0]; r.offset = offset; r.zero = elbo_out; r.nzero = T;
        return launch_randn(r, st) == hipSuccess ? ebuf[0] : nullptr;
    };
    psvi_adam_hp h = *hp;
    if (p->family == PSVI_FAMILY_MEANFIELD) {
        // two launches per step: the network kernel (which also draws the next
        // step's eps in Philox mode) and the slot-reducing update; the ELBO
        // accumulators are cleared once for the whole loop
        if (T == 0) return 0;
        const float* e = first_eps();
        if (!e) return fail(PSVI_EUNSUP, "randn launch failed");
        for (int t = 0; t < T; ++t) {
            h.step = hp->step + t;
            const bool draw = !eps && t + 1 < T;
            float* en_buf = draw ? ebuf[(t + 1) & 1] : nullptr;
            NetLaunch n = net_rows(u, zt, w, elbo_out + t);
            n.params = params; n.eps = e; n.mf_slots = p->mf_slots.dev;
            n.draw.out = en_buf; n.draw.n = draw ? p->Peps : 0;
            n.draw.seed = seed; n.draw.offset = offset + (uint64_t)(t + 1) * es;
            HIP_TRY(launch_net(*p, n, st));
            MfUpdate up;
            up.slot_eps = e; up.params = params; up.m = adam_m; up.v = adam_v; up.hp = &h;
            up.kl_out = elbo_out + t; up.include_kl = 1;
            HIP_TRY(launch_mf_update(*p, up, st));
            e = t + 1 < T ? (eps ? eps + (size_t)(t + 1) * p->Peps : en_buf) : nullptr;
        }
        return 0;
    }
    if (p->family != PSVI_FAMILY_FULLCOV) {
        for (int t = 0; t < T; ++t) {
            const float* e = eps_t(t);
            if (!e) return fail(PSVI_EUNSUP, "randn launch failed");
            h.step = hp->step + t;
            if (int rc = step_impl(p, u, zt, w, e, params, adam_m, adam_v, &h, elbo_out + t,
                                   nullptr, 1, ws, st))
                return rc;
        }
        return 0;
    }
    // full-cov: sample x_0, then per step net + update, the update also sampling
    // the next step's x from the updated parameters (fused where the plan allows)
    const size_t xs = sizeof(float) * (size_t)p->d.S * p->rows_tot[0];
    float* x = (float*)wsb;
    float* g = (float*)(wsb + align256(xs));
    // corr / m / v live in the tiled layout for the whole loop when the plan allows
    float* ts = tiled_ok(p) ? (float*)(wsb + align256(p->ws_bytes) + 2 * loop_ebuf_bytes(p))
                            : nullptr;
    // Philox mode: eps, eps' and G are the loop's own buffers -- their 64-float
    // pads are zeroed with the tiled conversion and the streaming update reads
    // them unclamped
    const bool padded = ts && !eps;
    // Philox mode on a bf-stream plan: every draw also as bf16 planes, one
    // plane buffer per eps buffer (their row pads zeroed here, never drawn)
    uint16_t* pbuf[2] = {nullptr, nullptr};
    if (padded && p->bf_stream) {
        char* pb = wsb + align256(p->ws_bytes) + 2 * loop_ebuf_bytes(p) +
                   align256(sizeof(float) * tiled_floats(p));
        pbuf[0] = (uint16_t*)pb;
        pbuf[1] = (uint16_t*)(pb + loop_pbuf_bytes(p));
    }
    float* pads[3] = {padded ? ebuf[0] + p->Peps : nullptr, padded ? ebuf[1] + p->Peps : nullptr,
                      padded ? g + (size_t)p->d.S * p->rows_tot[0] : nullptr};
    if (T == 0) return 0;
    // resident state of the last KEEP call (dropped by every call; taken up by
    // a RESUME call that continues it)
    const psvi_plan::Resident res = p->resident;
    p->resident.valid = false;
    const bool keep = (flags & PSVI_LOOP_KEEP) && padded;
    const bool resume = (flags & PSVI_LOOP_RESUME) && padded && res.valid && res.ws == ws &&
                        res.params == params && res.m == adam_m && res.v == adam_v &&
                        res.seed == seed && res.offset == offset;
    // eps buffer of step t (a resumed loop's step 0 is where the last one left it)
    const int eb0 = resume ? res.ebuf : 0;
    auto bi = [&](int t) { return (t + eb0) & 1; };
    bool join = false;
    const float* e;
    if (resume) {
        // the tiled state, step 0's eps (+ planes) and x are in ws already; the
        // ELBO accumulators cleared by the draw kernel's zero-fill with no draw
        // (a library kernel: hipMemsetAsync's first use in a process loads the
        // runtime's own fill kernels inside the caller's timed region)
        RandnLaunch clear;
        clear.out = ebuf[1 - bi(0)]; clear.zero = elbo_out; clear.nzero = T;
        HIP_TRY(launch_randn(clear, st));
        e = ebuf[bi(0)];
    } else {
        // packed -> tiled state on the plan's conversion stream, behind x_0 and the
        // first network step (joined before the first update)
        if (ts && p->aux.st) {
            HIP_TRY(hipEventRecord(p->aux.fork, st));
            HIP_TRY(hipStreamWaitEvent(p->aux.st, p->aux.fork, 0));
            HIP_TRY(launch_mvn_tile_convert(*p, params, adam_m, adam_v, ts, true, p->aux.st, pads));
            HIP_TRY(hipEventRecord(p->aux.join, p->aux.st));
            join = true;
        } else if (ts) {
            HIP_TRY(launch_mvn_tile_convert(*p, params, adam_m, adam_v, ts, true, st, pads));
        }
        if (pbuf[0]) {
            HIP_TRY(hipMemsetAsync(pbuf[0], 0, 2 * loop_pbuf_bytes(p), st));
            RandnLaunch r = rn;
            r.out = ebuf[0]; r.offset = offset; r.zero = elbo_out; r.nzero = T;
            r.planes_desc = &p->eps_planes; r.planes = pbuf[0];
            HIP_TRY(launch_randn(r, st));
            e = ebuf[0];
        } else {
            e = first_eps();
        }
        if (!e) return fail(PSVI_EUNSUP, "randn launch failed");
        HIP_TRY(launch_mvn_fwd(*p, e, params, x, st));
    }
    for (int t = 0; t < T; ++t) {
        h.step = hp->step + t;
        // Philox mode: the network kernel also draws the next step's eps (KEEP:
        // the last step too, for the next call)
        const bool last = t + 1 == T;
        const bool draw = !eps && (!last || keep);
        float* en_buf = draw ? ebuf[bi(t + 1)] : nullptr;
        uint16_t* en_pl = draw ? pbuf[bi(t + 1)] : nullptr;
        const bool tm = g_loop_every > 0 && t % g_loop_every == 0;
        if (tm) HIP_TRY(loop_event(0, st));
        NetLaunch n = net_rows(u, zt, w, elbo_out + t);
        n.xrecv = x; n.gsend = g;
        n.draw.out = en_buf; n.draw.n = draw ? p->Peps : 0; n.draw.planes = en_pl;
        n.draw.seed = seed; n.draw.offset = offset + (uint64_t)(t + 1) * es;
        HIP_TRY(launch_net(*p, n, st));
        if (tm) HIP_TRY(loop_event(0, st));
        const float* en = !last ? (eps ? eps + (size_t)(t + 1) * p->Peps : en_buf) : (keep ? en_buf : nullptr);
        if (tm) HIP_TRY(loop_event(1, st));
        if (join) {
            HIP_TRY(hipStreamWaitEvent(st, p->aux.join, 0));
            join = false;
        }
        // the last step (no next sample) writes corr / m / v back to the packed
        // arrays; KEEP: it samples as every step, then the tiled state is copied out
        MvnUpdate up = mvn_step(e, g, params, adam_m, adam_v, &h, elbo_out + t, 1);
        up.tstate = ts; up.packed_out = ts && !en; up.padded = padded; up.eps_planes = pbuf[bi(t)];
        if (en) {
            up.next.eps = en; up.next.x = x; up.next.planes = en_pl;
        }
        HIP_TRY(launch_mvn_update(*p, up, st));
        if (tm) HIP_TRY(loop_event(1, st));
        e = en;
    }
    if (keep) {
        HIP_TRY(launch_mvn_tile_convert(*p, params, adam_m, adam_v, ts, false, st, nullptr));
        p->resident = psvi_plan::Resident{true, ws, params, adam_m, adam_v, seed,
                                          offset + (uint64_t)T * es, bi(T)};
    }
    return 0;
}

// ext_coef == nullptr: the whole objective (stats, forward, combine, backward).
// Otherwise [rowcoef (S x 2) | ck (S) | sck (1)] replace the combine: the
// backward of a caller-formed softmax over samples (sample-sharded outer).
static int outer_impl(const psvi_plan* p, int32_t n_pseudo, const float* x_all,
                      const int32_t* z_abi, const float* w_all, const float* eps,
                      const float* params, double* loss_out, float* grad_params,
                      float* grad_u, float* grad_w, double* sample_out,
                      const float* ext_coef, void* ws, size_t ws_bytes, void* stream,
                      int ablated = 0, float* grad_z = nullptr) {
    drop_resident(p);
    if (int rc = check_plan(p)) return rc;
    if (int rc = refuse_bernoulli(p, "the outer objective has no Bernoulli-likelihood form "
                                     "(psvi_row_loglik + psvi_select_weight_grad)"))
        return rc;
    if (p->world != 1) return fail(PSVI_ESTATE, "the outer objective needs world == 1");
    if (p->d.S < 1) return fail(PSVI_EINVAL, "S must be >= 1");
    if (p->d.S > 2048) return fail(PSVI_EUNSUP, "the outer objective supports S <= 2048");
    if (n_pseudo < 0 || n_pseudo > p->d.M) return fail(PSVI_EINVAL, "n_pseudo out of [0, M]");
    if (!x_all || !z_abi || !w_all || !eps || !params || (!loss_out && !ext_coef))
        return fail(PSVI_EINVAL, "null pointer");
    const Targets z_all = abi_targets(p, z_abi);
    if (grad_u && !grad_params)
        return fail(PSVI_EINVAL, "grad_u needs grad_params (one backward pass gives both)");
    if (grad_z && p->lik != PSVI_LIK_GAUSSIAN)
        return fail(PSVI_ESTATE, "grad_z needs a Gaussian-likelihood plan");
    if (grad_z && !grad_params)
        return fail(PSVI_EINVAL, "grad_z needs grad_params (one backward pass gives both)");
    if (ablated && p->lik == PSVI_LIK_GAUSSIAN)
        return fail(PSVI_EUNSUP, "the ablated outer objective has no Gaussian-likelihood form");
    const OuterWs o = outer_ws(p, ws);
    if (!ws || ws_bytes < o.bytes) return fail(PSVI_ENOSPC, "workspace too small");
    hipStream_t st = as_stream(stream);
    char* wsb = (char*)ws;
    float* x = nullptr;
    float* g = nullptr;
    float* acc = nullptr;
    if (p->family == PSVI_FAMILY_FULLCOV) {
        const size_t xs = sizeof(float) * (size_t)p->d.S * p->rows_tot[0];
        x = (float*)wsb;
        g = (float*)(wsb + align256(xs));
        HIP_TRY(launch_mvn_fwd(*p, eps, params, x, st));
    } else {
        acc = (float*)wsb;
    }
    if (!ext_coef) HIP_TRY(launch_outer_stats(*p, params, eps, x, o.stats, st));
    // 1. forward: every row's NLL
    NetOuter fw{1, n_pseudo, o.nll, nullptr, nullptr, nullptr};
    NetLaunch n = net_rows(x_all, z_all, w_all, nullptr);
    n.params = params; n.eps = eps; n.xrecv = x; n.outer = &fw;
    if (p->family == PSVI_FAMILY_LENET)
        HIP_TRY(launch_lenet(*p, x_all, z_all.slots(), w_all, params, eps, nullptr, nullptr,
                             p->lenet_scratch.dev, st, &fw));
    else
        HIP_TRY(launch_net(*p, n, st));
    if (!ext_coef) {
        // 2. per-sample terms, softmax over samples, loss, backward coefficients
        HIP_TRY(launch_outer_combine(*p, n_pseudo, params, w_all, o.nll, o.stats, loss_out,
                                     o.rowcoef, o.ck, o.sck, grad_w, sample_out, ablated, st));
    } else {
        const size_t S = p->d.S;
        HIP_TRY(hipMemcpyAsync(o.rowcoef, ext_coef, sizeof(float) * 2 * S,
                               hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(o.ck, ext_coef + 2 * S, sizeof(float) * S,
                               hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(o.sck, ext_coef + 3 * S, sizeof(float), hipMemcpyDeviceToDevice,
                               st));
        if (grad_w) HIP_TRY(launch_outer_gradw(*p, n_pseudo, o.nll, o.rowcoef, grad_w, st));
    }
    if (!grad_params) return 0;
    // 3. backward through the network with the row coefficients (+ sampled-KL path)
    NetOuter bw{2, n_pseudo, nullptr, o.rowcoef, o.ck, grad_u ? o.du : nullptr, nullptr,
                grad_z ? o.dz : nullptr};
    NetLaunch b = net_rows(x_all, z_all, w_all, nullptr);
    b.outer = &bw;
    if (p->family == PSVI_FAMILY_FULLCOV) {
        b.xrecv = x; b.gsend = g;
        HIP_TRY(launch_net(*p, b, st));
        // 4. reparameterised backward (no KL term: the sampled KL came in through G)
        MvnUpdate up;
        up.eps = eps; up.g_shard = g; up.params = const_cast<float*>(params);
        up.grad_out = grad_params;
        HIP_TRY(launch_mvn_update(*p, up, st));
    } else {
        MfUpdate up;
        up.params = const_cast<float*>(params); up.grad_out = grad_params;
        if (p->family == PSVI_FAMILY_LENET) {
            HIP_TRY(launch_lenet(*p, x_all, z_all.slots(), w_all, params, eps, acc, nullptr,
                                 p->lenet_scratch.dev, st, &bw));
            up.acc = acc;
        } else {
            b.params = params; b.eps = eps; b.mf_slots = p->mf_slots.dev;
            HIP_TRY(launch_net(*p, b, st));
            up.slot_eps = eps;
        }
        HIP_TRY(launch_mf_update(*p, up, st));
    }
    // 5. explicit log-det term on the scales; d loss / d u
    HIP_TRY(launch_outer_finish(*p, n_pseudo, params, o.sck, grad_params, o.du, grad_u, st));
    if (grad_z) HIP_TRY(launch_sample_sum(p->d.S, n_pseudo, o.dz, grad_z, st));
    return 0;
}

static size_t eval_prob_off(const psvi_plan* p) { return outer_ws(p, nullptr).bytes; }

int psvi_outer_elbo_grad(const psvi_plan* p, int32_t n_pseudo, const float* x_all,
                         const int32_t* z_all, const float* w_all, const float* eps,
                         const float* params, double* loss_out, float* grad_params,
                         float* grad_u, float* grad_w, double* sample_out, void* ws,
                         size_t ws_bytes, void* stream) {
    return psvi_outer_elbo_grad_ex(p, n_pseudo, x_all, z_all, w_all, eps, params, loss_out,
                                   grad_params, grad_u, grad_w, nullptr, sample_out, ws, ws_bytes,
                                   stream);
}

int psvi_outer_elbo_grad_ex(const psvi_plan* p, int32_t n_pseudo, const float* x_all,
                            const int32_t* z_all, const float* w_all, const float* eps,
                            const float* params, double* loss_out, float* grad_params,
                            float* grad_u, float* grad_w, float* grad_z, double* sample_out,
                            void* ws, size_t ws_bytes, void* stream) {
    return outer_impl(p, n_pseudo, x_all, z_all, w_all, eps, params, loss_out, grad_params,
                      grad_u, grad_w, sample_out, nullptr, ws, ws_bytes, stream, 0, grad_z);
}

int psvi_outer_ablated_elbo_grad(const psvi_plan* p, const float* x_all,
                                 const int32_t* z_all, const float* w_all, const float* eps,
                                 const float* params, double* loss_out, float* grad_params,
                                 double* sample_out, void* ws, size_t ws_bytes, void* stream) {
    if (p && p->family == PSVI_FAMILY_FULLCOV)
        return fail(PSVI_EUNSUP, "PSVI_Ablated's sampled KL sums VILinear layers only; a "
                                 "full-covariance model has none (the reference fails there)");
    return outer_impl(p, 0, x_all, z_all, w_all, eps, params, loss_out, grad_params, nullptr,
                      nullptr, sample_out, nullptr, ws, ws_bytes, stream, 1);
}

int psvi_outer_elbo_grad_coef(const psvi_plan* p, int32_t n_pseudo, const float* x_all,
                              const int32_t* z_all, const float* w_all, const float* eps,
                              const float* params, const float* coef, float* grad_params,
                              float* grad_u, float* grad_w, void* ws, size_t ws_bytes,
                              void* stream) {
    return psvi_outer_elbo_grad_coef_ex(p, n_pseudo, x_all, z_all, w_all, eps, params, coef,
                                        grad_params, grad_u, grad_w, nullptr, ws, ws_bytes,
                                        stream);
}

int psvi_outer_elbo_grad_coef_ex(const psvi_plan* p, int32_t n_pseudo, const float* x_all,
                                 const int32_t* z_all, const float* w_all, const float* eps,
                                 const float* params, const float* coef, float* grad_params,
                                 float* grad_u, float* grad_w, float* grad_z, void* ws,
                                 size_t ws_bytes, void* stream) {
    if (!coef) return fail(PSVI_EINVAL, "null coefficients");
    return outer_impl(p, n_pseudo, x_all, z_all, w_all, eps, params, nullptr, grad_params,
                      grad_u, grad_w, nullptr, coef, ws, ws_bytes, stream, 0, grad_z);
}

int psvi_evaluate(const psvi_plan* p, int32_t n_pseudo, const float* x_all, const int32_t* z_all,
                  const float* w_all, const float* eps, const float* params, int32_t correction,
                  float* probs_out, double* stats_out, void* ws, size_t ws_bytes, void* stream) {
    drop_resident(p);
    if (int rc = check_plan(p)) return rc;
    if (p->world != 1) return fail(PSVI_ESTATE, "evaluate needs world == 1");
    if (int rc = refuse_bernoulli(p, "a Bernoulli-likelihood plan predicts from psvi_row_loglik"))
        return rc;
    if (p->lik != PSVI_LIK_CATEGORICAL)
        return fail(PSVI_ESTATE, "a Gaussian-likelihood plan evaluates with "
                                 "psvi_evaluate_regression");
    if (p->d.S < 2) return fail(PSVI_EINVAL, "evaluate needs S > 1 (psvi_classes.py:1036)");
    if (p->d.S > 2048) return fail(PSVI_EUNSUP, "evaluate supports S <= 2048");
    if (n_pseudo < 0 || n_pseudo > p->d.M) return fail(PSVI_EINVAL, "n_pseudo out of [0, M]");
    if (!x_all || !z_all || !w_all || !eps || !params || !stats_out)
        return fail(PSVI_EINVAL, "null pointer");
    if (!ws || ws_bytes < eval_ws_bytes(p)) return fail(PSVI_ENOSPC, "workspace too small");
    hipStream_t st = as_stream(stream);
    const OuterWs o = outer_ws(p, ws);
    char* wsb = (char*)ws;
    float* prob = (float*)(wsb + eval_prob_off(p));
    float* W = (float*)(wsb + eval_prob_off(p) +
                        align256(sizeof(float) * (size_t)p->d.S * p->d.M * p->lay[p->L - 1].dout));
    float* x = nullptr;
    if (p->family == PSVI_FAMILY_FULLCOV) {
        x = (float*)wsb;
        HIP_TRY(launch_mvn_fwd(*p, eps, params, x, st));
    }
    HIP_TRY(launch_outer_stats(*p, params, eps, x, o.stats, st));
    NetOuter fw{1, n_pseudo, o.nll, nullptr, nullptr, nullptr, prob};
    NetLaunch n = net_rows(x_all, Targets::labels(z_all), w_all, nullptr);
    n.params = params; n.eps = eps; n.xrecv = x; n.outer = &fw;
    if (p->family == PSVI_FAMILY_LENET)
        HIP_TRY(launch_lenet(*p, x_all, z_all, w_all, params, eps, nullptr, nullptr,
                             p->lenet_scratch.dev, st, &fw));
    else
        HIP_TRY(launch_net(*p, n, st));
    HIP_TRY(launch_eval(*p, n_pseudo, params, w_all, z_all, o.nll, o.stats, prob,
                        correction ? 1 : 0, W, probs_out, stats_out, st));
    return 0;
}

int psvi_evaluate_regression(const psvi_plan* p, int32_t n_pseudo, const float* x_all,
                             const float* y_all, const float* w_all, const float* eps,
                             const float* params, int32_t correction, float y_mean, float y_std,
                             float* pred_out, double* stats_out, void* ws, size_t ws_bytes,
                             void* stream) {
    drop_resident(p);
    if (int rc = check_plan(p)) return rc;
    if (int rc = refuse_bernoulli(p, "a Bernoulli-likelihood plan predicts from psvi_row_loglik"))
        return rc;
    if (p->lik != PSVI_LIK_GAUSSIAN)
        return fail(PSVI_ESTATE, "psvi_evaluate_regression needs a Gaussian-likelihood plan");
    if (p->d.S < 2) return fail(PSVI_EINVAL, "evaluate needs S > 1 (psvi_classes.py:2229)");
    if (p->d.S > 2048) return fail(PSVI_EUNSUP, "evaluate supports S <= 2048");
    if (n_pseudo < 0 || n_pseudo > p->d.M) return fail(PSVI_EINVAL, "n_pseudo out of [0, M]");
    if (!x_all || !y_all || !w_all || !eps || !params || !stats_out)
        return fail(PSVI_EINVAL, "null pointer");
    if (!ws || ws_bytes < eval_ws_bytes(p)) return fail(PSVI_ENOSPC, "workspace too small");
    hipStream_t st = as_stream(stream);
    const OuterWs o = outer_ws(p, ws);
    char* wsb = (char*)ws;
    float* f = (float*)(wsb + eval_prob_off(p));  // the data rows' outputs [S][M - n_pseudo]
    float* W = (float*)(wsb + eval_prob_off(p) +
                        align256(sizeof(float) * (size_t)p->d.S * p->d.M));
    HIP_TRY(launch_outer_stats(*p, params, eps, nullptr, o.stats, st));
    NetOuter fw{1, n_pseudo, o.nll, nullptr, nullptr, nullptr, f};
    NetLaunch n = net_rows(x_all, Targets::values(y_all), w_all, nullptr);
    n.params = params; n.eps = eps; n.outer = &fw;
    HIP_TRY(launch_net(*p, n, st));
    HIP_TRY(launch_eval_regression(*p, n_pseudo, params, y_all + n_pseudo, o.stats, f,
                                   correction ? 1 : 0, y_mean, y_std, W, pred_out, stats_out, st));
    return 0;
}

int psvi_sampled_kl_grad(const psvi_plan* p, const float* eps, const float* params,
                         double* nkl_out, float* grad_out, void* stream) {
    drop_resident(p);
    if (int rc = check_plan(p, 1u << PSVI_FAMILY_MEANFIELD, kNotMf)) return rc;
    if (p->world != 1) return fail(PSVI_EUNSUP, "the sampled KL term needs world == 1");
    if (!eps || !params || (!nkl_out && !grad_out)) return fail(PSVI_EINVAL, "null pointer");
    HIP_TRY(launch_mf_sampled_kl(*p, eps, params, nkl_out, grad_out, as_stream(stream)));
    return 0;
}

int psvi_row_loglik(const psvi_plan* p, const float* x_all, const int32_t* z_all,
                    const float* eps, const float* params, float* ll_out, float* logits_out,
                    double* nkl_out, void* stream) {
    drop_resident(p);
    if (int rc = check_plan(p)) return rc;
    if (p->lik != PSVI_LIK_BERNOULLI)
        return fail(PSVI_ESTATE, "psvi_row_loglik needs a Bernoulli-likelihood plan");
    if (p->d.S > 2048) return fail(PSVI_EUNSUP, "psvi_row_loglik supports S <= 2048");
    if (!x_all || !z_all || !eps || !params || !ll_out) return fail(PSVI_EINVAL, "null pointer");
    hipStream_t st = as_stream(stream);
    // the forward pass of the outer objective: every row's -NLL, the raw
    // output of the rows past n_pseudo = 0.  The forward reads no row weight:
    // its weight slots load the first M floats of x_all.
    NetOuter fw{1, 0, ll_out, nullptr, nullptr, nullptr, logits_out, nullptr};
    fw.loglik = true;
    NetLaunch n = net_rows(x_all, Targets::labels(z_all), x_all, nullptr);
    n.params = params; n.eps = eps; n.outer = &fw;
    HIP_TRY(launch_net(*p, n, st));
    if (nkl_out) HIP_TRY(launch_mf_sampled_kl(*p, eps, params, nkl_out, nullptr, st));
    return 0;
}

int psvi_select_scores(int32_t S, int32_t n_core, int32_t n_data, const float* ll,
                       const double* nkl, const float* w_core, double sum_scaling, float* W_out,
                       float* corr_out, float* corecorr_out, double* result_out, void* stream) {
    if (S < 2 || n_core < 0 || n_data < 1) return fail(PSVI_EINVAL, "bad selection shape");
    if (S > 2048) return fail(PSVI_EUNSUP, "the selection scores support S <= 2048");
    if (!ll || !nkl || !W_out || !corr_out || !result_out ||
        (n_core > 0 && (!w_core || !corecorr_out)))
        return fail(PSVI_EINVAL, "null pointer");
    HIP_TRY(launch_select_scores(S, n_core, n_data, ll, nkl, w_core, sum_scaling, W_out, corr_out,
                                 corecorr_out, result_out, as_stream(stream)));
    return 0;
}

int psvi_select_weight_grad(int32_t S, int32_t n_core, int32_t n_data, const float* ll,
                            const double* nkl, const float* w_core, double N, double* loss_out,
                            float* grad_w, void* stream) {
    if (S < 2 || n_core < 1 || n_data < 1) return fail(PSVI_EINVAL, "bad selection shape");
    if (S > 2048) return fail(PSVI_EUNSUP, "the weight objective supports S <= 2048");
    if (!ll || !nkl || !w_core || !loss_out || !grad_w) return fail(PSVI_EINVAL, "null pointer");
    HIP_TRY(launch_select_weight_grad(S, n_core, n_data, ll, nkl, w_core, N, loss_out, grad_w,
                                      as_stream(stream)));
    return 0;
}

int psvi_laplace_fit(const psvi_laplace_fit_req* q, void* stream) {
    if (!q) return fail(PSVI_EINVAL, "null request");
    if (q->d < 2 || q->d > kLapMaxD || q->n_core < 0 || q->n_core > kLapMaxNu || q->S < 0 ||
        q->S > 2048 || q->T < 0 || q->T > kLapMaxT)
        return fail(PSVI_EINVAL, "the Laplace fit supports 2 <= d <= 256, 0 <= n_core <= 4096, "
                                 "0 <= S <= 2048, 0 <= T <= 1048576");
    auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
    if (!pos(q->lr) || !pos(q->beta1) || !pos(q->beta2) || q->beta1 >= 1.0 || q->beta2 >= 1.0 ||
        !pos(q->adam_eps) || !pos(q->prior_sd) || !std::isfinite(q->prior_mean))
        return fail(PSVI_EINVAL, "bad Adam constants or prior");
    if (!q->theta || !q->prec_out || (q->n_core > 0 && (!q->x_core || !q->y_core || !q->w_core)) ||
        (q->eps && (!q->samples_out || q->S < 1)))
        return fail(PSVI_EINVAL, "null pointer");
    hipStream_t st = as_stream(stream);
    if (q->n_core > 0) {
        // zero weights add nothing to the reference's masked precision sum; negative ones would
        std::vector<float> w(q->n_core);
        HIP_TRY(hipMemcpyAsync(w.data(), q->w_core, sizeof(float) * w.size(), hipMemcpyDeviceToHost,
                               st));
        HIP_TRY(hipStreamSynchronize(st));
        for (float v : w)
            if (!(v >= 0.0f) || !std::isfinite(v))
                return fail(PSVI_EINVAL, "the Laplace fit needs finite weights >= 0");
    }
    LaplaceFit r;
    r.Nu = q->n_core; r.d = q->d; r.S = q->eps ? q->S : 0; r.T = q->T;
    r.x = q->x_core; r.y = q->y_core; r.w = q->w_core;
    r.mu0 = q->prior_mean; r.sd0 = q->prior_sd;
    r.theta = q->theta;
    r.lr = q->lr; r.beta1 = q->beta1; r.beta2 = q->beta2; r.adam_eps = q->adam_eps;
    r.eps = q->eps; r.loss_out = q->loss_out; r.prec_out = q->prec_out;
    r.samples_out = q->samples_out;
    HIP_TRY(launch_laplace_fit(r, st));
    return 0;
}

namespace {
// the descriptor's ranges of psvi_mfvi_fit and its shape; 0 or an error code
int mfvi_fit_desc(const psvi_net_desc* d, MfviFitShape& s) {
    if (!d) return fail(PSVI_EINVAL, "null descriptor");
    if (d->n_layers < 2 || d->n_layers > kMfFitMaxL)
        return fail(PSVI_EINVAL, "the MFVI fit supports 2 <= n_layers <= 4 (1..3 hidden layers)");
    if (d->dims[0] < 1 || d->dims[0] > kMfFitMaxD)
        return fail(PSVI_EINVAL, "the MFVI fit supports 1 <= dims[0] <= 128");
    for (int l = 1; l < d->n_layers; ++l)
        if (d->dims[l] < 1 || d->dims[l] > kMfFitMaxH)
            return fail(PSVI_EINVAL, "the MFVI fit supports hidden dims in [1, 64]");
    if (d->dims[d->n_layers] != 1) return fail(PSVI_EINVAL, "the MFVI fit needs one network output");
    if (d->M < 1 || d->M > kMfFitMaxB) return fail(PSVI_EINVAL, "the MFVI fit supports 1 <= M <= 512");
    if (d->S < 1 || d->S > kMfFitMaxS) return fail(PSVI_EINVAL, "the MFVI fit supports 1 <= S <= 64");
    if (!(d->prior_sd > 0.f) || !std::isfinite(d->prior_sd))
        return fail(PSVI_EINVAL, "prior_sd must be finite and > 0");
    if (mfvi_fit_shape(*d, s) != 0)
        return fail(PSVI_EUNSUP, "the MFVI fit's working set does not fit the LDS");
    return 0;
}
}  // namespace

int psvi_mfvi_fit_query(const psvi_net_desc* d, int64_t* out) {
    MfviFitShape s;
    if (int rc = mfvi_fit_desc(d, s)) return rc;
    if (!out) return fail(PSVI_EINVAL, "null pointer");
    out[0] = s.lds ? 1 : 0;
    out[1] = (int64_t)s.ws_bytes;
    out[2] = 2 * (int64_t)s.n_tot;
    out[3] = s.eps_count;
    return 0;
}

int psvi_mfvi_fit(const psvi_mfvi_fit_req* q, void* stream) {
    if (!q) return fail(PSVI_EINVAL, "null request");
    MfviFit r;
    if (int rc = mfvi_fit_desc(q->desc, r.shape)) return rc;
    if (q->G < 1 || q->G > kMfFitMaxG) return fail(PSVI_EINVAL, "the MFVI fit supports 1 <= G <= 16");
    if (q->T < 0 || q->T > kMfFitMaxT) return fail(PSVI_EINVAL, "the MFVI fit supports 0 <= T <= 1048576");
    if (q->step0 < 0 || (int64_t)q->step0 + q->T > (int64_t(1) << 30))
        return fail(PSVI_EINVAL, "the MFVI fit supports 0 <= step0, step0 + T <= 2^30");
    auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
    if (!pos(q->lr) || !pos(q->beta1) || !pos(q->beta2) || q->beta1 >= 1.0 || q->beta2 >= 1.0 ||
        !pos(q->adam_eps) || !pos(q->scale))
        return fail(PSVI_EINVAL, "bad Adam constants or scale");
    if (!q->x || !q->y || !q->tau || !q->params || !q->adam_m || !q->adam_v ||
        (!q->eps && !q->offset))
        return fail(PSVI_EINVAL, "null pointer");
    for (int g = 0; g < q->G; ++g) {
        if (!pos(q->tau[g])) return fail(PSVI_EINVAL, "tau must be finite and > 0");
        if (!q->eps && (q->offset[g] & 3)) return fail(PSVI_EINVAL, "offset must be a multiple of 4");
    }
    const size_t need = r.shape.ws_bytes * (size_t)q->G;
    if (need > 0 && !q->ws) return fail(PSVI_EINVAL, "null pointer");
    if (q->ws_bytes < need) return fail(PSVI_ENOSPC, "workspace too small");
    for (int l = 0; l <= q->desc->n_layers; ++l) r.dims[l] = q->desc->dims[l];
    r.G = q->G; r.T = q->T; r.step0 = q->step0;
    r.x = q->x; r.y = q->y; r.scale = q->scale; r.prior_sd = q->desc->prior_sd;
    r.tau = q->tau; r.offset = q->eps ? nullptr : q->offset; r.seed = q->seed; r.eps = q->eps;
    r.params = q->params; r.m = q->adam_m; r.v = q->adam_v;
    r.lr = q->lr; r.beta1 = q->beta1; r.beta2 = q->beta2; r.adam_eps = q->adam_eps;
    r.loss_out = q->loss_out; r.ws = q->ws;
    HIP_TRY(launch_mfvi_fit(r, as_stream(stream)));
    return 0;
}

int psvi_predict_scores(const psvi_predict_scores_req* q, void* stream) {
    if (!q) return fail(PSVI_EINVAL, "null request");
    const psvi_plan* p = q->plan;
    if (!p) return fail(PSVI_EINVAL, "null plan");
    if (p->family != PSVI_FAMILY_MEANFIELD || p->lik != PSVI_LIK_CATEGORICAL || p->world != 1)
        return fail(PSVI_ESTATE, "the predictive scores need a mean-field categorical plan of world 1");
    if (q->n_rows < 1 || q->rows_per_draw < 1)
        return fail(PSVI_EINVAL, "n_rows and rows_per_draw must be >= 1");
    if (!q->x || !q->eps || !q->params) return fail(PSVI_EINVAL, "null pointer");
    const int n_state = (q->last_acc != nullptr) + (q->forgetting != nullptr) + (q->never_learnt != nullptr);
    if (n_state != 0 && n_state != 3)
        return fail(PSVI_EINVAL, "last_acc, forgetting and never_learnt are given together or not at all");
    if (!q->mean_logits && !q->least_conf && !q->entropy && !q->el2n && !q->correct && !n_state &&
        !q->stats_out)
        return fail(PSVI_EINVAL, "no output requested");
    if ((q->el2n || q->correct || n_state || q->stats_out) && !q->z)
        return fail(PSVI_EINVAL, "el2n, correct, the forgetting state and stats_out need the labels z");
    PredictScores r;
    if (predict_shape(*p, q->rows_per_draw, r.shape) != 0)
        return fail(PSVI_EUNSUP, "a layer of the network does not fit the predictive scores' LDS "
                                 "budget: one unit's weights and one row's activations exceed 160 KiB");
    if (!p->on_device) return fail(PSVI_ESTATE, "plan was created without a HIP device");
    r.n_rows = q->n_rows; r.rpd = q->rows_per_draw;
    r.x = q->x; r.z = q->z; r.eps = q->eps; r.params = q->params;
    r.mean_logits = q->mean_logits; r.least_conf = q->least_conf; r.entropy = q->entropy;
    r.el2n = q->el2n; r.correct = q->correct;
    r.last_acc = q->last_acc; r.forgetting = q->forgetting; r.never_learnt = q->never_learnt;
    r.stats_out = q->stats_out;
    HIP_TRY(launch_predict_scores(*p, r, as_stream(stream)));
    return 0;
}

int psvi_laplace_sample_full(const psvi_laplace_sample_full_req* q, void* stream) {
    if (!q) return fail(PSVI_EINVAL, "null request");
    if (q->d < 2 || q->d > kLapFullMaxD || q->n_core < 0 || q->n_core > kLapMaxNu || q->S < 0 ||
        q->S > 2048)
        return fail(PSVI_EINVAL, "the full-precision Laplace samples support 2 <= d <= 128, "
                                 "0 <= n_core <= 4096, 0 <= S <= 2048");
    if (!q->theta || (q->n_core > 0 && (!q->x_core || !q->w_core)))
        return fail(PSVI_EINVAL, "null pointer");
    if ((q->eps != nullptr) != (q->S > 0))
        return fail(PSVI_EINVAL, "eps goes with S >= 1 and is NULL at S == 0");
    if (q->S > 0 && !q->samples_out)
        return fail(PSVI_EINVAL, "samples_out is required when S > 0");
    hipStream_t st = as_stream(stream);
    if (q->n_core > 0) {
        // as psvi_laplace_fit: zero weights add nothing, negative ones would break P >= I
        std::vector<float> w(q->n_core);
        HIP_TRY(hipMemcpyAsync(w.data(), q->w_core, sizeof(float) * w.size(), hipMemcpyDeviceToHost,
                               st));
        HIP_TRY(hipStreamSynchronize(st));
        for (float v : w)
            if (!(v >= 0.0f) || !std::isfinite(v))
                return fail(PSVI_EINVAL, "the full-precision Laplace samples need finite weights >= 0");
    }
    LaplaceSampleFull r;
    r.Nu = q->n_core; r.d = q->d; r.S = q->S;
    r.x = q->x_core; r.w = q->w_core; r.theta = q->theta; r.eps = q->eps;
    r.prec_out = q->prec_out; r.factor_out = q->factor_out; r.samples_out = q->samples_out;
    r.logdet_out = q->logdet_out;
    HIP_TRY(launch_laplace_sample_full(r, st));
    return 0;
}

int psvi_laplace_scores(const psvi_laplace_scores_req* q, void* stream) {
    if (!q) return fail(PSVI_EINVAL, "null request");
    if (q->S < 2 || q->S > 2048 || q->d < 2 || q->d > kLapMaxD || q->n_core < 0 ||
        q->n_data < 1 || (int64_t)q->n_core + q->n_data > kLapMaxRows)
        return fail(PSVI_EINVAL, "the Laplace scores support 2 <= S <= 2048, 2 <= d <= 256, "
                                 "n_data >= 1, n_core + n_data <= 2048");
    if (!q->samples || !q->rows || !q->labels || !q->corr_out || !q->result_out ||
        (q->n_core > 0 && (!q->w_core || !q->corecorr_out)))
        return fail(PSVI_EINVAL, "null pointer");
    LaplaceScores r;
    r.S = q->S; r.d = q->d; r.Nu = q->n_core; r.B = q->n_data;
    r.samples = q->samples; r.rows = q->rows; r.labels = q->labels; r.w = q->w_core;
    r.sum_scaling = q->sum_scaling;
    r.corr = q->corr_out; r.corecorr = q->corecorr_out; r.result = q->result_out;
    r.grad_w = q->grad_w; r.ll_out = q->ll_out; r.grad_u = q->grad_u;
    HIP_TRY(launch_laplace_scores(r, as_stream(stream)));
    return 0;
}

int psvi_giga_step(const psvi_giga_step_req* q, void* stream) {
    if (!q) return fail(PSVI_EINVAL, "null request");
    if (q->S < 2 || q->S > 2048 || q->d < 2 || q->d > kLapMaxD || q->n_data < 1 ||
        q->n_data > kLapMaxRows)
        return fail(PSVI_EINVAL, "the GIGA step supports 2 <= S <= 2048, 2 <= d <= 256, "
                                 "1 <= n_data <= 2048");
    if (!q->samples || !q->rows || !q->labels || !q->lw_in || !q->score_out || !q->lw_out ||
        !q->result_out)
        return fail(PSVI_EINVAL, "null pointer");
    if (q->lw_out < q->lw_in + q->S && q->lw_in < q->lw_out + q->S)
        return fail(PSVI_EINVAL, "lw_out must not alias lw_in");
    GigaStep r;
    r.S = q->S; r.d = q->d; r.n_data = q->n_data;
    r.samples = q->samples; r.rows = q->rows; r.labels = q->labels; r.lw_in = q->lw_in;
    r.score = q->score_out; r.lw_out = q->lw_out; r.ll_out = q->ll_out; r.result = q->result_out;
    HIP_TRY(launch_giga_step(r, as_stream(stream)));
    return 0;
}

int psvi_coreset_draw(const psvi_coreset_draw_req* q, void* stream) {
    if (!q) return fail(PSVI_EINVAL, "null request");
    if (!q->w || !q->idx_out || !q->status_out) return fail(PSVI_EINVAL, "null pointer");
    if (q->mode != PSVI_DRAW_REPLACE && q->mode != PSVI_DRAW_NOREPLACE)
        return fail(PSVI_EINVAL, "mode is PSVI_DRAW_REPLACE or PSVI_DRAW_NOREPLACE");
    if (q->offset % 4) return fail(PSVI_EINVAL, "draw offset must be a multiple of 4");
    if (q->M < 1 || q->n < 1 || q->n > kDrawMaxN || q->D < 0)
        return fail(PSVI_EINVAL, "the coreset draw supports M >= 1, 1 <= n <= 2^24, D >= 0");
    if ((q->rows && !q->rows_out) || (q->targets && !q->targets_out))
        return fail(PSVI_EINVAL, "rows / targets given without their output");
    if (q->M > kDrawMaxM)
        return fail(PSVI_EUNSUP, "the coreset draw holds its weights in LDS: M <= 4096");
    if (q->mode == PSVI_DRAW_NOREPLACE && q->n > q->M)
        return fail(PSVI_EINVAL, "a draw without replacement takes n <= M");
    CoresetDraw r;
    r.w = q->w; r.M = q->M; r.n = q->n; r.replace = q->mode == PSVI_DRAW_REPLACE;
    r.seed = q->seed; r.offset = q->offset;
    r.rows = q->rows; r.D = q->D; r.targets = q->targets;
    r.idx_out = q->idx_out; r.rows_out = q->rows_out; r.targets_out = q->targets_out;
    r.status_out = q->status_out;
    HIP_TRY(launch_coreset_draw(r, as_stream(stream)));
    return 0;
}

static int kmeans_range(int64_t N, int64_t D, int64_t K) {
    if (N < 1 || D < 1 || K < 1 || K > N)
        return fail(PSVI_EINVAL, "k-means takes N >= 1, D >= 1 and 1 <= K <= N");
    if (K > kKmMaxK || D > kKmMaxD || N > kKmMaxN)
        return fail(PSVI_EUNSUP, "k-means supports K <= 128, D <= 4096, N <= 2^24");
    return 0;
}

int psvi_kmeans_query(int32_t N, int32_t D, int32_t K, int64_t* out) {
    if (!out) return fail(PSVI_EINVAL, "null pointer");
    if (int rc = kmeans_range(N, D, K)) return rc;
    const KmeansShape s = kmeans_shape(N, D, K);
    out[0] = (int64_t)s.full_bytes;
    out[1] = (int64_t)s.min_bytes;
    out[2] = s.DT;
    out[3] = s.G;
    return 0;
}

int psvi_kmeans(const psvi_kmeans_req* q, void* stream) {
    if (!q) return fail(PSVI_EINVAL, "null request");
    if (!q->x || !q->centres_out || !q->labels_out || !q->counts_out || !q->inertia_out ||
        !q->n_iter_out || !q->status_out)
        return fail(PSVI_EINVAL, "null pointer");
    if (int rc = kmeans_range(q->N, q->D, q->K)) return rc;
    if (q->offset % 4) return fail(PSVI_EINVAL, "k-means offset must be a multiple of 4");
    if (q->max_iter < 0) return fail(PSVI_EINVAL, "max_iter must be >= 0");
    if (!(q->tol >= 0.0) || !std::isfinite(q->tol))
        return fail(PSVI_EINVAL, "tol must be finite and >= 0");
    if (!q->ws || q->ws_bytes < kmeans_shape(q->N, q->D, q->K).min_bytes)
        return fail(PSVI_ENOSPC, "workspace too small");
    Kmeans r;
    r.x = q->x; r.N = q->N; r.D = q->D; r.K = q->K;
    r.centres_in = q->centres_in; r.seed = q->seed; r.offset = q->offset;
    r.max_iter = q->max_iter; r.tol = q->tol;
    r.centres = q->centres_out; r.labels = q->labels_out; r.counts = q->counts_out;
    r.seeds = q->seeds_out; r.inertia = q->inertia_out; r.n_iter = q->n_iter_out;
    r.status = q->status_out; r.ws = q->ws; r.ws_bytes = q->ws_bytes;
    HIP_TRY(launch_kmeans(r, as_stream(stream)));
    return 0;
}

int psvi_hvp_partial(const psvi_plan* p, const float* u, const int32_t* z, const float* w,
                     const float* eps, const float* params, const float* vec,
                     int32_t include_kl, float* hv_out, float* du_out, float* dw_out, void* ws,
                     size_t ws_bytes, void* stream) {
    return psvi_hvp_ex(p, u, z, w, eps, params, vec, include_kl, hv_out, du_out, dw_out, nullptr,
                       ws, ws_bytes, stream);
}

int psvi_hvp_ex(const psvi_plan* p, const float* u, const int32_t* z, const float* w,
                const float* eps, const float* params, const float* vec, int32_t include_kl,
                float* hv_out, float* du_out, float* dw_out, float* dz_out, void* ws,
                size_t ws_bytes, void* stream) {
    drop_resident(p);
    if (int rc = check_plan(p)) return rc;
    if (int rc = refuse_bernoulli(p, "the R-op kernel has no Bernoulli head")) return rc;
    if (p->world != 1) return fail(PSVI_ESTATE, "psvi_hvp needs world == 1");
    if (!u || !z || !w || !eps || !params || !vec || !hv_out)
        return fail(PSVI_EINVAL, "null pointer");
    if (dz_out && p->lik != PSVI_LIK_GAUSSIAN)
        return fail(PSVI_ESTATE, "dz_out needs a Gaussian-likelihood plan");
    if (p->family == PSVI_FAMILY_LENET) {
        if (!ws || ws_bytes < lenet_tan_ws(*p, nullptr).bytes)
            return fail(PSVI_ENOSPC, "workspace too small");
        HIP_TRY(launch_lenet_hvp(*p, u, z, w, eps, params, vec, hv_out, du_out, dw_out, ws,
                                 as_stream(stream), include_kl != 0));
        return 0;
    }
    if (rop_rows(*p) == 0)
        return fail(PSVI_EUNSUP, "model too wide for the per-sample R-op kernel's LDS");
    const HvpWs o = hvp_ws(p, ws);
    if (!ws || ws_bytes < o.bytes) return fail(PSVI_ENOSPC, "workspace too small");
    hipStream_t st = as_stream(stream);
    float* x = nullptr;
    if (p->family == PSVI_FAMILY_FULLCOV) {
        x = (float*)ws;
        // x = mean + L eps; x_dot = v_mean + (sigmoid(sd) v_sd) eps + v_corr eps
        HIP_TRY(launch_mvn_fwd_pair(*p, eps, params, x, vec, o.xd, o.part2, st));
    }
    // two row-block slots per sample: added by their consumers (the K-split
    // gradient mode at staging, the assembly at its loads) rather than by a
    // slot-sum launch, when the K-split gradient mode runs
    const bool two = rop_splits(*p) == 2 &&
                     (p->family != PSVI_FAMILY_FULLCOV || mvn_grad_takes_slots(*p));
    const int64_t slot2 = two ? (int64_t)p->d.S * p->n_tot : 0;
    HvpAssemble asm_req;
    asm_req.params = params; asm_req.vec = vec; asm_req.eps = eps;
    asm_req.G = o.G; asm_req.Gd = o.Gd; asm_req.du = o.du; asm_req.nlld = o.nlld;
    asm_req.hv = hv_out; asm_req.d_u = du_out; asm_req.d_w = dw_out;
    asm_req.include_kl = include_kl != 0; asm_req.slot2 = slot2;
    NetRop rop;
    rop.u = u; rop.targets = abi_targets(p, z); rop.w = w; rop.x = x; rop.xd = o.xd;
    rop.params = params; rop.vec = vec; rop.eps = eps; rop.G = o.G; rop.Gd = o.Gd;
    if (du_out) rop.du = o.du;
    if (dw_out) rop.nlld = o.nlld;
    if (dz_out) rop.dzd = o.dzd;
    rop.sum_slots = !two;
    HIP_TRY(launch_net_rop(*p, rop, st));
    if (p->family == PSVI_FAMILY_FULLCOV) {  // J^T G_dot (mean, sd, corr; + the corr KL block)
        MvnUpdate up;
        up.eps = eps; up.g_shard = o.Gd; up.params = const_cast<float*>(params);
        up.grad_out = hv_out;
        if (include_kl) up.kl_vec = vec;
        if (two) up.g_shard2 = o.Gd + slot2;
        HIP_TRY(launch_mvn_update(*p, up, st));
    }
    HIP_TRY(launch_hvp_assemble(*p, asm_req, st));
    // d/dz_m (vec . d elbo / d params) = -sum_s delta_dot_sm, in sample order
    if (dz_out) HIP_TRY(launch_sample_sum(p->d.S, p->d.M, o.dzd, dz_out, st));
    return 0;
}

int psvi_hvp(const psvi_plan* p, const float* u, const int32_t* z, const float* w,
             const float* eps, const float* params, const float* vec, float* hv_out,
             float* du_out, float* dw_out, void* ws, size_t ws_bytes, void* stream) {
    return psvi_hvp_partial(p, u, z, w, eps, params, vec, 1, hv_out, du_out, dw_out, ws,
                            ws_bytes, stream);
}

int psvi_adam_adjoint(int64_t n, const float* lt, float* lm, float* lv, const float* adam_m,
                      const float* adam_v, const float* grad, float* lg_out,
                      const psvi_adam_hp* hp, void* stream) {
    if (n < 0 || !lt || !lm || !lv || !adam_m || !adam_v || !grad || !lg_out || !hp)
        return fail(PSVI_EINVAL, "bad adam adjoint arguments");
    if (hp->step < 1) return fail(PSVI_EINVAL, "adam step must be >= 1");
    if (hp->kind != PSVI_ADAM_HIGHER && hp->kind != PSVI_ADAM_HYPERGRAD)
        return fail(PSVI_EUNSUP, "adam adjoint: higher / hypergrad variants only");
    HIP_TRY(launch_adam_adjoint(n, lt, lm, lv, adam_m, adam_v, grad, lg_out, hp,
                                as_stream(stream)));
    return 0;
}

int psvi_nonfinite(const void* data, int64_t n, int32_t dtype, int32_t* flag, void* stream) {
    if (!data || !flag || n < 0 || (dtype != 0 && dtype != 1))
        return fail(PSVI_EINVAL, "bad nonfinite arguments");
    HIP_TRY(launch_nonfinite(data, n, dtype, flag, as_stream(stream)));
    return 0;
}

int psvi_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
    if (!out || n < 0) return fail(PSVI_EINVAL, "bad randn arguments");
    if (offset % 4) return fail(PSVI_EINVAL, "randn offset must be a multiple of 4");
    RandnLaunch r;
    r.out = out; r.n = n; r.seed = seed; r.offset = offset;
    HIP_TRY(launch_randn(r, as_stream(stream)));
    return 0;
}

int psvi_adam_update(int64_t n, float* params, const float* grad, float* adam_m, float* adam_v,
                     const psvi_adam_hp* hp, void* stream) {
    if (n < 0 || !params || !grad || !adam_m || !adam_v || !hp)
        return fail(PSVI_EINVAL, "bad adam arguments");
    if (int rc = check_adam(hp)) return rc;
    HIP_TRY(launch_adam(n, params, grad, adam_m, adam_v, hp, as_stream(stream)));
    return 0;
}

size_t psvi_cg_ws_bytes(void) { return cg_ws_bytes(); }

int psvi_cg_scale(int64_t n, const float* hv, double lr, float* out, void* stream) {
    if (n < 0 || !hv || !out) return fail(PSVI_EINVAL, "bad cg_scale arguments");
    HIP_TRY(launch_cg_scale(n, hv, lr, out, as_stream(stream)));
    return 0;
}

int psvi_cg_pap(int64_t n, const float* hv1, const float* hv2, double lr, const double* p,
                double* state, void* ws, size_t ws_bytes, void* stream) {
    if (n < 0 || !hv1 || !hv2 || !p || !state || !ws) return fail(PSVI_EINVAL, "bad cg_pap arguments");
    if (ws_bytes < cg_ws_bytes()) return fail(PSVI_EINVAL, "cg workspace too small");
    HIP_TRY(launch_cg_pap(n, hv1, hv2, lr, p, state, ws, as_stream(stream)));
    return 0;
}

int psvi_cg_residual(int64_t n, const float* hv1, const float* hv2, double lr, double* r,
                     double* state, double tol, void* ws, size_t ws_bytes, void* stream) {
    if (n < 0 || !hv1 || !hv2 || !r || !state || !ws)
        return fail(PSVI_EINVAL, "bad cg_residual arguments");
    if (ws_bytes < cg_ws_bytes()) return fail(PSVI_EINVAL, "cg workspace too small");
    HIP_TRY(launch_cg_residual(n, hv1, hv2, lr, r, state, tol, ws, as_stream(stream)));
    return 0;
}

int psvi_cg_update(int64_t n, double* x, double* p, float* p32, const double* r,
                   const double* state, void* stream) {
    if (n < 0 || !x || !p || !p32 || !r || !state) return fail(PSVI_EINVAL, "bad cg_update arguments");
    HIP_TRY(launch_cg_update(n, x, p, p32, r, state, as_stream(stream)));
    return 0;
}

}  // extern "C"
