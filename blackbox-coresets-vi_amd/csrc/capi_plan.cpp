// capi_plan.cpp -- extern "C" boundary of libpsvi_hip.so (declared in
// include/psvi_hip.h): plans, their queries and the diagnostics.  The fused
// entry points are in capi_inner.cpp and capi_outer.cpp, the plan-free tools in
// capi_tools.cpp.
//
// Plans hold the immutable geometry of one (family, layer sizes, S, M, world,
// rank) configuration: sample shards, nnz-balanced row shards of every
// full-cov layer, and the device work lists of the packed-triangular kernels
// (built on the host by plan_tables.cpp; uploaded and owned here).
// Steps are pure stream-ordered kernel launches + hipMemsetAsync (graph
// capturable: no allocation, no synchronisation).
#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "capi_common.hpp"

namespace psvi {
Diag g_diag;
thread_local std::string g_err;
}  // namespace psvi

using namespace psvi;

namespace {

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

std::vector<hipEvent_t> g_loop_ev[2];  // [net, update] x (start, end) pairs

void loop_events_clear() {
    for (auto& v : g_loop_ev) {
        for (hipEvent_t e : v) (void)hipEventDestroy(e);
        v.clear();
    }
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

int psvi::g_loop_every = 0;

hipError_t psvi::loop_event(int k, hipStream_t st) {
    hipEvent_t e;
    const hipError_t rc = hipEventCreate(&e);
    if (rc != hipSuccess) return rc;
    g_loop_ev[k].push_back(e);
    return hipEventRecord(e, st);
}

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

int psvi_plan_query(const psvi_plan* p, int32_t key, int64_t* value) {
    if (!p || !value) return fail(PSVI_EINVAL, "null argument");
    const int r = p->rank;
    switch (key) {
        case PSVI_Q_PARAM_COUNT: *value = p->P; break;
        case PSVI_Q_EPS_COUNT: *value = p->Peps; break;
        case PSVI_Q_WS_BYTES: *value = (int64_t)step_ws(*p, nullptr).bytes; break;
        case PSVI_Q_S_LOCAL: *value = p->s_cnt[r]; break;
        case PSVI_Q_S_OFFSET: *value = p->s_off[r]; break;
        case PSVI_Q_ACC_COUNT: *value = p->acc_count; break;
        case PSVI_Q_ROWS_LOCAL: *value = p->rows_tot[r]; break;
        case PSVI_Q_XSHARD_COUNT: *value = (int64_t)p->d.S * p->rows_tot[r]; break;
        case PSVI_Q_LOOP_WS_BYTES: *value = (int64_t)loop_ws(*p, nullptr).bytes; break;
        case PSVI_Q_TILED_FLOATS: *value = (int64_t)tiled_floats(*p); break;
        case PSVI_Q_XRECV_COUNT: *value = (int64_t)p->s_cnt[r] * p->n_tot; break;
        case PSVI_Q_OUTER_WS_BYTES: *value = (int64_t)outer_ws(*p, nullptr).bytes; break;
        case PSVI_Q_HVP_WS_BYTES:  // LeNet: the tangent scratch of launch_lenet_hvp
            *value = (int64_t)(p->family == PSVI_FAMILY_LENET ? lenet_tan_ws(*p, nullptr).bytes
                                                              : hvp_ws(*p, nullptr).bytes);
            break;
        case PSVI_Q_EVAL_WS_BYTES: *value = (int64_t)eval_ws(*p, nullptr).bytes; break;
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

}  // extern "C"
