// capi_inner.cpp -- the inner objective's entry points: the fused step, the
// phases of a sharded step, the tiled state and the inner loop.
#include "capi_common.hpp"

using namespace psvi;

namespace {

int check_step(const psvi_plan* p, const void* u, const void* z, const void* w, const void* eps) {
    if (int rc = check_plan(p)) return rc;
    if (p->world != 1) return fail(PSVI_ESTATE, "fused step needs world == 1 (use phases)");
    if (!u || !z || !w || !eps) return fail(PSVI_EINVAL, "null input pointer");
    return 0;
}

int step_impl(const psvi_plan* p, const float* u, Targets z, const float* w, const float* eps,
              float* params, float* m, float* v, const psvi_adam_hp* hp, double* elbo_out,
              float* grad_out, int include_kl, const StepWs& W, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(elbo_out, 0, sizeof(double), st));
    NetLaunch n = net_rows(u, z, w, elbo_out);
    if (p->family != PSVI_FAMILY_FULLCOV) {
        MfUpdate up;
        up.params = params; up.m = m; up.v = v; up.hp = hp;
        up.kl_out = elbo_out; up.grad_out = grad_out; up.include_kl = include_kl;
        if (p->family == PSVI_FAMILY_LENET) {
            HIP_TRY(launch_lenet(*p, u, z.slots(), w, params, eps, W.acc, elbo_out, p->lenet_scratch.dev, st));
            up.acc = W.acc;
        } else {
            // per-(sample, chunk) gradient slots, summed in a fixed order by the update
            n.params = params; n.eps = eps; n.mf_slots = p->mf_slots.dev;
            HIP_TRY(launch_net(*p, n, st));
            up.slot_eps = eps;
        }
        HIP_TRY(launch_mf_update(*p, up, st));
    } else {
        HIP_TRY(launch_mvn_fwd(*p, eps, params, W.x, st));
        n.xrecv = W.x; n.gsend = W.g;
        HIP_TRY(launch_net(*p, n, st));
        MvnUpdate up = mvn_step(eps, W.g, params, m, v, hp, elbo_out, include_kl);
        up.grad_out = grad_out;
        HIP_TRY(launch_mvn_update(*p, up, st));
    }
    return 0;
}

// One psvi_inner_loop_ex call: its arguments, its workspace and the draw of
// one step's eps from the loop's stream.
struct LoopCall {
    const psvi_plan* p = nullptr;
    const float* u = nullptr;
    Targets z;
    const float* w = nullptr;
    // eps of step t: the caller's [T][EPS_COUNT] array, or nullptr: Philox
    // (seed, offset + t * es)
    const float* eps = nullptr;
    uint64_t seed = 0, offset = 0;
    int64_t es = 0;
    int T = 0;
    float *params = nullptr, *m = nullptr, *v = nullptr;
    const psvi_adam_hp* hp = nullptr;
    double* elbo_out = nullptr;  // [T]
    const void* ws = nullptr;
    int flags = 0;
    LoopWs L{};
    RandnLaunch rn;
    hipStream_t st = nullptr;
};

// eps of step 0 with the ELBO accumulators cleared: Philox mode folds the
// clear into the draw's launch
const float* first_eps(const LoopCall& c) {
    if (c.eps) {
        return hipMemsetAsync(c.elbo_out, 0, sizeof(double) * (size_t)c.T, c.st) == hipSuccess
                   ? c.eps
                   : nullptr;
    }
    RandnLaunch r = c.rn;
    r.out = c.L.ebuf[0]; r.offset = c.offset; r.zero = c.elbo_out; r.nzero = c.T;
    return launch_randn(r, c.st) == hipSuccess ? c.L.ebuf[0] : nullptr;
}

// two launches per step: the network kernel (which also draws the next
// step's eps in Philox mode) and the slot-reducing update; the ELBO
// accumulators are cleared once for the whole loop
int loop_meanfield(const LoopCall& c) {
    const psvi_plan* p = c.p;
    if (c.T == 0) return 0;
    psvi_adam_hp h = *c.hp;
    const float* e = first_eps(c);
    if (!e) return fail(PSVI_EUNSUP, "randn launch failed");
    for (int t = 0; t < c.T; ++t) {
        h.step = c.hp->step + t;
        const bool draw = !c.eps && t + 1 < c.T;
        float* en_buf = draw ? c.L.ebuf[(t + 1) & 1] : nullptr;
        NetLaunch n = net_rows(c.u, c.z, c.w, c.elbo_out + t);
        n.params = c.params; n.eps = e; n.mf_slots = p->mf_slots.dev;
        n.draw.out = en_buf; n.draw.n = draw ? p->Peps : 0;
        n.draw.seed = c.seed; n.draw.offset = c.offset + (uint64_t)(t + 1) * c.es;
        HIP_TRY(launch_net(*p, n, c.st));
        MfUpdate up;
        up.slot_eps = e; up.params = c.params; up.m = c.m; up.v = c.v; up.hp = &h;
        up.kl_out = c.elbo_out + t; up.include_kl = 1;
        HIP_TRY(launch_mf_update(*p, up, c.st));
        e = t + 1 < c.T ? (c.eps ? c.eps + (size_t)(t + 1) * p->Peps : en_buf) : nullptr;
    }
    return 0;
}

// LeNet: T fused steps, each on its own draw
int loop_generic(const LoopCall& c) {
    const psvi_plan* p = c.p;
    psvi_adam_hp h = *c.hp;
    for (int t = 0; t < c.T; ++t) {
        const float* e = c.eps ? c.eps + (size_t)t * p->Peps : nullptr;
        if (!e) {
            RandnLaunch r = c.rn;
            r.out = c.L.ebuf[t & 1]; r.offset = c.offset + (uint64_t)t * c.es;
            if (launch_randn(r, c.st) != hipSuccess) return fail(PSVI_EUNSUP, "randn launch failed");
            e = r.out;
        }
        h.step = c.hp->step + t;
        if (int rc = step_impl(p, c.u, c.z, c.w, e, c.params, c.m, c.v, &h, c.elbo_out + t,
                               nullptr, 1, c.L.step, c.st))
            return rc;
    }
    return 0;
}

// full-cov: sample x_0, then per step net + update, the update also sampling
// the next step's x from the updated parameters (fused where the plan allows)
int loop_fullcov(const LoopCall& c) {
    const psvi_plan* p = c.p;
    const float* eps = c.eps;
    const int T = c.T;
    hipStream_t st = c.st;
    float* const* ebuf = c.L.ebuf;
    float *x = c.L.step.x, *g = c.L.step.g;
    // corr / m / v live in the tiled layout for the whole loop when the plan allows
    float* ts = c.L.tstate;
    // Philox mode: eps, eps' and G are the loop's own buffers -- their 64-float
    // pads are zeroed with the tiled conversion and the streaming update reads
    // them unclamped
    const bool padded = ts && !eps;
    // Philox mode on a bf-stream plan: every draw also as bf16 planes, one
    // plane buffer per eps buffer (their row pads zeroed here, never drawn)
    uint16_t* pbuf[2] = {padded ? c.L.pbuf[0] : nullptr, padded ? c.L.pbuf[1] : nullptr};
    float* pads[3] = {padded ? c.L.pads[0] : nullptr, padded ? c.L.pads[1] : nullptr,
                      padded ? c.L.pads[2] : nullptr};
    if (T == 0) return 0;
    psvi_adam_hp h = *c.hp;
    // resident state of the last KEEP call (dropped by every call; taken up by
    // a RESUME call that continues it)
    const psvi_plan::Resident res = p->resident;
    p->resident.valid = false;
    const bool keep = (c.flags & PSVI_LOOP_KEEP) && padded;
    const bool resume = (c.flags & PSVI_LOOP_RESUME) && padded && res.valid && res.ws == c.ws &&
                        res.params == c.params && res.m == c.m && res.v == c.v &&
                        res.seed == c.seed && res.offset == c.offset;
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
        clear.out = ebuf[1 - bi(0)]; clear.zero = c.elbo_out; clear.nzero = T;
        HIP_TRY(launch_randn(clear, st));
        e = ebuf[bi(0)];
    } else {
        // packed -> tiled state on the plan's conversion stream, behind x_0 and the
        // first network step (joined before the first update)
        if (ts && p->aux.st) {
            HIP_TRY(hipEventRecord(p->aux.fork, st));
            HIP_TRY(hipStreamWaitEvent(p->aux.st, p->aux.fork, 0));
            HIP_TRY(launch_mvn_tile_convert(*p, c.params, c.m, c.v, ts, true, p->aux.st, pads));
            HIP_TRY(hipEventRecord(p->aux.join, p->aux.st));
            join = true;
        } else if (ts) {
            HIP_TRY(launch_mvn_tile_convert(*p, c.params, c.m, c.v, ts, true, st, pads));
        }
        if (pbuf[0]) {
            HIP_TRY(hipMemsetAsync(pbuf[0], 0, 2 * c.L.pbuf_bytes, st));
            RandnLaunch r = c.rn;
            r.out = ebuf[0]; r.offset = c.offset; r.zero = c.elbo_out; r.nzero = T;
            r.planes_desc = &p->eps_planes; r.planes = pbuf[0];
            HIP_TRY(launch_randn(r, st));
            e = ebuf[0];
        } else {
            e = first_eps(c);
        }
        if (!e) return fail(PSVI_EUNSUP, "randn launch failed");
        HIP_TRY(launch_mvn_fwd(*p, e, c.params, x, st));
    }
    for (int t = 0; t < T; ++t) {
        h.step = c.hp->step + t;
        // Philox mode: the network kernel also draws the next step's eps (KEEP:
        // the last step too, for the next call)
        const bool last = t + 1 == T;
        const bool draw = !eps && (!last || keep);
        float* en_buf = draw ? ebuf[bi(t + 1)] : nullptr;
        uint16_t* en_pl = draw ? pbuf[bi(t + 1)] : nullptr;
        const bool tm = g_loop_every > 0 && t % g_loop_every == 0;
        if (tm) HIP_TRY(loop_event(0, st));
        NetLaunch n = net_rows(c.u, c.z, c.w, c.elbo_out + t);
        n.xrecv = x; n.gsend = g;
        n.draw.out = en_buf; n.draw.n = draw ? p->Peps : 0; n.draw.planes = en_pl;
        n.draw.seed = c.seed; n.draw.offset = c.offset + (uint64_t)(t + 1) * c.es;
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
        MvnUpdate up = mvn_step(e, g, c.params, c.m, c.v, &h, c.elbo_out + t, 1);
        up.tstate = ts; up.packed_out = ts && !en; up.padded = padded; up.eps_planes = pbuf[bi(t)];
        if (en) {
            up.next.eps = en; up.next.x = x; up.next.planes = en_pl;
        }
        HIP_TRY(launch_mvn_update(*p, up, st));
        if (tm) HIP_TRY(loop_event(1, st));
        e = en;
    }
    if (keep) {
        HIP_TRY(launch_mvn_tile_convert(*p, c.params, c.m, c.v, ts, false, st, nullptr));
        p->resident = psvi_plan::Resident{true, c.ws, c.params, c.m, c.v, c.seed,
                                          c.offset + (uint64_t)T * c.es, bi(T)};
    }
    return 0;
}

}  // namespace

extern "C" {

int psvi_inner_step(const psvi_plan* p, const float* u, const int32_t* z, const float* w,
                    const float* eps, float* params, float* adam_m, float* adam_v,
                    const psvi_adam_hp* hp, double* elbo_out, void* ws, size_t ws_bytes,
                    void* stream) {
    drop_resident(p);
    if (int rc = check_step(p, u, z, w, eps)) return rc;
    const StepWs W = step_ws(*p, ws);
    if (!ws || ws_bytes < W.bytes) return fail(PSVI_ENOSPC, "workspace too small");
    if (!params || !adam_m || !adam_v || !hp || !elbo_out)
        return fail(PSVI_EINVAL, "null state pointer");
    if (int rc = check_adam(hp)) return rc;
    return step_impl(p, u, abi_targets(p, z), w, eps, params, adam_m, adam_v, hp, elbo_out,
                     nullptr, 1, W, as_stream(stream));
}

int psvi_elbo_grad(const psvi_plan* p, const float* u, const int32_t* z, const float* w,
                   const float* eps, const float* params, int32_t include_kl, double* elbo_out,
                   float* grad_out, void* ws, size_t ws_bytes, void* stream) {
    drop_resident(p);
    if (int rc = check_step(p, u, z, w, eps)) return rc;
    const StepWs W = step_ws(*p, ws);
    if (!ws || ws_bytes < W.bytes) return fail(PSVI_ENOSPC, "workspace too small");
    if (!params || !elbo_out || !grad_out) return fail(PSVI_EINVAL, "null pointer");
    return step_impl(p, u, abi_targets(p, z), w, eps, const_cast<float*>(params), nullptr,
                     nullptr, nullptr, elbo_out, grad_out, include_kl ? 1 : 0, W,
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

int psvi_mvn_tiled_convert(const psvi_plan* p, float* params, float* adam_m, float* adam_v,
                           float* tstate, int32_t to_tiled, void* stream) {
    drop_resident(p);
    if (!p || !tiled_ok(*p)) return fail(PSVI_EUNSUP, "plan has no tiled state (full-cov, world 1, S <= 128)");
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
    if (!p || !tiled_ok(*p)) return fail(PSVI_EUNSUP, "plan has no tiled state (full-cov, world 1, S <= 128)");
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
    LoopCall c;
    c.L = loop_ws(*p, ws);
    if (!ws || ws_bytes < c.L.bytes) return fail(PSVI_ENOSPC, "workspace too small");
    c.p = p; c.u = u; c.z = abi_targets(p, z); c.w = w; c.eps = eps;
    c.seed = seed; c.offset = offset; c.es = eps_stride(*p); c.T = T;
    c.params = params; c.m = adam_m; c.v = adam_v; c.hp = hp; c.elbo_out = elbo_out;
    c.ws = ws; c.flags = flags; c.st = as_stream(stream);
    c.rn.n = p->Peps; c.rn.seed = seed;
    if (p->family == PSVI_FAMILY_MEANFIELD) return loop_meanfield(c);
    if (p->family != PSVI_FAMILY_FULLCOV) return loop_generic(c);
    return loop_fullcov(c);
}

}  // extern "C"
