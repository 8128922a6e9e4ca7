// capi_common.hpp -- what the units of the extern "C" boundary share
// (capi_plan.cpp, capi_inner.cpp, capi_outer.cpp, capi_tools.cpp): the error
// convention, the entry points' plan and argument checks, and the launch
// requests several of them fill the same way.
#pragma once
#include <string>

#include "psvi_diag.h"
#include "psvi_internal.hpp"
#include "workspace.hpp"

namespace psvi {

extern thread_local std::string g_err;  // psvi_last_error (capi_plan.cpp)

inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

inline int hip_fail(hipError_t e, const char* where) {
    g_err = std::string(where) + ": " + hipGetErrorString(e);
    return (int)e;
}

#define HIP_TRY(expr)                                      \
    do {                                                   \
        hipError_t e_ = (expr);                            \
        if (e_ != hipSuccess) return hip_fail(e_, #expr);  \
    } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Diagnostics (PSVI_DBG_LOOP_TIMING, capi_plan.cpp): HIP events around the
// network and the update launches of every `g_loop_every`-th full-cov
// inner-loop step.
extern int g_loop_every;
// records the next start or end event of phase k (0 net, 1 update) on the stream
hipError_t loop_event(int k, hipStream_t st);

// Every entry point that runs on a plan, except the loop that takes it up,
// drops the resident state of a PSVI_LOOP_KEEP call: it may have written the
// workspace, the parameters or the Adam state the state stands for.
inline void drop_resident(const psvi_plan* p) {
    if (p) p->resident.valid = false;
}

// The entry points' plan check.  families: the allowed PSVI_FAMILY_* as a bit
// mask, with `what` the message for a plan outside it (the phase entry points
// report a null plan the same way); without them a null plan is the error.
constexpr unsigned kFullCov = 1u << PSVI_FAMILY_FULLCOV, kNotFullCov = ~kFullCov;
inline int check_plan(const psvi_plan* p, unsigned families = ~0u, const char* what = nullptr) {
    if (!p && !what) return fail(PSVI_EINVAL, "null plan");
    if (!p || !(families >> p->family & 1u)) return fail(PSVI_ESTATE, what);
    if (!p->on_device) return fail(PSVI_ESTATE, "plan was created without a HIP device");
    return 0;
}
constexpr char kNotMf[] = "not a mean-field plan", kNotFc[] = "not a full-cov plan";

// Bernoulli plans run the inner objective, psvi_sampled_kl_grad and
// psvi_row_loglik only.
inline int refuse_bernoulli(const psvi_plan* p, const char* what) {
    if (p && p->lik == PSVI_LIK_BERNOULLI) return fail(PSVI_EUNSUP, what);
    return 0;
}

// The Adam hyper-parameters of an entry point that steps (required; the
// gradient-only calls pass false and may leave hp null).
inline int check_adam(const psvi_adam_hp* hp, bool required = true) {
    if (!required) return 0;
    if (hp->step < 1) return fail(PSVI_EINVAL, "adam step must be >= 1");
    if (hp->kind < 0 || hp->kind > 2) return fail(PSVI_EINVAL, "unknown adam kind");
    return 0;
}

// The ABI's `const int32_t* z`: labels, or a Gaussian plan's fp32 targets in
// the same 4-byte slots.
inline Targets abi_targets(const psvi_plan* p, const int32_t* z) {
    return p->lik == PSVI_LIK_GAUSSIAN ? Targets::values(reinterpret_cast<const float*>(z))
                                       : Targets::labels(z);
}

// the network launch on the rows (u, z, w), its NLL added into nll_out
inline NetLaunch net_rows(const float* u, Targets z, const float* w, double* nll_out) {
    NetLaunch n;
    n.u = u; n.targets = z; n.w = w; n.nll_out = nll_out;
    return n;
}

// the full-cov update's Adam step on g_shard, its KL added into kl_out
inline MvnUpdate mvn_step(const float* eps, const float* g_shard, float* params, float* m,
                          float* v, const psvi_adam_hp* hp, double* kl_out, int include_kl) {
    MvnUpdate up;
    up.eps = eps; up.g_shard = g_shard; up.params = params; up.m = m; up.v = v; up.hp = hp;
    up.kl_out = kl_out; up.include_kl = include_kl ? 1 : 0;
    return up;
}

}  // namespace psvi
