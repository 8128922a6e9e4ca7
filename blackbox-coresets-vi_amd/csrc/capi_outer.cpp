// capi_outer.cpp -- the outer objective's entry points: its loss and
// gradients, the predictive evaluation, the Bernoulli plans' row
// log-likelihoods and sampled KL, and the Hessian-vector product.
#include "capi_common.hpp"

using namespace psvi;

namespace {

// ext_coef == nullptr: the whole objective (stats, forward, combine, backward).
// Otherwise [rowcoef (S x 2) | ck (S) | sck (1)] replace the combine: the
// backward of a caller-formed softmax over samples (sample-sharded outer).
int outer_impl(const psvi_plan* p, int32_t n_pseudo, const float* x_all,
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
    const OuterWs o = outer_ws(*p, ws);
    if (!ws || ws_bytes < o.bytes) return fail(PSVI_ENOSPC, "workspace too small");
    hipStream_t st = as_stream(stream);
    float *x = o.step.x, *g = o.step.g, *acc = o.step.acc;
    if (p->family == PSVI_FAMILY_FULLCOV) HIP_TRY(launch_mvn_fwd(*p, eps, params, x, st));
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

}  // namespace

extern "C" {

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
    const EvalWs E = eval_ws(*p, ws);
    if (!ws || ws_bytes < E.bytes) return fail(PSVI_ENOSPC, "workspace too small");
    hipStream_t st = as_stream(stream);
    const OuterWs& o = E.outer;
    float* x = o.step.x;  // full-cov only
    if (p->family == PSVI_FAMILY_FULLCOV) HIP_TRY(launch_mvn_fwd(*p, eps, params, x, st));
    HIP_TRY(launch_outer_stats(*p, params, eps, x, o.stats, st));
    NetOuter fw{1, n_pseudo, o.nll, nullptr, nullptr, nullptr, E.out};
    NetLaunch n = net_rows(x_all, Targets::labels(z_all), w_all, nullptr);
    n.params = params; n.eps = eps; n.xrecv = x; n.outer = &fw;
    if (p->family == PSVI_FAMILY_LENET)
        HIP_TRY(launch_lenet(*p, x_all, z_all, w_all, params, eps, nullptr, nullptr,
                             p->lenet_scratch.dev, st, &fw));
    else
        HIP_TRY(launch_net(*p, n, st));
    HIP_TRY(launch_eval(*p, n_pseudo, params, w_all, z_all, o.nll, o.stats, E.out,
                        correction ? 1 : 0, E.W, probs_out, stats_out, st));
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
    const EvalWs E = eval_ws(*p, ws);
    if (!ws || ws_bytes < E.bytes) return fail(PSVI_ENOSPC, "workspace too small");
    hipStream_t st = as_stream(stream);
    const OuterWs& o = E.outer;
    float* f = E.out;  // the data rows' outputs [S][M - n_pseudo]
    HIP_TRY(launch_outer_stats(*p, params, eps, nullptr, o.stats, st));
    NetOuter fw{1, n_pseudo, o.nll, nullptr, nullptr, nullptr, f};
    NetLaunch n = net_rows(x_all, Targets::values(y_all), w_all, nullptr);
    n.params = params; n.eps = eps; n.outer = &fw;
    HIP_TRY(launch_net(*p, n, st));
    HIP_TRY(launch_eval_regression(*p, n_pseudo, params, y_all + n_pseudo, o.stats, f,
                                   correction ? 1 : 0, y_mean, y_std, E.W, pred_out, stats_out, st));
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
    if (p->rop.valu.rc == 0)
        return fail(PSVI_EUNSUP, "model too wide for the per-sample R-op kernel's LDS");
    const HvpWs o = hvp_ws(*p, ws);
    if (!ws || ws_bytes < o.bytes) return fail(PSVI_ENOSPC, "workspace too small");
    hipStream_t st = as_stream(stream);
    float* x = o.step.x;  // full-cov only
    if (p->family == PSVI_FAMILY_FULLCOV) {
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

}  // extern "C"
