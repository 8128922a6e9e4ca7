// capi_tools.cpp -- the entry points beside the inner and outer objectives:
// the coreset-selection baselines (selection scores, Laplace, MFVI fit,
// predictive scores, GIGA, coreset draws, k-means) and the element-wise tools
// (Adam, its adjoint, conjugate gradients, normals, the non-finite scan).
#include <cmath>
#include <vector>

#include "capi_common.hpp"

using namespace psvi;

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

int kmeans_range(int64_t N, int64_t D, int64_t K) {
    if (N < 1 || D < 1 || K < 1 || K > N)
        return fail(PSVI_EINVAL, "k-means takes N >= 1, D >= 1 and 1 <= K <= N");
    if (K > kKmMaxK || D > kKmMaxD || N > kKmMaxN)
        return fail(PSVI_EUNSUP, "k-means supports K <= 128, D <= 4096, N <= 2^24");
    return 0;
}

}  // namespace

extern "C" {

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

int psvi_predict_query(const psvi_plan* p, int32_t rows_per_draw, int64_t* out) {
    if (!p || !out) return fail(PSVI_EINVAL, "null pointer");
    if (p->family != PSVI_FAMILY_MEANFIELD || p->lik != PSVI_LIK_CATEGORICAL || p->world != 1)
        return fail(PSVI_ESTATE, "the predictive scores need a mean-field categorical plan of world 1");
    if (rows_per_draw < 1) return fail(PSVI_EINVAL, "rows_per_draw must be >= 1");
    PredictShape s;
    if (predict_shape(*p, rows_per_draw, s) != 0)
        return fail(PSVI_EUNSUP, "a layer of the network does not fit the predictive scores' LDS "
                                 "budget: one unit's weights and one row's activations exceed 160 KiB");
    out[0] = s.RG;
    out[1] = s.wcap;
    for (int l = 0; l < kMaxL; ++l) out[2 + l] = l < s.L ? s.ut[l] : 0;
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
