/*
 * psvi_hip.h -- C ABI of the MI355X (gfx950) coreset-ELBO inner-loop library
 * (libpsvi_hip.so).  Plain C: no HIP, torch or C++ types, so ctypes / cgo /
 * JNI / N-API can bind it directly (binding stubs: INTEGRATION.md).
 *
 * What it replaces (reference = souravc83/Blackbox-Coresets-VI, paths relative
 * to its repo root):
 *   one inner step of PSVI.nested_step / PSVI.hyper_step, i.e.
 *     PSVI.inner_elbo                     psvi/inference/psvi_classes.py:488-511
 *       -> VILinear.forward / rsample      psvi/models/neural_net.py:155-179
 *       -> VILinearMultivariateNormal      neural_net.py:408-491
 *       -> Categorical.log_prob, .matmul(N f(v)), sum, + sum(m.kl())
 *     DifferentiableOptimizer.step         psvi/robust_higher/optim.py:152-257
 *       -> DifferentiableAdam._update      optim.py:299-367      (trainer nested)
 *     hypergrad DifferentiableAdam.step    psvi/hypergrad/diff_optimizers.py:107-154
 *       -> adam_step                       diff_optimizers.py:184-213 (trainer hyper)
 *
 * Conventions
 *   - Every pointer argument is a DEVICE pointer (fp32 unless stated) owned by
 *     the caller; the library never allocates device memory inside a step
 *     (psvi_plan_create allocates its immutable work lists and the plan-owned
 *     split-K scratch of the full-cov sample phase and the LeNet activation
 *     scratch; a plan's calls must not
 *     run concurrently on different streams).
 *   - Steps are stream-ordered and asynchronous on `stream` (a hipStream_t
 *     passed as void*; NULL = default stream); no host synchronisation inside.
 *   - Return 0 on success, <0 for an invalid argument / shape (PSVI_E*),
 *     >0 for a hipError_t.  psvi_last_error() gives a thread-local message.
 *   - Parameter vectors use the reference's parameters_to_vector order:
 *       mean-field layer (in,out): [mu_W (out*in), mu_b (out), rho_W (out*in), rho_b (out)]
 *       full-cov   layer (in,out): n = out*in + out;
 *                                  [mean (n), sd (n), corr ((n-1)(n-2)/2)]
 *     corr is the packed row-major strict lower triangle of the top-left
 *     (n-1)x(n-1) block of L (neural_net.py:452-461): row r starts at r(r-1)/2.
 *   - Noise `eps` uses the reference draw order (Normal/MultivariateNormal
 *     rsample in forward order): mean-field per layer eps_W (S,out,in) then
 *     eps_b (S,out); full-cov per layer eps (S, n).  S is the GLOBAL sample
 *     count of the plan; every rank passes the full eps.
 *   - z holds int32 class ids; w holds the coreset weights N*f(v) (M floats,
 *     psvi_classes.py:505).
 *   - On a plan created with a Gaussian likelihood (psvi_plan_create_lik,
 *     PSVI_LIK_GAUSSIAN) every z / z_all argument of every entry point points
 *     to fp32 regression targets instead: the caller casts its const float*
 *     to the declared const int32_t*; the kernels read the same 32 bits as
 *     floats.
 *   - Scalar objective outputs (elbo_out, nll_out, kl_out) are DOUBLE device
 *     accumulators: the kernels add thousands of per-block partials into them
 *     and fp32 accumulation would bias the sum (rounding of similar-size adds
 *     into a large running total).  They are accumulated into (+=) unless a
 *     call documents that it zeroes them.
 */
#ifndef PSVI_HIP_H
#define PSVI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSVI_MAX_LAYERS 8

/* error codes (<0) */
#define PSVI_EINVAL   (-1)   /* bad descriptor / shape / pointer            */
#define PSVI_ENOSPC   (-2)   /* workspace too small                         */
#define PSVI_EUNSUP   (-3)   /* configuration not supported by the kernels  */
#define PSVI_ESTATE   (-4)   /* call not valid for this plan (family/world) */

/* model families */
#define PSVI_FAMILY_MEANFIELD 0   /* VILinear stack: logistic_regression, fn   */
#define PSVI_FAMILY_FULLCOV   1   /* VILinearMultivariateNormal stack: fn2,
                                     logistic_regression_fullcov              */
#define PSVI_FAMILY_LENET     2   /* make_lenet (neural_net.py:334-359): VIConv2d(1,6,5,p2)
                                     ReLU BatchMaxPool2d(2) VIConv2d(6,16,5) ReLU pool
                                     VILinear 400-120-84-10 (the last one ONE shared
                                     sample, mc_samples=1); u is (M,1,28,28).  The
                                     architecture is fixed: n_layers / dims of the
                                     descriptor are ignored.  Parameters: the
                                     mean-field layout per layer (conv weights in
                                     (out,in,5,5) order); eps per layer in draw order,
                                     W (S,n_w) then b (S,n_b), the last layer (n_w)
                                     then (n_b) without S.  KL on the VILinear layers
                                     only (psvi_classes.py:506-510).  Entry points:
                                     inner_step, elbo_grad, inner_loop and the
                                     mean-field phases; the plan owns the activation
                                     scratch (about S*M*7.9 KB).                  */

/* Adam variants */
#define PSVI_ADAM_HIGHER    0   /* robust_higher DifferentiableAdam (optim.py:318-367):
                                   denom = sqrt(v + 1e-8)/sqrt(bc2) + eps            */
#define PSVI_ADAM_HYPERGRAD 1   /* hypergrad adam_step (diff_optimizers.py:197-213):
                                   v += 1e-12 stored; denom = sqrt(v/bc2) + eps      */
#define PSVI_ADAM_TORCH     2   /* torch.optim.Adam (the MFVI baselines' optim_vi,
                                   baselines.py:870, 1020): denom = sqrt(v)/sqrt(bc2) + eps;
                                   not differentiable here (psvi_adam_adjoint refuses) */

typedef struct psvi_net_desc {
    int32_t n_layers;                     /* affine VI layers                     */
    int32_t dims[PSVI_MAX_LAYERS + 1];    /* dims[0] = D ... dims[n_layers] = C   */
    int32_t S;                            /* GLOBAL Monte-Carlo samples           */
    int32_t M;                            /* pseudopoints                         */
    float   prior_sd;                     /* sigma_0 (neural_net.py:61, 409)      */
} psvi_net_desc;

typedef struct psvi_adam_hp {
    float   lr;
    float   beta1;
    float   beta2;
    float   eps;
    int32_t step;      /* 1-based Adam step t (bias corrections 1 - beta^t) */
    int32_t kind;      /* PSVI_ADAM_HIGHER | PSVI_ADAM_HYPERGRAD            */
} psvi_adam_hp;

typedef struct psvi_plan psvi_plan;       /* opaque, immutable after create */

/* psvi_plan_query keys */
#define PSVI_Q_PARAM_COUNT   1  /* floats in params / adam_m / adam_v / grad          */
#define PSVI_Q_EPS_COUNT     2  /* floats of eps for all S (reference draw order)     */
#define PSVI_Q_WS_BYTES      3  /* workspace bytes for psvi_inner_step/elbo_grad      */
#define PSVI_Q_S_LOCAL       4  /* samples owned by this rank                         */
#define PSVI_Q_S_OFFSET      5  /* first global sample owned by this rank             */
#define PSVI_Q_ACC_COUNT     6  /* mean-field: floats in the all-reduced accumulator
                                   [sum_s dW | sum_s dW*eps] = 2 * sum_l n_l         */
#define PSVI_Q_ROWS_LOCAL    7  /* full-cov: x/g columns owned (sum over layers)      */
#define PSVI_Q_XSHARD_COUNT  8  /* full-cov: floats of x_shard / g_shard = S*ROWS_LOCAL */
#define PSVI_Q_XRECV_COUNT   9  /* full-cov: floats of x_recv / g_send = S_LOCAL*n_tot */
#define PSVI_Q_LOOP_WS_BYTES 10 /* workspace bytes for psvi_inner_loop                 */
#define PSVI_Q_TILED_FLOATS  11 /* floats of the tiled corr/m/v state (0: the plan has
                                   none -- it needs full-cov, world 1, S <= 128)      */
#define PSVI_Q_OUTER_WS_BYTES 12 /* workspace bytes for psvi_outer_elbo_grad          */
#define PSVI_Q_HVP_WS_BYTES  13 /* workspace bytes for psvi_hvp                       */
#define PSVI_Q_EVAL_WS_BYTES 14 /* workspace bytes for psvi_evaluate                  */
#define PSVI_Q_NET_PART_OK   15 /* full-cov: 1 if psvi_mvn_phase_net_part takes sample
                                   ranges (no per-chunk gradient slots), else 0    */
#define PSVI_Q_NET_MCHUNKS   16 /* pseudopoint chunks the network kernels split this
                                   plan's M rows into (1: one workgroup sees all)  */

/* Create a plan for `family` over `world` ranks, this process being `rank`.
 * Samples are split in contiguous blocks; for FULLCOV at world > 1 the rows
 * of the layers' L are split in whole 64-row bands, balanced by their 64 x 64
 * tile counts over all layers (ranks own the matching mean/sd/corr rows and
 * their Adam state; a rank's rows need not be contiguous -- see
 * psvi_plan_shard_runs). */
int psvi_plan_create(int32_t family, const psvi_net_desc* d, int32_t world,
                     int32_t rank, psvi_plan** out);

/* Observation models.  PSVI_LIK_CATEGORICAL: Categorical(logits), the class
 * ids in z (every plan of psvi_plan_create).  PSVI_LIK_GAUSSIAN: Normal(f,
 * 1 / sqrt(tau)) over ONE network output f with fixed precision tau -- the
 * reference's regressors (PSVI_regressor, psvi_classes.py:1940-2335, distr_fn
 * = gaussian_fn(scale = 1 / sqrt(tau)), make_regressor_net neural_net.py:300-331).
 * For a row with output f, target z and weight w:
 *   NLL = tau / 2 (f - z)^2 + log(2 pi / tau) / 2,  d NLL / d f = tau (f - z),
 *   d NLL / d z = -d NLL / d f.
 *
 * PSVI_LIK_BERNOULLI: Bernoulli(logits = f) over ONE network output f -- the
 * observation model of the sparse black-box VI coreset construction
 * (run_sparsevi_with_bb_elbo, psvi/inference/sparsebbvi.py; elbo /
 * forward_through_coreset / sparsevi_psvi_elbo / predict_through_coreset,
 * psvi/inference/utils.py:85-141).  z stays int32 class ids, in {0, 1} (the
 * caller checks the range); tau is ignored.  For output f, label z:
 *   NLL = softplus(f) - z f = max(f, 0) - z f + log1p(exp(-|f|)),
 *   d NLL / d f = sigmoid(f) - z. */
#define PSVI_LIK_CATEGORICAL 0
#define PSVI_LIK_GAUSSIAN    1
#define PSVI_LIK_BERNOULLI   2
typedef struct psvi_likelihood {
    int32_t kind;      /* PSVI_LIK_*                                      */
    float   tau;       /* PSVI_LIK_GAUSSIAN: the precision, > 0           */
} psvi_likelihood;

/* psvi_plan_create with an observation model.  lik == NULL or a categorical
 * lik: exactly psvi_plan_create.  A Gaussian lik needs family ==
 * PSVI_FAMILY_MEANFIELD and world == 1 (PSVI_EUNSUP otherwise), dims[n_layers]
 * == 1 and a finite tau > 0 (PSVI_EINVAL otherwise).  On such a plan
 * psvi_inner_step, psvi_elbo_grad, psvi_inner_loop(_ex), the mean-field
 * phases, psvi_outer_elbo_grad(_coef)(_ex), psvi_hvp(_partial / _ex) and
 * psvi_evaluate_regression run with fp32 targets (see Conventions);
 * psvi_evaluate returns PSVI_ESTATE and psvi_outer_ablated_elbo_grad
 * PSVI_EUNSUP (the reference has no ablated regressor).
 * A Bernoulli lik has the same limits (mean-field, world == 1: PSVI_EUNSUP
 * otherwise; dims[n_layers] == 1: PSVI_EINVAL otherwise).  On such a plan
 * psvi_inner_step, psvi_elbo_grad, psvi_inner_loop(_ex), the mean-field phases
 * (with include_kl = 1: the analytic KL, as on every plan), psvi_sampled_kl_grad
 * and psvi_row_loglik run; the outer-objective, evaluate, HVP and R-op entry
 * points return PSVI_EUNSUP. */
int psvi_plan_create_lik(int32_t family, const psvi_net_desc* d, int32_t world,
                         int32_t rank, const psvi_likelihood* lik, psvi_plan** out);
int psvi_plan_destroy(psvi_plan* plan);
int psvi_plan_query(const psvi_plan* plan, int32_t key, int64_t* value);
/* rows (full-cov) and samples owned by rank `r` of the plan's world:
 * out[0] = s_offset, out[1] = s_count, out[2] = rows_total,
 * out[3 + l] = first row of layer l when the rank's rows of layer l are one
 * contiguous run (-1 when they are several), out[3 + PSVI_MAX_LAYERS + l] =
 * row count of layer l. */
int psvi_plan_shard_info(const psvi_plan* plan, int32_t r, int64_t* out);
/* The rows of rank `r` as runs, in x-shard column order (layer-major, rows
 * ascending): out[4 i .. 4 i + 3] = (layer, first row, row count, x-shard
 * column of the first row) for i < *count.  out == NULL: *count only;
 * PSVI_ENOSPC when cap < *count.  x_shard / g_shard hold [S][ROWS_LOCAL] in
 * this column order; x_recv / g_send hold, per source rank q in rank order,
 * [S_LOCAL][rows_total of q] in q's column order. */
int psvi_plan_shard_runs(const psvi_plan* plan, int32_t r, int64_t* out, int32_t cap,
                         int32_t* count);

/* ---- single-process fused step (world == 1) --------------------------------
 * One inner step = reparameterise, batched forward over (S x M), weighted NLL
 * + KL, hand-derived backward, Adam update of params/adam_m/adam_v in place.
 * elbo_out[0] (double, zeroed by the call) <- negative inner ELBO (the value
 * inner_elbo returns) at the incoming params.  eps == NULL is invalid (draw
 * it with psvi_randn, or pass the reference-order draws). */
int psvi_inner_step(const psvi_plan* plan, const float* u, const int32_t* z,
                    const float* w, const float* eps, float* params,
                    float* adam_m, float* adam_v, const psvi_adam_hp* hp,
                    double* elbo_out, void* ws, size_t ws_bytes, void* stream);

/* Same objective without the update: grad_out (PARAM_COUNT floats) <- d elbo
 * / d params, elbo_out[0] (double, zeroed by the call) <- elbo.  Used by the
 * autograd.Function boundary.  include_kl = 0 drops the KL term and its
 * gradient. */
int psvi_elbo_grad(const psvi_plan* plan, const float* u, const int32_t* z,
                   const float* w, const float* eps, const float* params,
                   int32_t include_kl, double* elbo_out, float* grad_out,
                   void* ws, size_t ws_bytes, void* stream);

/* T chained inner steps (world == 1): the loop the reference runs as
 *   for t in range(T): diffopt.step(inner_elbo(fmodel))   (psvi_classes.py:549-555)
 * with Adam steps hp->step .. hp->step + T - 1 on params/adam_m/adam_v in place.
 * elbo_out[t] (T doubles) <- negative inner ELBO before step t.  eps: the T
 * steps' noise as [T][EPS_COUNT] floats, or NULL to draw step t's noise in the
 * library with psvi_randn(seed, offset + t * round_up(EPS_COUNT, 4)).  For
 * full-cov plans each update also samples the next step's weights from the
 * updated parameters (one fused kernel when S <= 128; the separate sample
 * phase otherwise): the same numbers as T psvi_inner_step calls up to fp32
 * summation order.  ws: PSVI_Q_LOOP_WS_BYTES. */
int psvi_inner_loop(const psvi_plan* plan, const float* u, const int32_t* z,
                    const float* w, const float* eps, uint64_t seed, uint64_t offset,
                    int32_t T, float* params, float* adam_m, float* adam_v,
                    const psvi_adam_hp* hp, double* elbo_out, void* ws, size_t ws_bytes,
                    void* stream);

/* psvi_inner_loop with the loop's state kept across calls (full-cov plans with a
 * tiled state, Philox mode).  The calls of a run of inner steps split over
 * several calls repeat the first steps' fixed work -- corr / m / v into the
 * tiled layout, step 0's draw and sample -- because one call cannot know that
 * the next continues it:
 *   PSVI_LOOP_KEEP   the last step also draws (seed, offset + T * stride) and
 *                    samples the next step's weights (the fused update, as
 *                    every other step), the tiled corr / m / v stay in ws, and
 *                    the packed params / adam_m / adam_v are written as usual;
 *   PSVI_LOOP_RESUME start from that resident state when this call continues
 *                    the last KEEP call on this plan: the same ws, params,
 *                    adam_m, adam_v pointers and seed, and offset = its offset
 *                    + T * stride.  The caller asserts that nothing wrote
 *                    params / adam_m / adam_v / ws since (the Python
 *                    InnerLoopPlan checks the tensors' version counters);
 *                    otherwise -- or when the state does not match -- the call
 *                    starts cold, as psvi_inner_loop.
 * Every call drops the resident state first, so a RESUME after any other loop
 * call on the plan starts cold.  RESUME without KEEP takes the state up and
 * ends as a plain call.  Calls of T1, T2, ... steps, each resuming the last
 * and all but the last with KEEP, give the numbers of one call of T1 + T2 +
 * ... steps bit for bit (a KEEP call's last step is the fused update with the
 * next sample, as every step but the last of a call; a plain call's last step
 * writes the packed arrays directly: the same values up to fp32 rounding).
 * Other plans and eps != NULL: the flags are ignored. */
#define PSVI_LOOP_KEEP   1
#define PSVI_LOOP_RESUME 2
int psvi_inner_loop_ex(const psvi_plan* plan, const float* u, const int32_t* z,
                       const float* w, const float* eps, uint64_t seed, uint64_t offset,
                       int32_t T, float* params, float* adam_m, float* adam_v,
                       const psvi_adam_hp* hp, double* elbo_out, void* ws, size_t ws_bytes,
                       int32_t flags, void* stream);

/* ---- sharded phases (any world; the caller runs the collectives) ------------
 * MEANFIELD (sample-parallel, replicated params):
 *   acc (ACC_COUNT floats, overwritten) <- [sum_s dW | sum_s dW*eps] over this
 *   rank's samples, summed in a fixed order from per-(sample, chunk) slots
 *   (plan-owned scratch: one call on a plan at a time; bitwise reproducible),
 *   nll_out[0] += their weighted NLL;  caller
 *   all-reduces acc (sum);  update applies KL gradient + Adam identically on
 *   every rank (grad_out != NULL: write the gradient instead), kl_out[0] +=
 *   KL (nullable; count it on one rank). */
int psvi_mf_phase_accumulate(const psvi_plan* plan, const float* u,
                             const int32_t* z, const float* w, const float* eps,
                             const float* params, float* acc, double* nll_out,
                             void* stream);
int psvi_mf_phase_update(const psvi_plan* plan, const float* acc, float* params,
                         float* adam_m, float* adam_v, const psvi_adam_hp* hp,
                         double* kl_out, float* grad_out, int32_t include_kl,
                         void* stream);

/* FULLCOV (rows of L sharded, samples sharded):
 *   sample: x_shard[S][ROWS_LOCAL] <- mean + L eps for this rank's rows, all S
 *   (all_to_all: rank r sends rows s in shard q to q -> x_recv)
 *   net:    x_recv[S_LOCAL][n_tot, blocked by source rank] -> g_send (same
 *           layout) = per-sample gradients; nll_out[0] += local weighted NLL
 *   (all_to_all back -> g_shard[S][ROWS_LOCAL])
 *   update: corr/mean/sd Adam for owned rows; kl_out[0] += owned KL part.
 *           grad_out != NULL writes the gradient instead of updating. */
int psvi_mvn_phase_sample(const psvi_plan* plan, const float* eps,
                          const float* params, float* x_shard, void* stream);
int psvi_mvn_phase_net(const psvi_plan* plan, const float* u, const int32_t* z,
                       const float* w, const float* x_recv, float* g_send,
                       double* nll_out, void* stream);
/* the net phase with the next step's noise drawn in the same launch (the
 * sharded inner loop: every rank draws the whole global eps of the next step,
 * normals [0, n) of the psvi_randn stream (seed, offset) into eps_out -- the
 * same values psvi_randn writes -- split over the network kernel's workgroups
 * after their gradients; no separate draw launch).  offset % 4 == 0. */
int psvi_mvn_phase_net_draw(const psvi_plan* plan, const float* u, const int32_t* z,
                            const float* w, const float* x_recv, float* g_send,
                            double* nll_out, float* eps_out, int64_t n, uint64_t seed,
                            uint64_t offset, void* stream);
/* the net phase (with, optionally, one part of the next step's draw) for the
 * rank's local samples [s_begin, s_begin + s_count) only -- the sharded loop's
 * sample halves, whose exchanges overlap the other half's network.  The
 * buffers are the whole rank's (x_recv / g_send [source rank][S_LOCAL][rows]);
 * this launch reads and writes its samples' rows.  Draw: normals of quad range
 * part of nparts (contiguous, in order) of [0, n) into eps_out (NULL, n = 0:
 * none).  Plans whose pseudopoint chunks use per-chunk slots (not looped)
 * take whole launches only (PSVI_EUNSUP). */
int psvi_mvn_phase_net_part(const psvi_plan* plan, const float* u, const int32_t* z,
                            const float* w, const float* x_recv, float* g_send,
                            double* nll_out, int32_t s_begin, int32_t s_count, float* eps_out,
                            int64_t n, uint64_t seed, uint64_t offset, int32_t part,
                            int32_t nparts, void* stream);
int psvi_mvn_phase_update(const psvi_plan* plan, const float* eps,
                          const float* g_shard, float* params, float* adam_m,
                          float* adam_v, const psvi_adam_hp* hp, double* kl_out,
                          float* grad_out, int32_t include_kl, void* stream);
/* update (Adam) followed by the next step's sample phase from the updated
 * parameters: x_next[S][ROWS_LOCAL] <- mean' + L' eps_next for this rank's
 * rows.  One fused kernel when the plan allows (world == 1, S <= 128). */
int psvi_mvn_phase_update_sample(const psvi_plan* plan, const float* eps,
                                 const float* g_shard, float* params, float* adam_m,
                                 float* adam_v, const psvi_adam_hp* hp, double* kl_out,
                                 int32_t include_kl, const float* eps_next,
                                 float* x_next, void* stream);

/* Tiled corr / m / v state for a run of inner steps (full-cov, world 1,
 * S <= 128): the packed triangles re-laid as 64x64 tiles in the update
 * kernel's fragment order, so every corr/m/v access is a contiguous 1 KB
 * wave transaction (the packed rows' scattered 256-byte runs stream at about
 * two thirds of that rate).  tstate: PSVI_Q_TILED_FLOATS floats.
 * to_tiled = 1 copies the corr parts of params / adam_m / adam_v in; 0 copies
 * them back (the mean / sd parts always stay in params / adam_m / adam_v).
 * psvi_inner_loop does this itself. */
int psvi_mvn_tiled_convert(const psvi_plan* plan, float* params, float* adam_m,
                           float* adam_v, float* tstate, int32_t to_tiled, void* stream);
/* psvi_mvn_phase_update with corr and its Adam state in tstate (mean / sd
 * and theirs stay in params / adam_m / adam_v; the packed corr parts are
 * neither read nor written until psvi_mvn_tiled_convert(..., 0)); with
 * eps_next / x_next also the next step's sample (fused). */
int psvi_mvn_phase_update_tiled(const psvi_plan* plan, const float* eps,
                                const float* g_shard, float* params, float* adam_m,
                                float* adam_v, float* tstate, const psvi_adam_hp* hp,
                                double* kl_out, int32_t include_kl,
                                const float* eps_next, float* x_next, void* stream);

/* ---- outer objective ------------------------------------------------------
 * PSVI.psvi_elbo (psvi/inference/psvi_classes.py:445-486) with the sampled KL
 * of every layer (VIMixin.sampled_nkl, psvi/models/neural_net.py:110-115;
 * MultivariateNormalVIMixin.sampled_nkl, neural_net.py:438-442), world == 1,
 * 2 <= S <= 2048.  The plan's M counts ALL rows of the batch: x_all
 * ([M][D]) = cat(u, xbatch) with the n_pseudo pseudopoints first, z_all their
 * class ids, w_all the row weights -- N f(v)_m for the pseudopoints, N / Nx
 * for the data rows -- and eps the draw order of model(all_data).
 *   loss_out[0] (double, written) <- sum_s W_s (data_s - pseudo_s) - mean_s lw_s,
 *       lw_s = -pseudo_s + nkl_s, W = softmax_s(lw)
 *   grad_params (PARAM_COUNT, nullable) <- d loss / d params (first order)
 *   grad_u ([n_pseudo][D], nullable; needs grad_params) <- d loss / d u
 *   grad_w (n_pseudo, nullable) <- d loss / d w_m (chain to v / alpha on the host)
 *   sample_out ([S][4] doubles, nullable) <- pseudo_s, data_s, nkl_s, W_s
 * The sampled KL uses L^-1 (x_s - mean) = eps_s (the reference's fp32
 * triangular solve overflows at fn2 sizes).  ws: PSVI_Q_OUTER_WS_BYTES. */
int psvi_outer_elbo_grad(const psvi_plan* plan, int32_t n_pseudo, const float* x_all,
                         const int32_t* z_all, const float* w_all, const float* eps,
                         const float* params, double* loss_out, float* grad_params,
                         float* grad_u, float* grad_w, double* sample_out, void* ws,
                         size_t ws_bytes, void* stream);

/* psvi_outer_elbo_grad plus the gradient of the pseudo rows' targets on a
 * Gaussian-likelihood plan (PSVI_regressor.psvi_elbo, psvi_classes.py:2034-2048,
 * with learn_z):
 *   grad_z (n_pseudo floats, nullable; needs grad_params) <- d loss / d z_m =
 *       -sum_s dlogit_sm, dlogit the head's coefficient-scaled d / d f, summed
 *       in sample order (one writer per element, no float atomics).
 * A non-NULL grad_z on a categorical plan returns PSVI_ESTATE.
 * psvi_outer_elbo_grad == psvi_outer_elbo_grad_ex(grad_z = NULL). */
int psvi_outer_elbo_grad_ex(const psvi_plan* plan, int32_t n_pseudo, const float* x_all,
                            const int32_t* z_all, const float* w_all, const float* eps,
                            const float* params, double* loss_out, float* grad_params,
                            float* grad_u, float* grad_w, float* grad_z, double* sample_out,
                            void* ws, size_t ws_bytes, void* stream);

/* PSVI_Ablated.psvi_elbo (psvi/inference/psvi_classes.py:1397-1408; also
 * PSVI_No_IW's, 1411): the outer objective without importance weighting,
 * over the data batch only (x_all = xbatch, the plan's M = Nx rows, w_all =
 * N / Nx each; no pseudopoints), 1 <= S <= 2048:
 *   loss_out[0] (double, written) <- mean_s data_s - mean_s nkl_s,
 *       data_s = sum_m w_m NLL_sm, nkl_s the sampled KL of the VILinear
 *       layers (every mean-field layer; LeNet's three linear layers)
 *   grad_params (PARAM_COUNT, nullable) <- d loss / d params (first order)
 *   sample_out ([S][4] doubles, nullable) <- 0, data_s, nkl_s, 1/S
 * A full-covariance plan returns PSVI_EUNSUP: the reference's sum over
 * VILinear modules is then the int 0 and 0.mean() raises.
 * ws: PSVI_Q_OUTER_WS_BYTES. */
int psvi_outer_ablated_elbo_grad(const psvi_plan* plan, const float* x_all,
                                 const int32_t* z_all, const float* w_all, const float* eps,
                                 const float* params, double* loss_out, float* grad_params,
                                 double* sample_out, void* ws, size_t ws_bytes, void* stream);

/* The backward half of psvi_outer_elbo_grad with caller-given per-sample
 * coefficients instead of the plan's own softmax over its S samples
 * (replaces the autograd backward of PSVI.psvi_elbo, psvi_classes.py:463-486,
 * when the samples are split over ranks):
 *   coef = [rowcoef (S x 2): d loss / d pseudo_s, d loss / d data_s |
 *           ck (S): d loss / d nkl_s | sck (1): the sum of ck over these samples]
 * (floats, device).  For the sample-sharded outer objective:
 * each rank runs psvi_outer_elbo_grad on a plan of its own samples for the
 * per-sample terms (sample_out), the host forms the softmax over ALL samples
 * (psvi.runtime.sharded.ShardedOuter), and each rank's grad_params / grad_u /
 * grad_w from this call are partial sums over its samples (sum over ranks).
 * S may be 1 here.  ws: PSVI_Q_OUTER_WS_BYTES. */
int psvi_outer_elbo_grad_coef(const psvi_plan* plan, int32_t n_pseudo, const float* x_all,
                              const int32_t* z_all, const float* w_all, const float* eps,
                              const float* params, const float* coef, float* grad_params,
                              float* grad_u, float* grad_w, void* ws, size_t ws_bytes,
                              void* stream);

/* psvi_outer_elbo_grad_coef with grad_z as psvi_outer_elbo_grad_ex (Gaussian
 * plans; coefficient 1 on every sample's pseudo term gives the target
 * gradient of the inner objective's weighted NLL). */
int psvi_outer_elbo_grad_coef_ex(const psvi_plan* plan, int32_t n_pseudo, const float* x_all,
                                 const int32_t* z_all, const float* w_all, const float* eps,
                                 const float* params, const float* coef, float* grad_params,
                                 float* grad_u, float* grad_w, float* grad_z, void* ws,
                                 size_t ws_bytes, void* stream);

/* Importance-weighted predictive evaluation of one test batch: PSVI.evaluate
 * (psvi_classes.py:1031-1108) and pred_on_grid (1130-1175), world == 1,
 * 2 <= S <= 2048.  Rows as psvi_outer_elbo_grad: x_all = cat(u, xtest), the
 * n_pseudo pseudopoints first; z_all their labels (test labels after);
 * w_all: N f(v) for the pseudopoints (the data rows' entries are unused).
 * Weights W = softmax_s(+sum_m w_m NLL_sm + sampled_nkl_s) -- the reference's
 * sign there (its pseudo_nll is the log-likelihood); correction = 0: W = 1/S.
 *   probs_out ([M - n_pseudo][C], nullable) <- sum_s W_s softmax(logits_s)
 *   stats_out[4] (double, written) <- entropy of W (over W > 0), normalised
 *     ESS (sum W)^2 / sum W^2 / S, correct predictions, summed test NLL
 *     (-log of the normalised probability of the label, clamped to fp32 eps).
 * ws: PSVI_Q_EVAL_WS_BYTES. */
int psvi_evaluate(const psvi_plan* plan, int32_t n_pseudo, const float* x_all,
                  const int32_t* z_all, const float* w_all, const float* eps,
                  const float* params, int32_t correction, float* probs_out,
                  double* stats_out, void* ws, size_t ws_bytes, void* stream);

/* The regressors' predictive evaluation of one test batch
 * (PSVI_regressor.evaluate, psvi_classes.py:2221-2264) on a Gaussian plan,
 * 2 <= S <= 2048.  Rows as psvi_evaluate: x_all = cat(u, xtest); y_all (fp32)
 * the pseudo targets, then the test targets in ORIGINAL units; w_all is not
 * read.  The reference sums its pseudo term over the samples as well, so
 * its weights are W = softmax_s(sampled_nkl_s) alone -- reproduced;
 * correction = 0: W = 1 / S.
 *   y_pred_j = sum_s W_s (f_sj y_std + y_mean)
 *   pred_out ([M - n_pseudo], nullable) <- y_pred
 *   stats_out[4] (double, written) <- entropy of W, normalised ESS, sum_j
 *     (y_pred_j - y_j)^2, sum_j log N(y_j; y_pred_j, 1 / sqrt(tau)).  The two
 *     sums are added per 256-row block with double atomics (as psvi_evaluate's):
 *     with more than 256 test rows their last bits may differ run to run.
 * A categorical plan returns PSVI_ESTATE.  ws: PSVI_Q_EVAL_WS_BYTES. */
int psvi_evaluate_regression(const psvi_plan* plan, int32_t n_pseudo, const float* x_all,
                             const float* y_all, const float* w_all, const float* eps,
                             const float* params, int32_t correction, float y_mean,
                             float y_std, float* pred_out, double* stats_out, void* ws,
                             size_t ws_bytes, void* stream);

/* ---- sparse black-box VI (run_sparsevi_with_bb_elbo) -----------------------
 * The sampled KL term of every mean-field layer (VIMixin.sampled_nkl,
 * psvi/models/neural_net.py:110-115) on a mean-field plan of any likelihood,
 * world == 1.  With theta_s = mu + sigma eps_s, sigma = softplus(rho), n
 * sampled elements and prior sd s0 (the log(2 pi) constants cancel):
 *   nkl_out[s] (S doubles, written; nullable) <- log p(theta_s) - log q(theta_s)
 *       = -n log s0 - |theta_s|^2 / (2 s0^2) + sum_i log sigma_i + |eps_s|^2 / 2
 *   grad_out (PARAM_COUNT floats, nullable, ADDED into) += d(-sum_s nkl_s) / d params:
 *       mu_i:  sum_s theta_si / s0^2
 *       rho_i: (sum_s theta_si eps_si / s0^2 - S / sigma_i) sigmoid(rho_i)
 * At least one of nkl_out / grad_out is given (PSVI_EINVAL otherwise); a NULL
 * one is skipped.  One writer per element, the sums over s and i in a fixed
 * order: bitwise reproducible run to run; no float atomics. */
int psvi_sampled_kl_grad(const psvi_plan* plan, const float* eps, const float* params,
                         double* nkl_out, float* grad_out, void* stream);

/* Per-sample, per-row log-likelihoods of a Bernoulli plan's M rows (the
 * network's forward pass; forward_through_coreset / predict_through_coreset,
 * psvi/inference/utils.py:108-141), world == 1:
 *   ll_out     ([S][M] floats, row index contiguous) <- -NLL_sm, unweighted
 *   logits_out ([S][M] floats, nullable)             <- the raw output f_sm
 *   nkl_out    (S doubles, nullable)                 <- as psvi_sampled_kl_grad
 * x_all ([M][D]), z_all (M class ids in {0, 1}), eps (EPS_COUNT: ONE draw for
 * all rows) and params as psvi_elbo_grad's.  No workspace. */
int psvi_row_loglik(const psvi_plan* plan, const float* x_all, const int32_t* z_all,
                    const float* eps, const float* params, float* ll_out, float* logits_out,
                    double* nkl_out, void* stream);

/* The greedy selection scores of sparse black-box VI (sparsebbvi.py:143-170)
 * from ll ([S][n_core + n_data], psvi_row_loglik's layout: core columns
 * first), nkl (S doubles), w_core (n_core floats) and sum_scaling = N / B:
 *   W_s         = softmax_s(sum_m w_m ll_sm + nkl_s)
 *   cll_sj      = ll_sj (1 - W_s)      (the reference scales, it does not centre)
 *   resid_s     = sum_scaling sum_n cll_sn - sum_m w_m cll_sm
 *   corr_n      = (cll_.n . resid) / |cll_.n| / S       -> corr_out (n_data)
 *   corecorr_m  = |cll_.m . resid| / |cll_.m| / S       -> corecorr_out (n_core)
 *   W_out (S floats) <- W
 *   result_out (4 doubles) <- max corr, its first arg (as a double), max
 *       corecorr (-inf when n_core == 0), attach = (n_core == 0 or max corr >
 *       max corecorr)
 * 2 <= S <= 2048, n_core >= 0 (w_core / corecorr_out may be NULL at 0),
 * n_data >= 1.  fp64 sums in a fixed order: bitwise reproducible. */
int psvi_select_scores(int32_t S, int32_t n_core, int32_t n_data, const float* ll,
                       const double* nkl, const float* w_core, double sum_scaling, float* W_out,
                       float* corr_out, float* corecorr_out, double* result_out, void* stream);

/* sparsevi_psvi_elbo (psvi/inference/utils.py:94-105) and its gradient with
 * respect to the core weights, from the same ll / nkl layout.  With c_sm =
 * -ll_sm over the core, d_s = -sum_n ll_sn over the data, a_s = (N / n_core)
 * sum_m w_m c_sm, lw_s = -a_s + nkl_s, W = softmax_s(lw), r_s = (N / n_data)
 * d_s - a_s, rbar = sum_s W_s r_s:
 *   loss_out[0] (double, written) <- rbar - mean_s lw_s
 *   grad_w (n_core floats) <- (N / n_core) sum_s c_sm [1 / S - W_s (1 + r_s - rbar)]
 * 2 <= S <= 2048, n_core >= 1, n_data >= 1; fixed-order fp64 sums. */
int psvi_select_weight_grad(int32_t S, int32_t n_core, int32_t n_data, const float* ll,
                            const double* nkl, const float* w_core, double N, double* loss_out,
                            float* grad_w, void* stream);

/* ---- Laplace coreset baselines (random, sparsevi, opsvi) -----------------
 * The Laplace fit of a weighted logistic regression on the coreset
 * (run_laplace, psvi/inference/baselines.py:35-70; model and
 * laplace_precision, psvi/models/logreg.py:17-26, 95-107), one launch of one
 * workgroup for the whole fit.  x_core ([n_core][d], d = D + 1: the caller
 * appends the ones column), y_core (n_core FLOAT labels: the likelihood is
 * y f - softplus(f) for any float y), w_core (n_core floats, >= 0), the prior
 * N(prior_mean, prior_sd^2) on every coordinate, theta (d floats, in / out).
 * T steps of torch.optim.Adam (PSVI_ADAM_TORCH arithmetic: step = lr / bc1,
 * denom = sqrt(v) / sqrt(bc2) + adam_eps) from zero moments and step count 0
 * -- every fit of the baselines starts from a new optimiser -- on
 *   loss = -sum_m w_m (y_m f_m - softplus(f_m)) - sum_j log N(theta_j),  f = x theta
 *   g    = -x^T (w o (y - sigmoid(f))) + (theta - prior_mean) / prior_sd^2
 * and then
 *   loss_out    (T doubles, nullable)  <- the loss before each step
 *   prec_out    (d floats)             <- 1 + sum_m w_m p_m (1 - p_m) x_mj^2 at the final theta
 *   samples_out ([S][d] floats)        <- theta + prec^(-1/2) o eps_s, written iff eps
 *                                         ([S][d] floats, nullable) is given
 * theta, the moments and every sum are fp64 inside the kernel, each sum with
 * one owner and a fixed order: bitwise reproducible; no atomics.  x_core stays
 * in LDS when n_core * d floats fit beside the state (160 KiB) and is read
 * from global memory otherwise.
 * Ranges (PSVI_EINVAL outside them): 2 <= d <= 256, 0 <= n_core <= 4096 (the
 * core pointers may be NULL at 0: the prior alone drives theta, prec = 1),
 * 0 <= S <= 2048 (S >= 1 with eps), 0 <= T <= 1048576, lr / betas / adam_eps /
 * prior_sd finite and > 0 (betas < 1).  A negative or NaN weight is
 * PSVI_EINVAL too: the entry reads w_core back before the launch, so it
 * synchronises the stream. */
typedef struct psvi_laplace_fit_req {
    int32_t n_core, d, S, T;
    const float* x_core;
    const float* y_core;
    const float* w_core;
    float prior_mean, prior_sd;
    float* theta;
    double lr, beta1, beta2, adam_eps;
    const float* eps;
    double* loss_out;
    float* prec_out;
    float* samples_out;
} psvi_laplace_fit_req;
int psvi_laplace_fit(const psvi_laplace_fit_req* req, void* stream);

/* Samples from the FULL-precision Laplace posterior at a fitted mode
 * (laplace_precision(diagonal=False), psvi/models/logreg.py:95-107;
 * MultivariateNormal(theta, precision_matrix=P).rsample, baselines.py:64-70),
 * one launch of one workgroup.  x_core ([n_core][d], ones column included),
 * w_core (n_core floats, >= 0), theta (d floats: psvi_laplace_fit's output,
 * read only), eps ([S][d] standard normals):
 *   p_m         = sigmoid(x_m . theta)
 *   P           = I + sum_m w_m p_m (1 - p_m) x_m x_m^T
 *   A           : lower-triangular, A^T A = P (the "reverse" Cholesky factor,
 *                 eliminated from the last row and column upwards); torch's
 *                 scale_tril, the lower Cholesky factor of P^-1, is A^-1
 *   prec_out    ([d][d] floats, nullable)  <- P, both triangles, exactly symmetric
 *   factor_out  ([d][d] floats, nullable)  <- A, exact zeros above the diagonal
 *   samples_out ([S][d] floats)            <- theta + y_s,  A y_s = eps_s (one
 *                                             forward substitution per sample)
 *   logdet_out  (1 double, nullable)       <- log det P = 2 sum_j log A_jj
 * Every eigenvalue of P is >= 1, so the factorisation needs neither pivoting
 * nor jitter.  theta, P (its lower triangle, packed), A and the substitutions
 * are fp64 in LDS, each sum with one owner and a fixed order; outputs are
 * rounded to float once: bitwise reproducible, no atomics.
 * Ranges (PSVI_EINVAL outside them): 2 <= d <= 128, 0 <= n_core <= 4096 (the
 * core pointers may be NULL at 0: P = I, samples = theta + eps), 0 <= S <=
 * 2048; eps is given iff S >= 1, and samples_out is required then.  A negative
 * or NaN weight is PSVI_EINVAL too: as psvi_laplace_fit, the entry reads
 * w_core back before the launch, so it synchronises the stream. */
typedef struct psvi_laplace_sample_full_req {
    int32_t n_core, d, S;
    const float* x_core;
    const float* w_core;
    const float* theta;
    const float* eps;
    float* prec_out;
    float* factor_out;
    float* samples_out;
    double* logdet_out;
} psvi_laplace_sample_full_req;
int psvi_laplace_sample_full(const psvi_laplace_sample_full_req* req, void* stream);

/* The selection scores and gradients of the Laplace baselines
 * (baselines.py:550-575, 617-635, 783-805) from samples ([S][d]), rows
 * ([n_core + n_data][d], core rows first), labels (n_core + n_data floats),
 * w_core (n_core floats) and sum_scaling = N / B:
 *   ll_sj       = y_j f_sj - softplus(f_sj),  f_sj = rows_j . samples_s
 *   cll_sj      = ll_sj - mean_s ll_sj    (these baselines centre; psvi_select_scores scales)
 *   resid_s     = sum_scaling sum_n cll_sn - sum_m w_m cll_sm
 *   corr_n      = (cll_.n . resid) / |cll_.n| / S       -> corr_out (n_data)
 *   corecorr_m  = |cll_.m . resid| / |cll_.m| / S       -> corecorr_out (n_core)
 *   result_out (4 doubles) <- as psvi_select_scores: max corr, its first arg,
 *       max corecorr (-inf when n_core == 0), attach
 *   grad_w (n_core floats, nullable)  <- -(cll_.m . resid) / S
 *   ll_out ([S][n_core + n_data] floats, nullable) <- ll
 *   grad_u ([n_core][d] floats, nullable) <- the gradient with respect to the
 *       core rows of -(1 / S) sum_s resid_s sum_m w_m cll_sm at constant resid
 *       (opsvi's u_function): -(w_m / S) sum_s (resid_s - mean resid)
 *       (y_m - sigmoid(f_sm)) samples_s, its last (ones) column set to 0
 * ll is rounded to float before any sum uses it (ll_out holds exactly the
 * values summed); the sums run in fp64 in a fixed order: bitwise reproducible.
 * Ranges (PSVI_EINVAL outside them): 2 <= S <= 2048, 2 <= d <= 256,
 * n_core >= 0 (w_core / corecorr_out / grad_w / grad_u may be NULL at 0),
 * n_data >= 1, n_core + n_data <= 2048. */
typedef struct psvi_laplace_scores_req {
    int32_t S, d, n_core, n_data;
    const float* samples;
    const float* rows;
    const float* labels;
    const float* w_core;
    double sum_scaling;
    float* corr_out;
    float* corecorr_out;
    double* result_out;
    float* grad_w;
    float* ll_out;
    float* grad_u;
} psvi_laplace_scores_req;
int psvi_laplace_scores(const psvi_laplace_scores_req* req, void* stream);

/* One geodesic-ascent step of GIGA (Campbell & Broderick, 2018; run_giga,
 * baselines.py:306-322, 362-413) from samples ([S][d]), the minibatch rows
 * ([n_data][d], ones column appended by the caller), labels (n_data floats)
 * and lw_in (S floats: the coreset's current unit vector, all zeros before
 * the first step); normalize(v) = v / max(|v|, 1e-12) as F.normalize:
 *   ll_sn    = y_n f_sn - softplus(f_sn),  cll_sn = ll_sn - mean_s ll_sn
 *   sum_lls  = sum_n cll_.n,  L = |sum_lls|,  ell = normalize(sum_lls)
 *   ell_n    = normalize(cll_.n)
 *   d        = normalize(ell - (ell . lw) lw)
 *   d_n      = normalize(ell_n - (ell_n . lw) lw)
 *   score_n  = d . d_n                              -> score_out (n_data)
 *   n*       = the first argmax of score,  ell* = ell_n*
 *   zeta0    = ell . ell*,  zeta1 = ell . lw,  zeta2 = ell* . lw
 *   gamma    = (zeta0 - zeta1 zeta2) / (zeta0 - zeta1 zeta2 + zeta1 - zeta0 zeta2)
 *   lw_out   = normalize((1 - gamma) lw + gamma ell*)   (S floats, not lw_in)
 *   scale    = 1 / |(1 - gamma) lw_out + gamma ell*|
 *   result_out (8 doubles) <- max score, n*, zeta0, zeta1, zeta2, gamma, scale, L
 *   ll_out ([S][n_data] floats, nullable) <- ll
 * scale divides the reference's weight update, w <- ((1 - gamma) w + gamma
 * e_pt) scale; it is taken with the NEW lw because the reference reassigns lw
 * before it forms that norm.  The attached point is a row of the minibatch
 * and the samples are fixed over a run, so ell* needs no core rows.
 * ll is rounded to float before any sum uses it; the sums run in fp64 in a
 * fixed order with one owner each: bitwise reproducible, no atomics.
 * Ranges (PSVI_EINVAL outside them): 2 <= S <= 2048, 2 <= d <= 256,
 * 1 <= n_data <= 2048; lw_out overlapping lw_in is PSVI_EINVAL. */
typedef struct psvi_giga_step_req {
    int32_t S, d, n_data;
    const float* samples;
    const float* rows;
    const float* labels;
    const float* lw_in;
    float* score_out;
    float* lw_out;
    float* ll_out;
    double* result_out;
} psvi_giga_step_req;
int psvi_giga_step(const psvi_giga_step_req* req, void* stream);

/* ---- coreset draws (PSVI.prune_coreset / the incremental-learning schedule) --
 * n indices of coreset rows drawn in proportion to the weights w (M floats,
 * f(v) of the PSVI classes), where the reference calls torch.multinomial
 * (psvi_classes.py:946-965, 1177-1192) -- on the library's own Philox stream,
 * so that a run stays a function of its seed, a CPU restatement predicts the
 * draw and every rank of a multi-GPU run draws the same rows.
 * Word j of the stream (seed, offset), offset a multiple of 4, is element
 * j % 4 of Philox4x32-10 at counter offset / 4 + j / 4 with key seed: the
 * indexing of psvi_randn.  Its uniform is U_j = (word_j + 0.5) 2^-32, exact in
 * fp64 and strictly inside (0, 1).  Both modes decide in fp64.
 * PSVI_DRAW_REPLACE (independent draws):  C_i = the inclusive fp64 prefix sum
 *   of w in index order; draw j takes t = U_j C_{M-1} and returns the smallest
 *   i with C_i > t, clamped to the last index with w_i > 0 -- a row of zero
 *   weight is never returned.  The prefix is summed in runs of consecutive
 *   weights whose totals are added in run order: a fixed association, the same
 *   in every launch, that differs from a strictly sequential sum by fp64
 *   rounding only (not at all when the sums are exact).
 *   Consumes 4 ceil(n / 4) words of the stream.
 * PSVI_DRAW_NOREPLACE (n distinct rows; Efraimidis-Spirakis sampling, the law
 *   of drawing one row at a time in proportion to the remaining weights, as
 *   torch.multinomial(replacement=False)):  key_i = log(U_i) / w_i for
 *   w_i > 0, -inf for w_i == 0; the n largest keys win and come out in
 *   descending key order.  Equal keys are ordered by the lower index first
 *   (with equal weights two equal 32-bit words make a tie).
 *   Consumes 4 ceil(M / 4) words of the stream, whatever n.
 * Optional gather: rows ([M][D] floats) -> rows_out ([n][D]) and targets (M
 * 4-byte slots: int32 labels or fp32 values, copied as bits) -> targets_out
 * (n), both by idx_out.
 * status_out (one device int32): 0 ok; 1 a weight is negative or not finite;
 * 2 the weights sum to zero; 3 NOREPLACE with fewer than n positive weights.
 * On a non-zero status every idx_out entry is -1 and rows_out / targets_out are
 * not written.  The call itself returns 0 then: the status is the caller's to
 * read (one host read; a draw runs once per prune / increment, never per step).
 * Refused without a launch: PSVI_EINVAL for a NULL w / idx_out / status_out,
 * offset % 4 != 0, an unknown mode, M < 1, n < 1, n > 2^24, D < 0, rows /
 * targets without their output, n > M under NOREPLACE; PSVI_EUNSUP for
 * M > 4096 (the prefix and the sort's keys live in LDS).
 * Bitwise reproducible: no atomics on anything that decides an index. */
#define PSVI_DRAW_REPLACE   0
#define PSVI_DRAW_NOREPLACE 1
typedef struct psvi_coreset_draw_req {
    const float* w;
    int32_t M, n, mode;
    uint64_t seed, offset;
    const float* rows;      /* nullable */
    int32_t D;
    const void* targets;    /* nullable */
    int32_t* idx_out;
    float* rows_out;        /* required with rows */
    void* targets_out;      /* required with targets */
    int32_t* status_out;
} psvi_coreset_draw_req;
int psvi_coreset_draw(const psvi_coreset_draw_req* req, void* stream);

/* ---- k-means clustering (the k-means data-selection baselines) -------------
 * The clustering behind KmeansCluster (reference psvi/inference/utils.py:
 * 455-552, which calls sklearn's KMeans on the CPU): K clusters of the N rows
 * x ([N][D] device fp32), seeded from the library's Philox stream so that a
 * selection stays a function of its seed, then Lloyd iterations.
 * Arithmetic: every number that decides a label or a seed is fp64.  x is
 * widened exactly, the centres live in fp64, d(i,k) = sum_f (x_if - c_kf)^2
 * (the differences squared and added, not the expanded form).  A result
 * differs from a float64 restatement of these rules by the rounding of the
 * order of fp64 sums only; with a relative margin between the best and the
 * second-best centre of every row far above D 2^-53 the labels are equal.
 * Initial centres: centres_in ([K][D] device fp64) when given; seeds_out is
 * then all -1 and no word of the stream is used.  Otherwise k-means++ with
 * one candidate per centre.  Word j of the stream (seed, offset) and its
 * uniform U_j = (word_j + 0.5) 2^-32 are those of psvi_coreset_draw; centre j
 * takes word 4 j (one quad per centre: the call consumes 4 K words).
 *   centre 0 = row floor(U_0 N), clamped to N - 1;
 *   centre j >= 1: m_i = min over the chosen centres of d(i, .), C = the
 *   inclusive fp64 prefix sum of m in index order, t = U_{4j} C_{N-1}, the
 *   smallest i with C_i > t, clamped to the last i with m_i > 0.  A chosen
 *   row has m_i = 0 and repeats its predecessor's prefix value, so it is
 *   never chosen again.  The prefix is summed in runs of 64 consecutive rows
 *   whose totals are added in run order (C_i = the runs before + within the
 *   run): the fixed association of PSVI_DRAW_REPLACE, equal to the sequential
 *   sum when the sums are exact.
 * Lloyd: iteration t = 0, 1, ... assigns label_i = argmin_k d(i,k) against
 * the centres C_t, the lowest k among equal distances.
 *   If t == max_iter, or t > 0 and the summed squared shift
 *   sum_kf (C_t - C_{t-1})^2 <= tol, this was the final assignment: stop,
 *   n_iter = t.
 *   Else if t > 0 and no label changed: stop, n_iter = t + 1 (the update
 *   would reproduce C_t bit for bit and is not made; the count is
 *   sklearn's n_iter_).
 *   Else C_{t+1,k} = (the sum of cluster k's rows) / its count; a cluster
 *   without rows keeps its centre (sklearn's relocation is not ported).
 * max_iter == 0 is the assignment against the initial centres alone.
 * Outputs (device): centres_out [K][D] fp64 (also the working centres),
 * labels_out [N], counts_out [K] (of labels_out), seeds_out [K] (nullable),
 * inertia_out [1] = sum_i d(i, label_i) against centres_out, n_iter_out [1],
 * status_out [1]: 0 ok; 1 a non-finite input (a row or a given centre);
 * 2 fewer than K distinct rows reachable by the seeding (all remaining
 * distances zero).  On a non-zero status every label is -1, counts_out,
 * inertia_out and n_iter_out are 0, centres_out is unspecified and seeds_out
 * holds the rows chosen before the failure, then -1.  The call returns 0 then:
 * the status is the caller's to read.
 * Determinism: no atomic on anything that decides a label, a centre, the
 * inertia or a seed.  Cluster sums are per-workgroup partials of consecutive
 * rows, added in row order and combined in workgroup order; the inertia meets
 * in a fixed tree.  Two calls with the same arguments (ws_bytes included) are
 * bitwise equal.
 * Launches: ordinary ones only -- no workgroup waits for another.  The
 * iterations are enqueued 16 at a time; a device word `done` makes the
 * launches behind the stopping one return at once, and the call reads it once
 * per 16 iterations (the call synchronises the stream then, and returns with
 * the last launch enqueued).  Centres and rows are staged in LDS in tiles of
 * out[2] columns; D above that is tiled.
 * psvi_kmeans_query(N, D, K, out), no device needed: out[0] = the ws bytes
 * from which the cluster sums are formed in the assignment launch (one
 * partial per workgroup, x read from memory once per iteration), out[1] = the
 * least ws bytes a call takes (one partial), out[2] = the columns of a tile,
 * out[3] = the assignment workgroups.  Between out[1] and out[0] the sums run
 * as a second launch over as many row chunks as the workspace holds partials;
 * the two forms differ by the rounding of the order of sums only.
 * PSVI_EINVAL: a NULL request, x or non-nullable output; N < 1, D < 1, K < 1,
 * K > N; offset % 4 != 0; max_iter < 0; tol negative or not finite.
 * PSVI_EUNSUP: K > 128, D > 4096, N > 2^24.  PSVI_ENOSPC: ws NULL or
 * ws_bytes < out[1]. */
typedef struct psvi_kmeans_req {
    const float* x;            /* [N][D] rows, device fp32 */
    int32_t N, D, K;
    const double* centres_in;  /* [K][D] nullable: given initial centres */
    uint64_t seed, offset;     /* Philox stream of the seeding when centres_in == NULL; offset % 4 == 0 */
    int32_t max_iter;          /* >= 0 centre updates */
    double tol;                /* >= 0: stop when the summed squared centre shift <= tol */
    double* centres_out;       /* [K][D] */
    int32_t* labels_out;       /* [N] */
    int32_t* counts_out;       /* [K] */
    int32_t* seeds_out;        /* [K] row indices the seeding chose (nullable; -1s with centres_in) */
    double* inertia_out;       /* [1] */
    int32_t* n_iter_out;       /* [1] */
    int32_t* status_out;       /* [1] */
    void* ws;
    size_t ws_bytes;
} psvi_kmeans_req;
int psvi_kmeans(const psvi_kmeans_req* req, void* stream);
int psvi_kmeans_query(int32_t N, int32_t D, int32_t K, int64_t* out);

/* ---- MFVI regression baselines (fit, run_mfvi_regressor) -------------------
 * The whole fit of a mean-field Gaussian-likelihood MLP on a FIXED batch (fit,
 * psvi/inference/baselines.py:1283-1346: every step takes next(iter(loader)) of
 * an unshuffled loader), one launch, for G independent members -- one per
 * candidate precision tau (run_mfvi_regressor's model selection,
 * baselines.py:1117-1144) -- each on one persistent workgroup; nothing is
 * shared between members, so a member's numbers depend on its own tau, offset
 * and eps only, not on G or on its index.
 * desc: the network (make_regressor_net, neural_net.py:300-331: Linear-ReLU
 * ... Linear): dims[n_layers] == 1, S samples, M = the batch rows B, prior_sd.
 * Each member runs T steps of
 *   loss = scale sum_{s,b} [tau_g / 2 (f_sb - y_b)^2 + log(2 pi / tau_g) / 2]
 *          + sum_layers KL(q || N(0, prior_sd^2))        (summed over s, not averaged)
 * with the mean-field gradient of psvi_elbo_grad, each followed by one
 * torch.optim.Adam step (PSVI_ADAM_TORCH arithmetic in fp32) with step number
 * step0 + t + 1.  A new fit passes step0 = 0 and zeroed adam_m / adam_v; a fit
 * split over calls carries params, adam_m, adam_v, step0 + T and (Philox mode)
 * offset + T * round_up(EPS_COUNT, 4) to the next call and gives the numbers of
 * one call bit for bit.
 *   x ([B][D]), y ([B]): the batch, device fp32;  scale: n_train / B
 *   tau    (G floats, HOST memory, finite and > 0)
 *   params, adam_m, adam_v ([G][P] device floats, in / out), P =
 *          PSVI_Q_PARAM_COUNT of a mean-field plan of desc (out[2] of the query)
 *   eps    ([G][T][EPS_COUNT] device floats in the library's eps layout), or
 *          NULL: member g's step t takes exactly what psvi_randn(seed,
 *          offset[g] + t * round_up(EPS_COUNT, 4)) writes; offset (G uint64,
 *          HOST memory, each a multiple of 4).  The two modes agree bit for bit.
 *   loss_out ([G][T] device doubles, nullable) <- the loss before each step
 *   ws     G * out[1] bytes of device scratch (may be NULL when out[1] == 0)
 * tau and offset are read on the host during the call; every other pointer is
 * a device pointer as everywhere else.
 * Numerics: the network, the gradient sums and Adam accumulate in fp32 (the
 * arithmetic of the step-by-step path), the per-row NLL terms, the sum of the
 * KL terms and the bias corrections in fp64.  Every sum has one owner and a
 * fixed order, the loss meets in a fixed tree: run-to-run bitwise equal; no
 * atomics.
 * Placement: params / adam_m / adam_v, the gradient accumulators and the batch
 * stay in LDS when they fit the 160 KiB beside the working set (two n_tot
 * vectors and a chunk of min(B, 16) rows' activations); otherwise they are
 * read and written in global memory (the accumulators in ws).
 * psvi_mfvi_fit_query: out[0] = 1 (LDS) / 0 (global memory), out[1] = ws bytes
 * per member, out[2] = P, out[3] = EPS_COUNT; no device needed.
 * Ranges (PSVI_EINVAL outside them): 2 <= n_layers <= 4 (1..3 hidden layers),
 * dims[0] <= 128, hidden dims <= 64, dims[n_layers] == 1, 1 <= M <= 512,
 * 1 <= S <= 64, prior_sd > 0, 1 <= G <= 16, 0 <= T <= 1048576, 0 <= step0,
 * step0 + T <= 2^30, scale / lr / adam_eps finite and > 0, 0 < betas < 1;
 * ws_bytes below G * out[1] is PSVI_ENOSPC. */
typedef struct psvi_mfvi_fit_req {
    const psvi_net_desc* desc;
    int32_t G, T, step0;
    const float* x;
    const float* y;
    double scale;
    const float* tau;
    float* params;
    float* adam_m;
    float* adam_v;
    double lr, beta1, beta2, adam_eps;
    const float* eps;
    uint64_t seed;
    const uint64_t* offset;
    double* loss_out;
    void* ws;
    size_t ws_bytes;
} psvi_mfvi_fit_req;
int psvi_mfvi_fit(const psvi_mfvi_fit_req* req, void* stream);
int psvi_mfvi_fit_query(const psvi_net_desc* desc, int64_t* out);

/* ---- predictive scores (the MFVI data-selection baselines) ----------------
 * The scoring pass of run_selection_with_mfvi (reference
 * psvi/inference/baselines.py:1515-1952; MeanFieldVI.test / after_epoch,
 * psvi/inference/utils.py:342-387; ScoreSelection._get_uncertainty_score,
 * utils.py:992-1084): a forward pass of the plan's S-sample mean-field
 * categorical net over n_rows rows in ONE launch, and per row
 *   mean_logits = mean over s of logits_s;  p = softmax_c(mean_logits)
 *   least_conf  = 1 - max_c p            entropy = -sum_c p log(p + 1e-20)
 *   el2n        = | p - onehot(z) |_2    correct = 1.0 if argmax_c mean_logits == z
 * (the softmax of the mean logit, not the mean of softmaxes; the first index
 * among equal maxima, as torch.argmax), and with the three state vectors,
 * MeanFieldVI.after_epoch's forgetting update in its order:
 *   forgetting += (last_acc > correct); last_acc = correct;
 *   never_learnt = min(never_learnt, 1 - correct).
 * stats_out[0] <- sum_j correct_j, stats_out[1] <- sum_j -log p_j[z_j]
 * (written, not accumulated).
 * eps holds one block of EPS_COUNT floats (psvi_elbo_grad's layout) per
 * rows_per_draw rows: rows [k rpd, (k + 1) rpd) use block k, as the reference
 * draws fresh weights for every minibatch of an unshuffled loader.  The plan's
 * M is not read; its scratch serves one call at a time.
 * Numerics: fp32 network and scores, every dot product from the bias over the
 * inputs in ascending order, the mean over s in ascending s; stats_out in
 * double: a fixed tree per group of rows, then the workgroups' partials in
 * a fixed strided-then-tree order by a last one-workgroup kernel.  Every per-row output has one
 * writer; no atomics; two runs are bitwise equal.  [S][n_rows][C] logits are
 * never written to memory.
 * Errors: PSVI_ESTATE for a full-covariance, LeNet, Gaussian or Bernoulli plan
 * or world > 1; PSVI_EINVAL for n_rows / rows_per_draw < 1, null x / eps /
 * params, no output requested, the state pointers not given together, or an
 * output that reads labels without z; PSVI_EUNSUP when one unit's weights of a
 * layer and one row's activations exceed the 160 KiB of LDS.  Labels outside
 * [0, C) are not detected here (a row with one counts as wrong, with
 * -log p = 0): the caller checks them. */
typedef struct psvi_predict_scores_req {
    const psvi_plan* plan;     /* mean-field, categorical, world 1; its M is NOT read   */
    int32_t n_rows;            /* >= 1, any value                                         */
    int32_t rows_per_draw;     /* >= 1: rows [k*rpd, (k+1)*rpd) use eps block k           */
    const float*   x;          /* [n_rows][D]                                             */
    const int32_t* z;          /* [n_rows] class ids; nullable if no output needs labels  */
    const float*   eps;        /* [ceil(n_rows/rpd)][EPS_COUNT], psvi_elbo_grad's layout  */
    const float*   params;
    float* mean_logits;        /* [n_rows][C]   mean over s of logits_s      (nullable)   */
    float* least_conf;         /* [n_rows]  1 - max_c p                      (nullable)   */
    float* entropy;            /* [n_rows]  -sum_c p log(p + 1e-20)          (nullable)   */
    float* el2n;               /* [n_rows]  | p - onehot(z) |_2              (nullable)   */
    float* correct;            /* [n_rows]  1.0 if argmax_c mean logit == z  (nullable)   */
    float* last_acc;           /* [n_rows] in/out, forgetting state          (nullable)   */
    float* forgetting;         /* [n_rows] in/out                            (nullable)   */
    float* never_learnt;       /* [n_rows] in/out                            (nullable)   */
    double* stats_out;         /* [2]: correct count, sum_j -log p_j[z_j]    (nullable)   */
} psvi_predict_scores_req;
int psvi_predict_scores(const psvi_predict_scores_req* req, void* stream);
/* What psvi_predict_scores does with `plan` at rows_per_draw (no device
 * needed): out[0] = the rows of a group, out[1] = the floats of the W tile in
 * LDS, out[2 + l] = the output units per tile of layer l (less than the
 * layer's width: the layer runs in several tiles); out holds
 * 2 + PSVI_MAX_LAYERS values, zero past the last layer.  Errors as
 * psvi_predict_scores' for the plan and rows_per_draw. */
int psvi_predict_query(const psvi_plan* plan, int32_t rows_per_draw, int64_t* out);

/* ---- second order (the `hyper` trainer's implicit hypergradient) ----------
 * Hessian-vector product of the negative inner ELBO (psvi_inner_step's
 * objective, KL included) at fixed eps, world == 1:
 *   hv_out (PARAM_COUNT) <- H vec
 *   du_out ([M][D], nullable) <- d/du (vec . d elbo / d params)
 *   dw_out (M, nullable)      <- d/dw (vec . d elbo / d params)
 * -- the products hypergrad's CG_normaleq takes from autograd through
 * GradientDescent's fp_map (psvi/hypergrad/hypergradients.py:199-244, 300-311,
 * diff_optimizers.py:51-60; PSVI.hyper_step psvi_classes.py:602-687):
 * J^T x = x - lr H x, J x = x - lr H x (jvp), torch_grad(w_mapped, hparams, v)
 * = -lr (du_out, dw_out chained to v).  Forward-over-reverse (R-op) through
 * the per-sample network, one workgroup per sample (the model's per-sample
 * weights and row chunks in LDS; PSVI_EUNSUP when they do not fit).
 * ws: PSVI_Q_HVP_WS_BYTES. */
int psvi_hvp(const psvi_plan* plan, const float* u, const int32_t* z, const float* w,
             const float* eps, const float* params, const float* vec, float* hv_out,
             float* du_out, float* dw_out, void* ws, size_t ws_bytes, void* stream);

/* psvi_hvp over this plan's samples only, for the sample-sharded second-order
 * trainers (PSVI.hyper_step's CG_normaleq products and PSVI.nested_step's
 * reverse pass, psvi/hypergrad/hypergradients.py:199-244, 300-311;
 * psvi_classes.py:541-687, split over ranks): each rank runs it on a world-1
 * plan of its own samples with its slice of the global eps; include_kl = 1 on
 * exactly one rank adds the KL Hessian (sample-independent), 0 leaves it out,
 * so hv_out / du_out / dw_out summed over ranks (one all-reduce) equal
 * psvi_hvp over all S samples.  psvi_hvp == psvi_hvp_partial(include_kl = 1). */
int psvi_hvp_partial(const psvi_plan* plan, const float* u, const int32_t* z, const float* w,
                     const float* eps, const float* params, const float* vec,
                     int32_t include_kl, float* hv_out, float* du_out, float* dw_out, void* ws,
                     size_t ws_bytes, void* stream);

/* psvi_hvp_partial plus the mixed product w.r.t. the targets of a Gaussian
 * plan (the regressors' learn_z):
 *   dz_out (M floats, nullable) <- d/dz (vec . d elbo / d params) =
 *       -sum_s delta_dot_sm, delta_dot = w tau f_dot, summed in sample order.
 * A non-NULL dz_out on a categorical plan returns PSVI_ESTATE.
 * psvi_hvp_partial == psvi_hvp_ex(dz_out = NULL). */
int psvi_hvp_ex(const psvi_plan* plan, const float* u, const int32_t* z, const float* w,
                const float* eps, const float* params, const float* vec, int32_t include_kl,
                float* hv_out, float* du_out, float* dw_out, float* dz_out, void* ws,
                size_t ws_bytes, void* stream);

/* Reverse of one Adam step (either variant) for the nested trainer's
 * reverse-mode pass through the unrolled inner loop (PSVI.nested_step,
 * psvi_classes.py:541-600; DifferentiableAdam._update optim.py:318-367 /
 * adam_step diff_optimizers.py:184-213).  The step took (p, m, v, grad) to
 * (p', adam_m, adam_v) with Adam step hp->step; given lt = adjoint of p' and
 * lm / lv = adjoints of (adam_m, adam_v) (in/out: replaced by the adjoints of
 * the step's incoming m, v), writes lg_out = adjoint of grad.  The adjoint of
 * p is lt + H^T lg_out (psvi_hvp at p).  Evaluated in double from the fp32
 * buffers: lg_out's two terms cancel almost fully on a fresh Adam state.
 * n = 0 is a no-op that returns 0. */
int psvi_adam_adjoint(int64_t n, const float* lt, float* lm, float* lv, const float* adam_m,
                      const float* adam_v, const float* grad, float* lg_out,
                      const psvi_adam_hp* hp, void* stream);

/* ---- utilities ----------------------------------------------------------- */
/* out[i] ~ N(0,1), Philox4x32-10 counter (seed, offset + i) + Box-Muller.
 * Throughput-mode replacement for torch's normal_() draw (not bit-identical
 * to torch's generator; parity mode passes torch-drawn eps instead). */
int psvi_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
/* flag[0] |= 1 when any of the n values at data (dtype 0: float, 1: double;
 * device) is NaN or +-inf; flag is a caller-zeroed device int32.  The HIP
 * path's stand-in for torch.autograd.set_detect_anomaly, which the reference
 * driver turns on (psvi/experiments/flow_psvi.py:50): PSVI's trainers check
 * their ELBO / loss / gradient buffers with it and read the flag once per
 * outer step when anomaly detection is enabled. */
int psvi_nonfinite(const void* data, int64_t n, int32_t dtype, int32_t* flag, void* stream);
/* Generic fused Adam over n floats (either variant). */
int psvi_adam_update(int64_t n, float* params, const float* grad, float* adam_m,
                     float* adam_v, const psvi_adam_hp* hp, void* stream);

/* ---- hyper_step's conjugate-gradient iteration (CG_normaleq) ----
 * Replaces the vector work of one iteration of the reference's
 * psvi/hypergrad/CG_torch.py:21-43 cg() over hypergradients.py:217-230's
 * normal-equation operator A(p) = vmj - J vmj, vmj = lr H_A p, J y = y - lr
 * H_B y, given the two fp32 Hessian-vector products hv1 = H_A p (from p32)
 * and hv2 = H_B vmj32 (psvi_hvp):
 *   psvi_cg_scale:    vmj32 = float(lr hv1)  (hv2's input)
 *   psvi_cg_pap:      state[1] = p . A p
 *   psvi_cg_residual: alpha = state[0] / state[1]; r -= alpha A p; state[2] =
 *                     r . r; done (state[3]) |= sqrt(state[2]) < tol; the step
 *                     length for x (state[4]: 0 once done), beta (state[5]),
 *                     and rTr (state[0]) unless done
 *   psvi_cg_update:   x += state[4] p; unless done p = r + beta p, p32 = float(p)
 * state: 7 float64 on the device, [0] = r . r and the rest 0 on entry to the
 * first iteration; x = 0, r = p = b (float64), p32 = float(b).  Where the
 * reference breaks, x keeps its last iterate and p freezes (the step length
 * is selected, never multiplied by a non-finite alpha); the caller reads
 * state[3] when it wants to stop.  ws: psvi_cg_ws_bytes() bytes, zeroed once
 * (the grid sums leave their counter at 0).  The sums are deterministic. */
size_t psvi_cg_ws_bytes(void);
int psvi_cg_scale(int64_t n, const float* hv, double lr, float* out, void* stream);
int psvi_cg_pap(int64_t n, const float* hv1, const float* hv2, double lr, const double* p,
                double* state, void* ws, size_t ws_bytes, void* stream);
int psvi_cg_residual(int64_t n, const float* hv1, const float* hv2, double lr, double* r,
                     double* state, double tol, void* ws, size_t ws_bytes, void* stream);
int psvi_cg_update(int64_t n, double* x, double* p, float* p32, const double* r,
                   const double* state, void* stream);

const char* psvi_last_error(void);
const char* psvi_version(void);

/* Diagnostics (ablation masks, A/B switches, per-phase stamps:
   psvi_debug_set / psvi_debug_set_ptr / psvi_debug_loop_timing) are exported
   for profiling tools but are not part of this interface: they are declared
   in the library's internal header csrc/psvi_diag.h. */

#ifdef __cplusplus
}
#endif
#endif /* PSVI_HIP_H */
