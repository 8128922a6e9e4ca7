// kernels_select.hip -- the greedy point selection and the weight objective of
// the sparse black-box VI coreset construction, from the row log-likelihoods
// ll [S][n_core + n_data] (psvi_row_loglik; core columns first) and the
// sampled KL term nkl [S].
//
// Reference:
//   run_sparsevi_with_bb_elbo   psvi/inference/sparsebbvi.py:143-170 (scores)
//   forward_through_coreset     psvi/inference/utils.py:108-122
//   sparsevi_psvi_elbo          psvi/inference/utils.py:94-105
//
// Scores:  W = softmax_s(sum_m w_m ll_sm + nkl_s), cll_sj = ll_sj (1 - W_s) (the
// reference's einsum "s,ns->ns" scales by W_s; it does not subtract a mean),
//   resid_s = (N / B) sum_n cll_sn - sum_m w_m cll_sm,
//   corr_n = (cll_.n . resid) / |cll_.n| / S, corecorr_m = |cll_.m . resid| / |cll_.m| / S.
// resid is a difference of two sums of like size, so every sum here runs in
// fp64.  Weight objective: c_sm = -ll_sm, d_s = -sum_n ll_sn, a_s = (N / Nu)
// sum_m w_m c_sm, lw_s = -a_s + nkl_s, W = softmax(lw), r_s = (N / B) d_s - a_s:
//   loss = sum_s W_s r_s - mean_s lw_s
//   d loss / d a_s = 1 / S - W_s (1 + r_s - rbar)   (d W_t / d a_s = -W_t (1[t = s] - W_s))
//   d loss / d w_m = (N / Nu) sum_s c_sm d loss / d a_s.
// One workgroup: S <= 2048 per-sample terms live in LDS; a thread owns whole
// samples (loops over the rows) or whole columns (loops over the samples), so
// every sum has one owner and a fixed order; the block-wide sums meet in a
// fixed tree.  No atomics.
#include "psvi_internal.hpp"

namespace psvi {

// softmax over lw[0, S) in place (LDS): W_s = exp(lw_s - max) / sum
__device__ __forceinline__ void sel_softmax(double* lw, int S, double* red) {
    double mx = -INFINITY;
    for (int s = threadIdx.x; s < S; s += kSelThreads) mx = fmax(mx, lw[s]);
    mx = tree_max<kSelThreads>(mx, red);
    double se = 0.0;
    for (int s = threadIdx.x; s < S; s += kSelThreads) {
        const double e = exp(lw[s] - mx);
        lw[s] = e;
        se += e;
    }
    se = tree_sum<kSelThreads>(se, red);
    for (int s = threadIdx.x; s < S; s += kSelThreads) lw[s] /= se;
    __syncthreads();
}

struct SelArgs {
    int S, Nu, B;
    const float* ll;     // [S][Nu + B]
    const double* nkl;   // [S]
    const float* w;      // [Nu]
    double scale;        // scores: N / B; weight objective: N
    float* W_out;        // [S]
    float* corr;         // [B]
    float* corecorr;     // [Nu]
    double* result;      // [4]
    double* loss;        // [1]
    float* grad_w;       // [Nu]
};

__global__ __launch_bounds__(kSelThreads) void select_scores_kernel(SelArgs a) {
    __shared__ double Wl[kSelMaxS], resid[kSelMaxS], red[kSelThreads];
    __shared__ int redi[kSelThreads];
    const int S = a.S, Nu = a.Nu, B = a.B, M = Nu + B, tid = threadIdx.x;
    // per sample: the core's weighted log-likelihood and the data's sum
    for (int s = tid; s < S; s += kSelThreads) {
        const float* row = a.ll + (size_t)s * M;
        double core = 0.0, data = 0.0;
        for (int m = 0; m < Nu; ++m) core += (double)a.w[m] * row[m];
        for (int n = 0; n < B; ++n) data += (double)row[Nu + n];
        Wl[s] = core + a.nkl[s];
        resid[s] = a.scale * data - core;  // times (1 - W_s) below
    }
    sel_softmax(Wl, S, red);
    for (int s = tid; s < S; s += kSelThreads) {
        resid[s] *= 1.0 - Wl[s];
        a.W_out[s] = (float)Wl[s];
    }
    __syncthreads();
    // per column: cll_.j . resid and |cll_.j|, samples in order
    double best = -INFINITY, bestc = -INFINITY;
    int besti = 0x7fffffff;
    for (int j = tid; j < M; j += kSelThreads) {
        double dot = 0.0, sq = 0.0;
        for (int s = 0; s < S; ++s) {
            const double c = (double)a.ll[(size_t)s * M + j] * (1.0 - Wl[s]);
            dot += c * resid[s];
            sq += c * c;
        }
        if (j < Nu) {
            const double v = fabs(dot) / sqrt(sq) / S;
            a.corecorr[j] = (float)v;
            bestc = fmax(bestc, v);
        } else {
            const double v = dot / sqrt(sq) / S;
            a.corr[j - Nu] = (float)v;
            if (v > best) {  // columns ascending per thread: the first of equal values stays
                best = v;
                besti = j - Nu;
            }
        }
    }
    bestc = tree_max<kSelThreads>(bestc, red);
    // max corr and its first argument: (value, index) pairs in a fixed tree
    tree_argmax_first<kSelThreads>(best, besti, red, redi);
    if (tid == 0) {
        a.result[0] = red[0];
        a.result[1] = (double)(redi[0] == 0x7fffffff ? 0 : redi[0]);
        a.result[2] = bestc;
        a.result[3] = (Nu == 0 || red[0] > bestc) ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(kSelThreads) void select_weight_grad_kernel(SelArgs a) {
    __shared__ double Wl[kSelMaxS], rs[kSelMaxS], red[kSelThreads];
    const int S = a.S, Nu = a.Nu, B = a.B, M = Nu + B, tid = threadIdx.x;
    const double sp = a.scale / Nu, sd = a.scale / B;
    double lwsum = 0.0;
    for (int s = tid; s < S; s += kSelThreads) {
        const float* row = a.ll + (size_t)s * M;
        double core = 0.0, data = 0.0;
        for (int m = 0; m < Nu; ++m) core -= (double)a.w[m] * row[m];
        for (int n = 0; n < B; ++n) data -= (double)row[Nu + n];
        const double as = sp * core, lw = -as + a.nkl[s];
        Wl[s] = lw;
        rs[s] = sd * data - as;
        lwsum += lw;
    }
    lwsum = tree_sum<kSelThreads>(lwsum, red);
    sel_softmax(Wl, S, red);
    double rb = 0.0;
    for (int s = tid; s < S; s += kSelThreads) rb += Wl[s] * rs[s];
    rb = tree_sum<kSelThreads>(rb, red);
    if (tid == 0) a.loss[0] = rb - lwsum / S;
    // d loss / d a_s, in place of r_s
    for (int s = tid; s < S; s += kSelThreads) rs[s] = 1.0 / S - Wl[s] * (1.0 + rs[s] - rb);
    __syncthreads();
    for (int m = tid; m < Nu; m += kSelThreads) {
        double g = 0.0;
        for (int s = 0; s < S; ++s) g -= (double)a.ll[(size_t)s * M + m] * rs[s];
        a.grad_w[m] = (float)(sp * g);
    }
}

hipError_t launch_select_scores(int S, int Nu, int B, const float* ll, const double* nkl,
                                const float* w, double sum_scaling, float* W_out, float* corr,
                                float* corecorr, double* result, hipStream_t st) {
    if (S < 1 || S > kSelMaxS || Nu < 0 || B < 1) return hipErrorInvalidValue;
    SelArgs a{};
    a.S = S; a.Nu = Nu; a.B = B; a.ll = ll; a.nkl = nkl; a.w = w; a.scale = sum_scaling;
    a.W_out = W_out; a.corr = corr; a.corecorr = corecorr; a.result = result;
    hipLaunchKernelGGL(select_scores_kernel, dim3(1), dim3(kSelThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_select_weight_grad(int S, int Nu, int B, const float* ll, const double* nkl,
                                     const float* w, double N, double* loss, float* grad_w,
                                     hipStream_t st) {
    if (S < 1 || S > kSelMaxS || Nu < 1 || B < 1) return hipErrorInvalidValue;
    SelArgs a{};
    a.S = S; a.Nu = Nu; a.B = B; a.ll = ll; a.nkl = nkl; a.w = w; a.scale = N;
    a.loss = loss; a.grad_w = grad_w;
    hipLaunchKernelGGL(select_weight_grad_kernel, dim3(1), dim3(kSelThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace psvi
