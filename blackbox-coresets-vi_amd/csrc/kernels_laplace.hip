// kernels_laplace.hip -- the computational core of the Laplace coreset
// baselines (random, sparsevi, opsvi): the Laplace fit of a weighted logistic
// regression on the coreset, its diagonal precision and samples, and the
// selection scores / weight gradient / pseudo-input gradient from the samples'
// centred log-likelihoods.
//
// Reference:
//   run_laplace         psvi/inference/baselines.py:35-70
//   model               psvi/models/logreg.py:17-26
//   laplace_precision   psvi/models/logreg.py:95-107 (diagonal in the fit kernel; the
//                       full matrix in laplace_sample_full_kernel below)
//   scores / gradients  psvi/inference/baselines.py:550-575, 617-635, 783-805
//
// Fit: T torch-Adam steps on theta [d] of the negative log-joint
//   loss = -sum_m w_m (y_m f_m - softplus(f_m)) - sum_j log N(theta_j; mu0, sd0),  f = X theta
//   g    = -X^T (w o (y - sigmoid(f))) + (theta - mu0) / sd0^2
// in ONE launch of ONE workgroup: a chain of up to a million dependent steps
// on a few hundred numbers is latency, not throughput.  theta is double-
// buffered in LDS (the step reads one copy, the column owners write the
// other), m / v / theta live in the column owner's registers, X is staged to
// LDS (rows padded to an odd stride) when it fits beside them and read from
// global memory otherwise.  Two barriers per step:
//   rows:    thread t owns rows t, t + 256, ...: f_m, r_m = w_m (y_m - p_m) -> LDS,
//            its rows' share of the objective -> part[t]
//   columns: thread j < d owns column j: g_j over the rows in order, the Adam
//            update; thread 255 sums part[] and the prior in order -> loss_out[t]
// Every sum has one owner and a fixed order, all of them in fp64; theta is
// rounded to float on output only.  No atomics.
//
// Scores: one workgroup as kernels_select.hip, which scales ll by 1 - W_s where
// these baselines centre it by the per-row mean over the samples.  ll_sj = y_j f_sj -
// softplus(f_sj) is rounded to float (what ll_out holds) before any sum uses it.
//
// GIGA (Campbell & Broderick, 2018; baselines.py:306-322, 362-413): the
// geodesic direction of every minibatch point on the unit sphere of centred
// log-likelihood vectors, the greedy pick and the line-search step, one
// workgroup over the same float-rounded ll (giga_step_kernel below).
#include "lds_layout.hpp"

namespace psvi {

// overflow-safe Bernoulli terms of a logit f: e = exp(-|f|),
// sigmoid(f) = 1 / (1 + e) or e / (1 + e), softplus(f) = max(f, 0) + log1p(e)
__device__ __forceinline__ double lap_sigmoid(double f) {
    const double e = exp(-fabs(f));
    return f >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}
// y f - softplus(f) in BCEWithLogits' arrangement, -((1 - y) f + max(-f, 0) +
// log1p(e)): at a saturated logit on the label's side the first two terms
// vanish exactly and the tiny log1p(e) survives
__device__ __forceinline__ double lap_loglik(double y, double f) {
    return -((1.0 - y) * f + fmax(-f, 0.0) + log1p(exp(-fabs(f))));
}

struct LapFitArgs {
    int Nu, d, S, T, ds;
    const float *x, *y, *w, *eps;
    double mu0, inv_var0, log_norm0;  // log_norm0 = -log(sd0) - log(2 pi) / 2
    double lr, b1, b2, adam_eps;
    float* theta;
    double* loss;
    float* prec;
    float* samples;
};

template <bool XLDS>
__global__ __launch_bounds__(kLapThreads) void laplace_fit_kernel(LapFitArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lap_sm[];
    const int Nu = a.Nu, d = a.d, tid = threadIdx.x;
    const LapFitLds l = lap_fit_lds(lap_sm, Nu, a.ds, XLDS);
    double *th = l.th, *part = l.part, *r = l.r;
    float* xs = l.xs;
    const int ld = XLDS ? a.ds : d;
    if (XLDS) {
        for (int i = tid; i < Nu * d; i += kLapThreads) xs[(i / d) * ld + i % d] = a.x[i];
    }
    auto X = [&](int m, int j) -> double {
        return XLDS ? (double)xs[m * ld + j] : (double)a.x[(size_t)m * d + j];
    };
    double tj = 0.0, mj = 0.0, vj = 0.0;  // column owner's theta_j and Adam moments
    if (tid < d) {
        tj = (double)a.theta[tid];
        th[tid] = tj;
    }
    __syncthreads();
    double p1 = 1.0, p2 = 1.0;  // beta^t
    for (int t = 0; t < a.T; ++t) {
        const double* tc = th + (t & 1) * kLapMaxD;
        double* tn = th + ((t + 1) & 1) * kLapMaxD;
        double lt = 0.0;
        for (int m = tid; m < Nu; m += kLapThreads) {
            double f = 0.0;
            for (int j = 0; j < d; ++j) f += X(m, j) * tc[j];
            const double wm = a.w[m], ym = a.y[m];
            r[m] = wm * (ym - lap_sigmoid(f));
            if (a.loss) lt += wm * lap_loglik(ym, f);
        }
        part[tid] = lt;
        __syncthreads();
        p1 *= a.b1;
        p2 *= a.b2;
        if (tid < d) {
            double g = 0.0;
            for (int m = 0; m < Nu; ++m) g += X(m, tid) * r[m];
            g = (tj - a.mu0) * a.inv_var0 - g;
            // torch.optim.Adam: step = lr / bc1, denom = sqrt(v) / sqrt(bc2) + eps
            mj = a.b1 * mj + (1.0 - a.b1) * g;
            vj = a.b2 * vj + (1.0 - a.b2) * g * g;
            const double denom = sqrt(vj) / sqrt(1.0 - p2) + a.adam_eps;
            tj -= a.lr / (1.0 - p1) * (mj / denom);
            tn[tid] = tj;
        }
        if (a.loss && tid == kLapThreads - 1) {
            double s = 0.0;
            for (int i = 0; i < kLapThreads; ++i) s += part[i];
            for (int j = 0; j < d; ++j) {
                const double z = tc[j] - a.mu0;
                s += a.log_norm0 - 0.5 * z * z * a.inv_var0;
            }
            a.loss[t] = -s;
        }
        __syncthreads();
    }
    // diagonal precision at the fitted theta and the samples from it
    const double* tc = th + (a.T & 1) * kLapMaxD;
    for (int m = tid; m < Nu; m += kLapThreads) {
        double f = 0.0;
        for (int j = 0; j < d; ++j) f += X(m, j) * tc[j];
        const double p = lap_sigmoid(f);
        r[m] = (double)a.w[m] * p * (1.0 - p);
    }
    __syncthreads();
    if (tid < d) {
        double pr = 0.0;
        for (int m = 0; m < Nu; ++m) {
            const double xv = X(m, tid);
            pr += r[m] * xv * xv;
        }
        pr += 1.0;
        a.theta[tid] = (float)tj;
        a.prec[tid] = (float)pr;
        if (a.eps) {
            const double sd = 1.0 / sqrt(pr);
            for (int s = 0; s < a.S; ++s)
                a.samples[(size_t)s * d + tid] = (float)(tj + sd * (double)a.eps[(size_t)s * d + tid]);
        }
    }
}

hipError_t launch_laplace_fit(const LaplaceFit& r, hipStream_t st) {
    if (r.d < 1 || r.d > kLapMaxD || r.Nu < 0 || r.Nu > kLapMaxNu || r.S < 0 || r.T < 0 ||
        r.T > kLapMaxT)
        return hipErrorInvalidValue;
    LapFitArgs a{};
    a.Nu = r.Nu; a.d = r.d; a.S = r.S; a.T = r.T;
    a.ds = r.d | 1;  // odd row stride: the row owners' reads of one column spread over the banks
    a.x = r.x; a.y = r.y; a.w = r.w; a.eps = r.eps;
    a.mu0 = r.mu0;
    a.inv_var0 = 1.0 / (r.sd0 * r.sd0);
    a.log_norm0 = -std::log(r.sd0) - 0.5 * std::log(2.0 * 3.14159265358979323846);
    a.lr = r.lr; a.b1 = r.beta1; a.b2 = r.beta2; a.adam_eps = r.adam_eps;
    a.theta = r.theta; a.loss = r.loss_out; a.prec = r.prec_out; a.samples = r.samples_out;
    const bool xlds = lap_fit_xlds(r.Nu, a.ds);
    const size_t lds = lap_fit_lds(nullptr, r.Nu, a.ds, xlds).bytes;
    auto kernel = xlds ? laplace_fit_kernel<true> : laplace_fit_kernel<false>;
    if (hipError_t e = allow_dynamic_lds((const void*)kernel, kLapLds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(kLapThreads), lds, st, a);
    return hipGetLastError();
}

// Full-precision samples (laplace_precision(diagonal=False), logreg.py:95-107;
// MultivariateNormal(theta, precision_matrix=P).rsample, baselines.py:64-70):
//   P = I + sum_m w_m p_m (1 - p_m) x_m x_m^T,   p_m = sigmoid(x_m . theta)
// torch samples theta + L eps with L the lower Cholesky factor of P^-1.  With
// the "reverse" factorisation P = A^T A, A lower-triangular (eliminated from
// the last row and column upwards), L = A^-1: a sample is theta + y, A y = eps,
// one forward substitution, and L is never formed.  Every eigenvalue of P is
// >= 1 (w >= 0): no pivoting, no jitter.
// One workgroup; th, the lower triangle of P / A packed by rows (tri(i) + j,
// j <= i) and a work area are fp64 in LDS (lap_full_lds):
//   phase 1  rows:    thread t owns rows t, t + 256, ...: r_m = w_m p_m (1 - p_m) -> work
//            entries: thread t owns the packed entries t, t + 256, ...: the sum
//                     over the rows in order, x from global memory, then + I
//   phase 2  for k = d - 1 .. 0: pivot A_kk = sqrt(P_kk) | row k /= A_kk |
//            P_ji -= A_kj A_ki over the packed prefix (i <= j < k), a barrier
//            after each; thread 0 then sums log A_jj in order
//   phase 3  thread t < nb owns the samples t, t + nb, ...; its y lives in the
//            work area as y[i][t] (nb = the columns that fit, <= 256)
// Every sum has one owner and a fixed order, all in fp64; outputs are rounded
// to float once.  No atomics.
struct LapFullArgs {
    int Nu, d, S, nb;
    const float *x, *w, *theta, *eps;
    float *prec, *factor, *samples;
    double* logdet;
};

__device__ __forceinline__ int lap_tri(int i) { return i * (i + 1) / 2; }
// the row i of packed entry e: tri(i) <= e < tri(i + 1)
__device__ __forceinline__ int lap_tri_row(int e) {
    int i = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    while (lap_tri(i) > e) --i;
    while (lap_tri(i + 1) <= e) ++i;
    return i;
}

__global__ __launch_bounds__(kLapThreads) void laplace_sample_full_kernel(LapFullArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lapf_sm[];
    const int Nu = a.Nu, d = a.d, tid = threadIdx.x, ntri = lap_tri(d);
    const LapFullLds l = lap_full_lds(lapf_sm, Nu, d, a.nb);
    double *th = l.th, *P = l.P, *work = l.work;
    for (int j = tid; j < d; j += kLapThreads) th[j] = (double)a.theta[j];
    __syncthreads();
    for (int m = tid; m < Nu; m += kLapThreads) {
        const float* xm = a.x + (size_t)m * d;
        double f = 0.0;
        for (int j = 0; j < d; ++j) f += (double)xm[j] * th[j];
        const double p = lap_sigmoid(f);
        work[m] = (double)a.w[m] * p * (1.0 - p);
    }
    __syncthreads();
    for (int e = tid; e < ntri; e += kLapThreads) {
        const int i = lap_tri_row(e), j = e - lap_tri(i);
        const float *xi = a.x + i, *xj = a.x + j;
        double acc = 0.0;
#pragma unroll 8
        for (int m = 0; m < Nu; ++m)
            acc += work[m] * (double)xi[(size_t)m * d] * (double)xj[(size_t)m * d];
        P[e] = i == j ? acc + 1.0 : acc;
    }
    __syncthreads();
    if (a.prec) {
        for (int q = tid; q < d * d; q += kLapThreads) {
            const int i = q / d, j = q % d;
            a.prec[q] = (float)P[i >= j ? lap_tri(i) + j : lap_tri(j) + i];
        }
    }
    for (int k = d - 1; k >= 0; --k) {
        double* Ak = P + lap_tri(k);
        __syncthreads();  // the reads of P for prec_out / the previous update
        if (tid == 0) Ak[k] = sqrt(Ak[k]);
        __syncthreads();
        for (int i = tid; i < k; i += kLapThreads) Ak[i] /= Ak[k];
        __syncthreads();
        for (int e = tid; e < lap_tri(k); e += kLapThreads) {
            const int j = lap_tri_row(e), i = e - lap_tri(j);
            P[e] -= Ak[j] * Ak[i];
        }
    }
    __syncthreads();
    if (a.factor) {
        for (int q = tid; q < d * d; q += kLapThreads) {
            const int i = q / d, j = q % d;
            a.factor[q] = i >= j ? (float)P[lap_tri(i) + j] : 0.0f;
        }
    }
    if (a.logdet && tid == 0) {
        double s = 0.0;
        for (int j = 0; j < d; ++j) s += log(P[lap_tri(j) + j]);
        a.logdet[0] = 2.0 * s;
    }
    if (tid >= a.nb) return;  // no barrier below
    const int nb = a.nb;
    for (int s = tid; s < a.S; s += nb) {
        const float* es = a.eps + (size_t)s * d;
        float* out = a.samples + (size_t)s * d;
        for (int i = 0; i < d; ++i) {
            const double* Ai = P + lap_tri(i);
            double acc = (double)es[i];
            for (int j = 0; j < i; ++j) acc -= Ai[j] * work[j * nb + tid];
            const double yi = acc / Ai[i];
            work[i * nb + tid] = yi;
            out[i] = (float)(th[i] + yi);
        }
    }
}

hipError_t launch_laplace_sample_full(const LaplaceSampleFull& r, hipStream_t st) {
    if (r.d < 2 || r.d > kLapFullMaxD || r.Nu < 0 || r.Nu > kLapMaxNu || r.S < 0 ||
        r.S > kSelMaxS || (r.S > 0 && (!r.eps || !r.samples_out)))
        return hipErrorInvalidValue;
    LapFullArgs a{};
    a.Nu = r.Nu; a.d = r.d; a.S = r.S;
    a.x = r.x; a.w = r.w; a.theta = r.theta; a.eps = r.eps;
    a.prec = r.prec_out; a.factor = r.factor_out; a.samples = r.samples_out;
    a.logdet = r.logdet_out;
    a.nb = lap_full_cols(r.d, r.S);
    const size_t lds = lap_full_lds(nullptr, r.Nu, r.d, a.nb).bytes;
    if (lds > kLapLds) return hipErrorInvalidValue;
    if (hipError_t e = allow_dynamic_lds((const void*)laplace_sample_full_kernel, kLapLds);
        e != hipSuccess)
        return e;
    hipLaunchKernelGGL(laplace_sample_full_kernel, dim3(1), dim3(kLapThreads), lds, st, a);
    return hipGetLastError();
}

struct LapScoreArgs {
    int S, d, Nu, B;
    const float *samples, *rows, *labels, *w;
    double scale;
    float *corr, *corecorr, *grad_w, *ll, *grad_u;
    double* result;
};

// ll_sj as the float the sums use
__device__ __forceinline__ double lap_ll(const float* samples, const float* rows,
                                         const float* labels, int d, int s, int j) {
    const float* th = samples + (size_t)s * d;
    const float* x = rows + (size_t)j * d;
    double f = 0.0;
    for (int k = 0; k < d; ++k) f += (double)x[k] * (double)th[k];
    return (double)(float)lap_loglik((double)labels[j], f);
}
__device__ __forceinline__ double lap_ll(const LapScoreArgs& a, int s, int j) {
    return lap_ll(a.samples, a.rows, a.labels, a.d, s, j);
}

__global__ __launch_bounds__(kSelThreads) void laplace_scores_kernel(LapScoreArgs a) {
    __shared__ double mean[kLapMaxRows], resid[kSelMaxS], coef[kSelMaxS], red[kSelThreads];
    __shared__ int redi[kSelThreads];
    const int S = a.S, d = a.d, Nu = a.Nu, B = a.B, M = Nu + B, tid = threadIdx.x;
    // per column: the mean over the samples, in sample order
    for (int j = tid; j < M; j += kSelThreads) {
        double sum = 0.0;
        for (int s = 0; s < S; ++s) {
            const double l = lap_ll(a, s, j);
            if (a.ll) a.ll[(size_t)s * M + j] = (float)l;
            sum += l;
        }
        mean[j] = sum / S;
    }
    __syncthreads();
    // per sample: resid_s = scale sum_n cll_sn - sum_m w_m cll_sm, rows in order
    double rsum = 0.0;
    for (int s = tid; s < S; s += kSelThreads) {
        double core = 0.0, data = 0.0;
        for (int m = 0; m < Nu; ++m) core += (double)a.w[m] * (lap_ll(a, s, m) - mean[m]);
        for (int n = Nu; n < M; ++n) data += lap_ll(a, s, n) - mean[n];
        resid[s] = a.scale * data - core;
        rsum += resid[s];
    }
    const double rbar = tree_sum<kSelThreads>(rsum, red) / S;
    // per column: cll_.j . resid and |cll_.j|, samples in order
    double best = -INFINITY, bestc = -INFINITY;
    int besti = 0x7fffffff;
    for (int j = tid; j < M; j += kSelThreads) {
        double dot = 0.0, sq = 0.0;
        for (int s = 0; s < S; ++s) {
            const double c = lap_ll(a, s, j) - mean[j];
            dot += c * resid[s];
            sq += c * c;
        }
        if (j < Nu) {
            const double v = fabs(dot) / sqrt(sq) / S;
            a.corecorr[j] = (float)v;
            if (a.grad_w) a.grad_w[j] = (float)(-dot / S);
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
    tree_argmax_first<kSelThreads>(best, besti, red, redi);
    if (tid == 0) {
        a.result[0] = red[0];
        a.result[1] = (double)(redi[0] == 0x7fffffff ? 0 : redi[0]);
        a.result[2] = bestc;
        a.result[3] = (Nu == 0 || red[0] > bestc) ? 1.0 : 0.0;
    }
    if (!a.grad_u) return;
    // d u_function / d u_m = -(w_m / S) sum_s (resid_s - rbar) (z_m - sigmoid(f_sm)) theta_s:
    // per core row, the S coefficients to LDS, then one owner per input column
    for (int m = 0; m < Nu; ++m) {
        __syncthreads();
        const float* x = a.rows + (size_t)m * d;
        for (int s = tid; s < S; s += kSelThreads) {
            const float* th = a.samples + (size_t)s * d;
            double f = 0.0;
            for (int k = 0; k < d; ++k) f += (double)x[k] * (double)th[k];
            coef[s] = (resid[s] - rbar) * ((double)a.labels[m] - lap_sigmoid(f));
        }
        __syncthreads();
        for (int k = tid; k < d; k += kSelThreads) {
            double g = 0.0;
            for (int s = 0; s < S; ++s) g += coef[s] * (double)a.samples[(size_t)s * d + k];
            // the ones column takes no gradient
            a.grad_u[(size_t)m * d + k] = k == d - 1 ? 0.0f : (float)(-(double)a.w[m] / S * g);
        }
    }
}

hipError_t launch_laplace_scores(const LaplaceScores& r, hipStream_t st) {
    if (r.S < 2 || r.S > kSelMaxS || r.d < 1 || r.Nu < 0 || r.B < 1 || r.Nu + r.B > kLapMaxRows)
        return hipErrorInvalidValue;
    LapScoreArgs a{};
    a.S = r.S; a.d = r.d; a.Nu = r.Nu; a.B = r.B;
    a.samples = r.samples; a.rows = r.rows; a.labels = r.labels; a.w = r.w;
    a.scale = r.sum_scaling;
    a.corr = r.corr; a.corecorr = r.corecorr; a.grad_w = r.grad_w; a.ll = r.ll_out;
    a.grad_u = r.grad_u; a.result = r.result;
    hipLaunchKernelGGL(laplace_scores_kernel, dim3(1), dim3(kSelThreads), 0, st, a);
    return hipGetLastError();
}

struct GigaArgs {
    int S, d, N;
    const float *samples, *rows, *labels, *lw;
    float *score, *lw_out, *ll;
    double* result;
};

// One geodesic-ascent step of GIGA in one workgroup.  A thread owns whole
// columns (data rows: n = tid, tid + 512, ...) or whole samples (s = tid, ...);
// the vectors over the samples meet in the fixed trees of block_reduce.hpp.
//   columns: mean_n, 1 / max(|cll_.n|, 1e-12), ell_n . lw            -> LDS
//   samples: sum_lls_s -> L, ell, zeta1, d = normalize(ell - zeta1 lw) -> LDS
//   columns: score_n = d . normalize(ell_n - (ell_n . lw) lw), first argmax n*
//   samples: ell* = ell_n*, zeta0, zeta2, gamma, lw_out, scale
__global__ __launch_bounds__(kSelThreads) void giga_step_kernel(GigaArgs a) {
    extern __shared__ __attribute__((aligned(16))) double giga_sm[];
    __shared__ double red[kSelThreads];
    __shared__ int redi[kSelThreads];
    const int S = a.S, d = a.d, N = a.N, tid = threadIdx.x;
    const GigaLds l = giga_lds(giga_sm, N, S);
    double *mean = l.mean, *inv = l.inv, *b = l.b, *ell = l.ell, *dd = l.dd;
    auto LL = [&](int s, int n) { return lap_ll(a.samples, a.rows, a.labels, d, s, n); };
    for (int n = tid; n < N; n += kSelThreads) {
        double sum = 0.0;
        for (int s = 0; s < S; ++s) {
            const double l = LL(s, n);
            if (a.ll) a.ll[(size_t)s * N + n] = (float)l;
            sum += l;
        }
        const double m = sum / S;
        double sq = 0.0, dot = 0.0;
        for (int s = 0; s < S; ++s) {
            const double c = LL(s, n) - m;
            sq += c * c;
            dot += c * (double)a.lw[s];
        }
        mean[n] = m;
        inv[n] = 1.0 / fmax(sqrt(sq), 1e-12);
        b[n] = dot * inv[n];
    }
    __syncthreads();
    double sq = 0.0;
    for (int s = tid; s < S; s += kSelThreads) {
        double sum = 0.0;
        for (int n = 0; n < N; ++n) sum += LL(s, n) - mean[n];
        ell[s] = sum;
        sq += sum * sum;
    }
    const double L = sqrt(tree_sum<kSelThreads>(sq, red));
    double z1 = 0.0;
    for (int s = tid; s < S; s += kSelThreads) {
        ell[s] /= fmax(L, 1e-12);
        z1 += ell[s] * (double)a.lw[s];
    }
    z1 = tree_sum<kSelThreads>(z1, red);
    sq = 0.0;
    for (int s = tid; s < S; s += kSelThreads) {
        dd[s] = ell[s] - z1 * (double)a.lw[s];
        sq += dd[s] * dd[s];
    }
    const double dnorm = fmax(sqrt(tree_sum<kSelThreads>(sq, red)), 1e-12);
    for (int s = tid; s < S; s += kSelThreads) dd[s] /= dnorm;
    __syncthreads();
    double best = -INFINITY;
    int besti = 0x7fffffff;
    for (int n = tid; n < N; n += kSelThreads) {
        double num = 0.0, vsq = 0.0;
        for (int s = 0; s < S; ++s) {
            const double v = (LL(s, n) - mean[n]) * inv[n] - b[n] * (double)a.lw[s];
            num += v * dd[s];
            vsq += v * v;
        }
        const double v = num / fmax(sqrt(vsq), 1e-12);
        a.score[n] = (float)v;
        if (v > best) {  // columns ascending per thread: the first of equal values stays
            best = v;
            besti = n;
        }
    }
    tree_argmax_first<kSelThreads>(best, besti, red, redi);
    const double smax = red[0];
    const int ns = redi[0] == 0x7fffffff ? 0 : redi[0];
    // every thread is past its reads of d (the barriers of the argmax): dd takes ell*
    double z0 = 0.0, z2 = 0.0;
    for (int s = tid; s < S; s += kSelThreads) {
        dd[s] = (LL(s, ns) - mean[ns]) * inv[ns];
        z0 += ell[s] * dd[s];
        z2 += dd[s] * (double)a.lw[s];
    }
    z0 = tree_sum<kSelThreads>(z0, red);
    z2 = tree_sum<kSelThreads>(z2, red);
    const double gamma = (z0 - z1 * z2) / (z0 - z1 * z2 + z1 - z0 * z2);
    sq = 0.0;
    for (int s = tid; s < S; s += kSelThreads) {
        ell[s] = (1.0 - gamma) * (double)a.lw[s] + gamma * dd[s];
        sq += ell[s] * ell[s];
    }
    const double tnorm = fmax(sqrt(tree_sum<kSelThreads>(sq, red)), 1e-12);
    // the reference scales the weights by the norm taken with the NEW lw
    // (baselines.py:405-413: lw is reassigned before the norm is formed)
    sq = 0.0;
    for (int s = tid; s < S; s += kSelThreads) {
        const double l = ell[s] / tnorm;
        a.lw_out[s] = (float)l;
        const double u = (1.0 - gamma) * l + gamma * dd[s];
        sq += u * u;
    }
    const double unorm = sqrt(tree_sum<kSelThreads>(sq, red));
    if (tid == 0) {
        a.result[0] = smax;
        a.result[1] = (double)ns;
        a.result[2] = z0;
        a.result[3] = z1;
        a.result[4] = z2;
        a.result[5] = gamma;
        a.result[6] = 1.0 / unorm;
        a.result[7] = L;
    }
}

hipError_t launch_giga_step(const GigaStep& r, hipStream_t st) {
    if (r.S < 2 || r.S > kSelMaxS || r.d < 2 || r.d > kLapMaxD || r.n_data < 1 ||
        r.n_data > kLapMaxRows)
        return hipErrorInvalidValue;
    GigaArgs a{};
    a.S = r.S; a.d = r.d; a.N = r.n_data;
    a.samples = r.samples; a.rows = r.rows; a.labels = r.labels; a.lw = r.lw_in;
    a.score = r.score; a.lw_out = r.lw_out; a.ll = r.ll_out; a.result = r.result;
    // above the 64 KiB a launch gets unasked at the range's far corner
    const size_t max_lds = giga_lds(nullptr, kLapMaxRows, kSelMaxS).bytes;
    if (hipError_t e = allow_dynamic_lds((const void*)giga_step_kernel, max_lds); e != hipSuccess)
        return e;
    const size_t lds = giga_lds(nullptr, r.n_data, r.S).bytes;
    hipLaunchKernelGGL(giga_step_kernel, dim3(1), dim3(kSelThreads), lds, st, a);
    return hipGetLastError();
}

}  // namespace psvi
