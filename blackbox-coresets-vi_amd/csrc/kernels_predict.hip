// kernels_predict.hip -- the scoring pass of the MFVI data-selection baselines:
// a forward pass of the S-sample mean-field categorical net over n_rows rows,
// the logits averaged over the samples BEFORE the softmax, and every score of
// the reference's ScoreSelection / MeanFieldVI read off that one probability
// vector in the same launch.
//
// Reference:
//   MeanFieldVI.test / after_epoch        psvi/inference/utils.py:342-387
//   ScoreSelection._get_uncertainty_score psvi/inference/utils.py:992-1084
//   VILinear.forward                      psvi/models/neural_net.py:101-108
//
// The reference draws fresh weights for every minibatch of an unshuffled
// loader: rows [k rpd, (k + 1) rpd) share eps block k (psvi_elbo_grad's layout,
// [EPS_COUNT] floats per block).  A work item is (eps block k, group of at most
// RG rows of it); a workgroup takes items blockIdx.x, blockIdx.x + gridDim.x,
// ... and, per item (DESIGN §4 "MFVI selection"):
//   stage the group's rows in LDS; for s = 0 .. S - 1, layer by layer and in
//   tiles of `ut` output units: form W_s = mu + softplus(rho) eps_s of the tile
//   in LDS (softplus(rho) comes from a one-off pass into plan scratch), then
//   one thread per (row, four units) runs the dot products over the tile (the
//   row's input read once per four units; the W rows are wave-uniform LDS
//   broadcasts).  The head adds into the group's [row][C] logit sums in LDS:
//   [S][n_rows][C] logits never reach global memory.
//   Then one thread per row: mean logit, first argmax, softmax, the scores and
//   the forgetting update -- the only writer of every per-row output.
// Sums: the dot products run over the inputs in ascending order from the bias,
// the mean over s in ascending s, both fp32; the statistics (correct count,
// sum of -log p[z]) are doubles: a fixed tree per item, the items of a
// workgroup in their order, the workgroups' partials by a last one-workgroup
// kernel (thread t sums partials t, t + 256, ... in order, then the same
// tree).  No atomics; two runs give the same bits.
#include "lds_layout.hpp"

namespace psvi {

struct PredArgs {
    int L, S, C, D, RG, wcap, hs, xs;
    int din[kMaxL], dout[kMaxL], woff[kMaxL], ut[kMaxL];
    int64_t n_rows, rpd, n_items, gpb, eps_count;
    const float *x, *eps, *params, *sig;
    const int32_t* z;
    float *mean_logits, *least_conf, *entropy, *el2n, *correct;
    float *last_acc, *forgetting, *never_learnt;
    double* part;  // [gridDim.x][2], null without stats
};

// softplus(rho) of every element, in weight-space order ([n_tot])
__global__ __launch_bounds__(256) void predict_sigma_kernel(PredArgs a, float* sig) {
    for (int l = 0; l < a.L; ++l) {
        const int n = a.din[l] * a.dout[l] + a.dout[l];
        const float* rho = a.params + 2 * (size_t)a.woff[l] + n;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
            sig[a.woff[l] + i] = softplus_f(rho[i]);
    }
}

__global__ __launch_bounds__(kPredThreads) void predict_scores_kernel(PredArgs a) {
    extern __shared__ __attribute__((aligned(16))) double pred_sm[];
    const int tid = threadIdx.x, NT = kPredThreads;
    const int L = a.L, S = a.S, C = a.C, D = a.D, RG = a.RG, hs = a.hs, xs = a.xs;
    const PredLds sh = pred_lds(pred_sm, RG, a.wcap, xs, hs, C);
    double* red = sh.red;
    float *Wt = sh.Wt, *xin = sh.xin, *hA = sh.hA, *hB = sh.hB, *lg = sh.lg;
    const float Sf = (float)S;
    double tot_c = 0.0, tot_n = 0.0;  // thread 0: this workgroup's statistics
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t k = item / a.gpb;
        const int g = (int)(item - k * a.gpb);
        const int64_t r0 = k * a.rpd + (int64_t)g * RG;
        const int64_t rend = min((k + 1) * a.rpd, a.n_rows);
        if (r0 >= rend) continue;  // the last block's empty groups (the same for every thread)
        const int rg = (int)min((int64_t)RG, rend - r0);
        {
            const float* xg = a.x + (size_t)r0 * D;
            for (int i = tid; i < rg * D; i += NT) {
                const int r = i / D;
                xin[r * xs + (i - r * D)] = xg[i];
            }
        }
        const float* eg = a.eps + (size_t)k * a.eps_count;
        for (int s = 0; s < S; ++s) {
            const float* in = xin;
            int is = xs;
            float* out = hA;
            for (int l = 0; l < L; ++l) {
                const int din = a.din[l], dout = a.dout[l], nw = din * dout;
                const float* mu = a.params + 2 * (size_t)a.woff[l];
                const float* sg = a.sig + a.woff[l];
                const float* ew = eg + (size_t)S * a.woff[l] + (size_t)s * nw;
                const float* ebias = eg + (size_t)S * a.woff[l] + (size_t)S * nw + (size_t)s * dout;
                const bool head = l == L - 1;
                for (int j0 = 0; j0 < dout; j0 += a.ut[l]) {
                    const int u = min(a.ut[l], dout - j0);
                    // the last tile's readers are done with Wt; the rows / the previous
                    // layer's activations are written
                    __syncthreads();
                    for (int idx = tid; idx < u * din; idx += NT) {
                        const int e = j0 * din + idx;
                        Wt[idx] = fmaf(sg[e], ew[e], mu[e]);
                    }
                    for (int idx = tid; idx < u; idx += NT) {
                        const int e = nw + j0 + idx;
                        Wt[u * din + idx] = fmaf(sg[e], ebias[j0 + idx], mu[e]);
                    }
                    __syncthreads();
                    const int nq = (u + 3) >> 2;
                    for (int it = tid; it < rg * nq; it += NT) {
                        const int q = it / rg, r = it - q * rg, j = 4 * q;
                        // units past the tile repeat its last one and are not stored
                        const int j1 = min(j + 1, u - 1), j2 = min(j + 2, u - 1), j3 = min(j + 3, u - 1);
                        const float *w0 = Wt + j * din, *w1 = Wt + j1 * din, *w2 = Wt + j2 * din,
                                    *w3 = Wt + j3 * din;
                        const float* xr = in + (size_t)r * is;
                        float a0 = Wt[u * din + j], a1 = Wt[u * din + j1], a2 = Wt[u * din + j2],
                              a3 = Wt[u * din + j3];
                        // unrolled for the loads only: every sum keeps its order
#pragma unroll 4
                        for (int i = 0; i < din; ++i) {
                            const float xv = xr[i];
                            a0 = fmaf(w0[i], xv, a0);
                            a1 = fmaf(w1[i], xv, a1);
                            a2 = fmaf(w2[i], xv, a2);
                            a3 = fmaf(w3[i], xv, a3);
                        }
                        if (head) {
                            float* o = lg + r * C + j0 + j;
                            if (s == 0) {
                                o[0] = a0;
                                if (j + 1 < u) o[1] = a1;
                                if (j + 2 < u) o[2] = a2;
                                if (j + 3 < u) o[3] = a3;
                            } else {
                                o[0] += a0;
                                if (j + 1 < u) o[1] += a1;
                                if (j + 2 < u) o[2] += a2;
                                if (j + 3 < u) o[3] += a3;
                            }
                        } else {
                            float* o = out + r * hs + j0 + j;
                            o[0] = fmaxf(a0, 0.f);
                            if (j + 1 < u) o[1] = fmaxf(a1, 0.f);
                            if (j + 2 < u) o[2] = fmaxf(a2, 0.f);
                            if (j + 3 < u) o[3] = fmaxf(a3, 0.f);
                        }
                    }
                }
                in = out;
                is = hs;
                out = out == hA ? hB : hA;
            }
        }
        __syncthreads();
        double dc = 0.0, dn = 0.0;
        for (int r = tid; r < rg; r += NT) {
            const int64_t row = r0 + r;
            const float* lr = lg + r * C;
            const int zz = a.z ? a.z[row] : -1;
            // the mean logit as torch takes it (sum / S); the first of equal maxima
            float mx = lr[0] / Sf;
            int am = 0;
            for (int c = 1; c < C; ++c) {
                const float v = lr[c] / Sf;
                if (v > mx) {
                    mx = v;
                    am = c;
                }
            }
            float sum = 0.f;
            for (int c = 0; c < C; ++c) sum += expf(lr[c] / Sf - mx);
            float pmax = 0.f, ent = 0.f, e2 = 0.f, lpz = 0.f;
            for (int c = 0; c < C; ++c) {
                const float v = lr[c] / Sf;
                const float p = expf(v - mx) / sum;
                pmax = fmaxf(pmax, p);
                ent -= p * logf(p + 1e-20f);
                const float d = p - (c == zz ? 1.f : 0.f);
                e2 = fmaf(d, d, e2);
                if (c == zz) lpz = (v - mx) - logf(sum);
                if (a.mean_logits) a.mean_logits[(size_t)row * C + c] = v;
            }
            const float cj = am == zz ? 1.f : 0.f;
            if (a.least_conf) a.least_conf[row] = 1.f - pmax;
            if (a.entropy) a.entropy[row] = ent;
            if (a.el2n) a.el2n[row] = sqrtf(e2);
            if (a.correct) a.correct[row] = cj;
            if (a.last_acc) {
                // MeanFieldVI.after_epoch, in its order
                if (a.last_acc[row] > cj) a.forgetting[row] += 1.f;
                a.last_acc[row] = cj;
                a.never_learnt[row] = fminf(a.never_learnt[row], 1.f - cj);
            }
            dc += (double)cj;
            dn -= (double)lpz;
        }
        if (a.part) {
            tree_sum<NT>({dc, dn}, red);
            if (tid == 0) {
                tot_c += red[0];
                tot_n += red[NT];
            }
        }
    }
    if (a.part && tid == 0) {
        a.part[2 * (size_t)blockIdx.x] = tot_c;
        a.part[2 * (size_t)blockIdx.x + 1] = tot_n;
    }
}

// stats[0 .. 1] <- the nb workgroups' partials: thread t sums t, t + 256, ... in
// order, then a fixed tree over the threads
__global__ __launch_bounds__(kPredThreads) void predict_stats_kernel(const double* part, int nb,
                                                                     double* stats) {
    __shared__ double red[2 * kPredThreads];
    const int tid = threadIdx.x;
    double c = 0.0, n = 0.0;
    for (int b = tid; b < nb; b += kPredThreads) {
        c += part[2 * b];
        n += part[2 * b + 1];
    }
    tree_sum<kPredThreads>({c, n}, red);
    if (tid == 0) {
        stats[0] = red[0];
        stats[1] = red[kPredThreads];
    }
}

hipError_t launch_predict_scores(const psvi_plan& p, const PredictScores& r, hipStream_t st) {
    const PredictShape& s = r.shape;
    if (s.RG < 1 || s.wcap < 1 || r.n_rows < 1 || r.rpd < 1 || !p.pred_scratch.dev ||
        pred_lds_bytes(s, s.RG, s.wcap) > kPredLds)
        return hipErrorInvalidValue;
    PredArgs a{};
    a.L = s.L; a.S = s.S; a.C = s.C; a.D = s.D; a.RG = s.RG; a.wcap = s.wcap; a.hs = s.hs; a.xs = s.xs;
    for (int l = 0; l < s.L; ++l) {
        a.din[l] = p.lay[l].din;
        a.dout[l] = p.lay[l].dout;
        a.woff[l] = p.lay[l].woff;
        a.ut[l] = s.ut[l];
    }
    a.n_rows = r.n_rows;
    a.rpd = r.rpd;
    a.gpb = (r.rpd + s.RG - 1) / s.RG;
    a.n_items = ((r.n_rows + r.rpd - 1) / r.rpd) * a.gpb;
    a.eps_count = s.eps_count;
    float* sig = (float*)p.pred_scratch.dev + 4 * (size_t)kPredMaxGrid;  // behind the partials
    a.x = r.x; a.eps = r.eps; a.params = r.params; a.sig = sig; a.z = r.z;
    a.mean_logits = r.mean_logits; a.least_conf = r.least_conf; a.entropy = r.entropy;
    a.el2n = r.el2n; a.correct = r.correct;
    a.last_acc = r.last_acc; a.forgetting = r.forgetting; a.never_learnt = r.never_learnt;
    a.part = r.stats_out ? (double*)p.pred_scratch.dev : nullptr;
    if (hipError_t e = allow_dynamic_lds((const void*)predict_scores_kernel, kPredLds);
        e != hipSuccess)
        return e;
    const int grid = (int)std::min<int64_t>(a.n_items, kPredMaxGrid);
    hipLaunchKernelGGL(predict_sigma_kernel, dim3(std::min(64, (s.n_tot + 255) / 256)), dim3(256), 0,
                       st, a, sig);
    hipLaunchKernelGGL(predict_scores_kernel, dim3(grid), dim3(kPredThreads),
                       pred_lds_bytes(s, s.RG, s.wcap), st, a);
    if (r.stats_out)
        hipLaunchKernelGGL(predict_stats_kernel, dim3(1), dim3(kPredThreads), 0, st,
                           (const double*)p.pred_scratch.dev, grid, r.stats_out);
    return hipGetLastError();
}

}  // namespace psvi
