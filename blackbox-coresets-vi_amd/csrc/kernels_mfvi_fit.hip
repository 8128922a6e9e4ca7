// kernels_mfvi_fit.hip -- the whole fit of the MFVI regression baselines in one
// launch: T chained steps of a mean-field Gaussian-likelihood MLP on a fixed
// batch, for G independent members (one per candidate precision tau), one
// persistent workgroup per member and nothing shared between them.
//
// Reference:
//   fit                    psvi/inference/baselines.py:1283-1346 (the loss, 1308-1314;
//                          the batch is next(iter(loader)) of an unshuffled loader: fixed)
//   run_mfvi_regressor     baselines.py:1066-1169 (one fit per tau, then the chosen one)
//   VILinear / kl          psvi/models/neural_net.py:101-108, 155-179
//   make_regressor_net     neural_net.py:300-331 (Linear-ReLU ... Linear, one output)
//
// One step of member g (DESIGN §4 "MFVI regressor fit"):
//   loss = scale sum_{s,b} [tau_g / 2 (f_sb - y_b)^2 + log(2 pi / tau_g) / 2] + sum_layers KL
//   d mu = sum_s dW_s + mu / s0^2,  d rho = (sum_s dW_s eps_s + sp / s0^2 - 1 / sp) sigmoid(rho)
//   then torch.optim.Adam (adam_apply, PSVI_ADAM_TORCH) on every parameter.
// Per sample s the workgroup stages eps_s (replayed from global memory or drawn
// from psvi_randn's Philox stream: the same floats) and W_s = mu + sp eps_s in
// LDS, then walks the batch in chunks of RB rows: a forward phase per layer
// (one thread per (row, unit)), the head, and a backward phase per layer in
// which an element's owner sums its weight gradient over the chunk's rows and
// adds it (and its product with eps_s) to the element's two accumulators,
// while one thread per (row, input) forms the previous layer's delta.
// Ownership: element idx of layer l belongs to thread idx % 512 in every phase
// that touches its mu / rho / m / v / accumulators, so with the state in
// global memory no thread reads another's global write.  Every sum has one
// owner and a fixed order (samples, chunks, rows ascending); the loss meets in
// a fixed tree of doubles.  No atomics.
// Accumulation: fp32 for the network, the gradient and Adam (the arithmetic of
// the step-by-step path: net_kernel, mf_update_kernel, adam_apply); fp64 for
// the per-row NLL terms, the KL terms' sum and the bias corrections.
#include "lds_layout.hpp"

namespace psvi {

struct MfFitArgs {
    int L, B, S, T, step0, RB;
    int din[kMfFitMaxL], dout[kMfFitMaxL], woff[kMfFitMaxL], n[kMfFitMaxL];
    int n_tot, eps_count, eps_stride;
    int hs, xs;  // row strides of the activations and of the staged batch (odd)
    const float *x, *y;
    float tau[kMfFitMaxG];
    uint64_t offset[kMfFitMaxG];
    uint64_t seed;
    const float* eps;  // [G][T][eps_count], or null: Philox
    float scale, inv_s0sq;
    double b1, b2, lr;
    float b1f, b2f, omb1, omb2, adam_eps;
    float *params, *m, *v;  // [G][2 n_tot]
    double* loss;           // [G][T], nullable
    float* ws;              // [G][2 n_tot]: the accumulators of the global placement
};

// normals [a, a + len) of the stream (seed, off) into dst[0, len)
__device__ __forceinline__ void mffit_draw(float* dst, int64_t a, int len, uint64_t seed,
                                           uint64_t off) {
    const int64_t q1 = (a + len - 1) / 4;
    for (int64_t q = a / 4 + threadIdx.x; q <= q1; q += kMfFitThreads) {
        float r[4];
        randn_quad_vals(seed, off, q, r);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = 4 * q + k - a;
            if (i >= 0 && i < len) dst[i] = r[k];
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(kMfFitThreads) void mfvi_fit_kernel(MfFitArgs a) {
    extern __shared__ __attribute__((aligned(16))) double mffit_sm[];
    const int tid = threadIdx.x, g = blockIdx.x, NT = kMfFitThreads;
    const int L = a.L, B = a.B, S = a.S, n_tot = a.n_tot, hs = a.hs, RB = a.RB;
    const int P = 2 * n_tot;
    const MfFitLds sh = mffit_lds(mffit_sm, LDS, L, B, n_tot, hs, a.xs, RB);
    double* red = sh.red;
    float *Wb = sh.Wb, *eb = sh.eb, *h = sh.h, *dA = sh.dA, *dB = sh.dB;
    float *gmu = sh.gmu, *grho = sh.grho, *sp_ = sh.sp, *sm_ = sh.sm, *sv_ = sh.sv;
    const float* xb = sh.xl;
    int xs = a.xs;
    if (LDS) {
        const int D = a.din[0];
        for (int i = tid; i < B * D; i += NT) sh.xl[(i / D) * xs + i % D] = a.x[i];
    } else {
        gmu = a.ws + (size_t)g * P;
        grho = gmu + n_tot;
        sp_ = a.params + (size_t)g * P;
        sm_ = a.m + (size_t)g * P;
        sv_ = a.v + (size_t)g * P;
        xb = a.x;
        xs = a.din[0];
    }
    if (LDS) {
        // owner-mapped as every later access of the state
        for (int l = 0; l < L; ++l)
            for (int idx = tid; idx < 2 * a.n[l]; idx += NT) {
                const size_t o = 2 * (size_t)a.woff[l] + idx;
                sp_[o] = a.params[(size_t)g * P + o];
                sm_[o] = a.m[(size_t)g * P + o];
                sv_[o] = a.v[(size_t)g * P + o];
            }
    }
    const float tau = a.tau[g];
    const float dscale = a.scale * tau;  // d NLL / d f = scale tau (f - y)
    const double nll_c = 0.5 * log(2.0 * 3.14159265358979323846 / (double)tau);
    __syncthreads();
    for (int t = 0; t < a.T; ++t) {
        for (int l = 0; l < L; ++l)
            for (int idx = tid; idx < a.n[l]; idx += NT) {
                gmu[a.woff[l] + idx] = 0.f;
                grho[a.woff[l] + idx] = 0.f;
            }
        double lpart = 0.0;  // this thread's rows' NLL, then its elements' KL
        const float* eg = a.eps ? a.eps + ((size_t)g * a.T + t) * a.eps_count : nullptr;
        const uint64_t off = a.offset[g] + (uint64_t)t * a.eps_stride;
        for (int s = 0; s < S; ++s) {
            // eps_s in the library's layout: layer l holds W [S][nw], then b [S][dout]
            for (int l = 0; l < L; ++l) {
                const int nw = a.din[l] * a.dout[l], dout = a.dout[l];
                const int64_t e0 = (int64_t)S * a.woff[l];
                const int64_t aw = e0 + (int64_t)s * nw, ab = e0 + (int64_t)S * nw + (int64_t)s * dout;
                float* dst = eb + a.woff[l];
                if (eg) {
                    for (int idx = tid; idx < nw; idx += NT) dst[idx] = eg[aw + idx];
                    for (int idx = tid; idx < dout; idx += NT) dst[nw + idx] = eg[ab + idx];
                } else {
                    mffit_draw(dst, aw, nw, a.seed, off);
                    mffit_draw(dst + nw, ab, dout, a.seed, off);
                }
            }
            __syncthreads();
            for (int l = 0; l < L; ++l)
                for (int idx = tid; idx < a.n[l]; idx += NT) {
                    const size_t o = 2 * (size_t)a.woff[l] + idx;
                    const int e = a.woff[l] + idx;
                    Wb[e] = sp_[o] + softplus_f(sp_[o + a.n[l]]) * eb[e];
                }
            __syncthreads();
            for (int c0 = 0; c0 < B; c0 += RB) {
                const int rb = min(RB, B - c0);
                // forward: one thread per (row, unit), rows fastest
                for (int l = 0; l < L; ++l) {
                    const int din = a.din[l], dout = a.dout[l];
                    const float* W = Wb + a.woff[l];
                    const float* in = l == 0 ? xb + (size_t)c0 * xs : h + (size_t)(l - 1) * RB * hs;
                    const int is = l == 0 ? xs : hs;
                    float* out = h + (size_t)l * RB * hs;
                    for (int it = tid; it < rb * dout; it += NT) {
                        const int j = it / rb, r = it - j * rb;
                        const float* wj = W + j * din;
                        const float* xr = in + (size_t)r * is;
                        float acc = W[din * dout + j];
                        // unrolled for the loads only: the sum keeps its order
#pragma unroll 8
                        for (int i = 0; i < din; ++i) acc = fmaf(wj[i], xr[i], acc);
                        if (l < L - 1) {
                            out[r * hs + j] = fmaxf(acc, 0.f);
                        } else {
                            const float d = acc - a.y[c0 + r];
                            dA[r * hs] = dscale * d;
                            lpart += (double)a.scale * (0.5 * (double)tau * (double)d * (double)d + nll_c);
                        }
                    }
                    __syncthreads();
                }
                // backward: dc holds d loss / d (pre-activation) of layer l, [row][unit]
                float *dc = dA, *dp = dB;
                for (int l = L - 1; l >= 0; --l) {
                    const int din = a.din[l], dout = a.dout[l], nw = din * dout;
                    const float* W = Wb + a.woff[l];
                    const float* in = l == 0 ? xb + (size_t)c0 * xs : h + (size_t)(l - 1) * RB * hs;
                    const int is = l == 0 ? xs : hs;
                    for (int idx = tid; idx < a.n[l]; idx += NT) {
                        float gsum = 0.f;
                        if (idx < nw) {
                            const int j = idx / din, i = idx - j * din;
#pragma unroll 8
                            for (int r = 0; r < rb; ++r)
                                gsum = fmaf(dc[r * hs + j], in[(size_t)r * is + i], gsum);
                        } else {
                            const int j = idx - nw;
                            for (int r = 0; r < rb; ++r) gsum += dc[r * hs + j];
                        }
                        const int e = a.woff[l] + idx;
                        gmu[e] += gsum;
                        grho[e] = fmaf(gsum, eb[e], grho[e]);
                    }
                    if (l > 0) {
                        for (int it = tid; it < rb * din; it += NT) {
                            const int i = it / rb, r = it - i * rb;
                            float acc = 0.f;
#pragma unroll 8
                            for (int j = 0; j < dout; ++j) acc = fmaf(W[j * din + i], dc[r * hs + j], acc);
                            dp[r * hs + i] = in[(size_t)r * is + i] > 0.f ? acc : 0.f;
                        }
                    }
                    __syncthreads();
                    float* sw = dc;
                    dc = dp;
                    dp = sw;
                }
            }
        }
        // KL gradient and value, torch.optim.Adam; step number step0 + t + 1
        AdamC ad{};
        {
            const double st = (double)(a.step0 + t + 1);
            const double bc1 = 1.0 - pow(a.b1, st), bc2 = 1.0 - pow(a.b2, st);
            ad.b1 = a.b1f; ad.b2 = a.b2f; ad.omb1 = a.omb1; ad.omb2 = a.omb2; ad.eps = a.adam_eps;
            ad.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
            ad.lr_bc1 = (float)(a.lr / bc1);
            ad.kind = PSVI_ADAM_TORCH;
        }
        for (int l = 0; l < L; ++l)
            for (int idx = tid; idx < a.n[l]; idx += NT) {
                const size_t pmu = 2 * (size_t)a.woff[l] + idx, prho = pmu + a.n[l];
                const int e = a.woff[l] + idx;
                const float mu = sp_[pmu], rho = sp_[prho];
                const float sp = softplus_f(rho), sg = sigmoid_f(rho);
                float gm = gmu[e], gr = grho[e] * sg;
                gm += mu * a.inv_s0sq;
                gr += (sp * a.inv_s0sq - 1.f / sp) * sg;
                // _kl_normal_normal against N(0, s0): 0.5 (vr + mu^2 / s0^2 - 1 - log vr)
                const float vr = sp * sp * a.inv_s0sq;
                lpart += (double)(0.5f * (vr + mu * mu * a.inv_s0sq - 1.f - logf(vr)));
                float mm = sm_[pmu], vv = sv_[pmu];
                sp_[pmu] = adam_apply(ad, mu, gm, mm, vv);
                sm_[pmu] = mm;
                sv_[pmu] = vv;
                mm = sm_[prho];
                vv = sv_[prho];
                sp_[prho] = adam_apply(ad, rho, gr, mm, vv);
                sm_[prho] = mm;
                sv_[prho] = vv;
            }
        if (a.loss) {
            const double loss = tree_sum<NT>(lpart, red);
            if (tid == 0) a.loss[(size_t)g * a.T + t] = loss;
        }
        __syncthreads();
    }
    if (LDS) {
        for (int l = 0; l < L; ++l)
            for (int idx = tid; idx < 2 * a.n[l]; idx += NT) {
                const size_t o = 2 * (size_t)a.woff[l] + idx;
                a.params[(size_t)g * P + o] = sp_[o];
                a.m[(size_t)g * P + o] = sm_[o];
                a.v[(size_t)g * P + o] = sv_[o];
            }
    }
}

hipError_t launch_mfvi_fit(const MfviFit& r, hipStream_t st) {
    const MfviFitShape& s = r.shape;
    if (s.L < 2 || s.L > kMfFitMaxL || r.G < 1 || r.G > kMfFitMaxG || s.RB < 1 || r.T < 0 ||
        mffit_lds_bytes(s, s.lds, s.RB) > kMfFitLds || (!s.lds && !r.ws))
        return hipErrorInvalidValue;
    if (r.T == 0) return hipSuccess;
    MfFitArgs a{};
    a.L = s.L; a.B = s.B; a.S = s.S; a.T = r.T; a.step0 = r.step0; a.RB = s.RB;
    int wo = 0;
    for (int l = 0; l < s.L; ++l) {
        a.din[l] = r.dims[l];
        a.dout[l] = r.dims[l + 1];
        a.n[l] = a.din[l] * a.dout[l] + a.dout[l];
        a.woff[l] = wo;
        wo += a.n[l];
    }
    a.n_tot = s.n_tot;
    a.eps_count = (int)s.eps_count;
    a.eps_stride = (int)((s.eps_count + 3) / 4 * 4);
    a.hs = s.hs; a.xs = s.xs;
    a.x = r.x; a.y = r.y;
    for (int g = 0; g < r.G; ++g) {
        a.tau[g] = r.tau[g];
        a.offset[g] = r.offset ? r.offset[g] : 0;
    }
    a.seed = r.seed;
    a.eps = r.eps;
    a.scale = (float)r.scale;
    a.inv_s0sq = 1.f / (r.prior_sd * r.prior_sd);
    a.b1 = r.beta1; a.b2 = r.beta2; a.lr = r.lr;
    a.b1f = (float)r.beta1; a.b2f = (float)r.beta2;
    a.omb1 = (float)(1.0 - r.beta1); a.omb2 = (float)(1.0 - r.beta2);
    a.adam_eps = (float)r.adam_eps;
    a.params = r.params; a.m = r.m; a.v = r.v;
    a.loss = r.loss_out;
    a.ws = (float*)r.ws;
    auto kernel = s.lds ? mfvi_fit_kernel<true> : mfvi_fit_kernel<false>;
    if (hipError_t e = allow_dynamic_lds((const void*)kernel, kMfFitLds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(r.G), dim3(kMfFitThreads), mffit_lds_bytes(s, s.lds, s.RB), st, a);
    return hipGetLastError();
}

}  // namespace psvi
