// kernels_mf.hip -- mean-field (VILinear) KL + gradient assembly + Adam, the
// generic fused Adam, and the Philox normal generator.
//
// Reference (/root/reference):
//   VIMixin.kl              psvi/models/neural_net.py:101-108 (-> torch
//                           _kl_normal_normal: 0.5(vr + t1 - 1 - log vr))
//   softplus sigma          neural_net.py:133-135, 150-153
//   DifferentiableAdam      psvi/robust_higher/optim.py:299-367
//   hypergrad adam_step     psvi/hypergrad/diff_optimizers.py:184-213
// Gradient: d mu = sum_s dW_s + mu/s0^2,
//   d rho = (sum_s dW_s*eps_s + sp/s0^2 - 1/sp) * sigmoid(rho).
#include <cstdio>
#include <cstdlib>

#include "mvn_common.hpp"  // diag_grad: the mean / sd gradient arithmetic shared with the full-cov head

namespace psvi {

// The shortest decimal that rounds to f (what Python's repr shows): the
// hyperparameters reach the ABI as floats, but the reference forms 1 - beta
// and the bias corrections 1 - beta^t from the Python doubles (0.999, not
// 0.999f = 0.99900001287): 1.f - 0.999f = 0.00099998713 would put a 1.3e-5
// relative error on every (1 - beta2) g^2 term of the second moment.
static double decimal_of(float f) {
    char buf[40];
    for (int digits = 6; digits <= 9; ++digits) {
        std::snprintf(buf, sizeof buf, "%.*g", digits, (double)f);
        const double d = std::strtod(buf, nullptr);
        if ((float)d == f) return d;
    }
    return (double)f;
}

AdamC make_adam(const psvi_adam_hp* hp) {
    AdamC a{};
    const double b1 = decimal_of(hp->beta1), b2 = decimal_of(hp->beta2), lr = decimal_of(hp->lr);
    a.lr = hp->lr;
    a.b1 = hp->beta1;
    a.b2 = hp->beta2;
    a.eps = hp->eps;
    a.omb1 = (float)(1.0 - b1);
    a.omb2 = (float)(1.0 - b2);
    const double bc1 = 1.0 - std::pow(b1, (double)hp->step);
    const double bc2 = 1.0 - std::pow(b2, (double)hp->step);
    a.inv_bc1 = (float)(1.0 / bc1);
    a.inv_sqrt_bc2 = (float)(1.0 / std::sqrt(bc2));
    a.lr_bc1 = (float)(lr / bc1);
    a.inv_bc2 = (float)(1.0 / bc2);
    a.kind = hp->kind;
    return a;
}

struct MfUpdArgs {
    int L;
    int woff[kMaxL + 1];
    int64_t poff[kMaxL];
    int n[kMaxL];
    const float* acc;   // [sum_s dW (n_tot) | sum_s dW*eps (n_tot)]
    int n_tot;
    float* params;
    float* m;
    float* v;
    float* grad_out;
    double* kl_out;
    int include_kl;
    unsigned kl_mask;  // layers carrying a KL term (LeNet: the VILinear layers only)
    float inv_s0sq, log_s0;
    AdamC adam;
    // SLOTS: acc from the plan's gradient slots [S_loc][nz][n_tot] and the
    // step's eps (layer l: weights [S_total][nw], then biases [S_total][dout])
    const float* slots;
    const float* seps;
    int S_loc, nz, s_goff, S_total;
    int64_t eoff[kMaxL];
    int nw[kMaxL], dout[kMaxL];
};

// Fixed-order slot sums for parameter e (layer l, element idx) over the samples
// s = s0, s0 + sstep, ...: g = sum_s sum_c slot[s][c][e], ge = sum_s (sum_c
// slot[s][c][e]) eps_s[idx] -- the net kernel's per-(sample, chunk) gradients
// (VIMixin sampling, neural_net.py:155-162: d mu = sum_s dW_s, d rho via
// sum_s dW_s eps_s).
__device__ __forceinline__ void mf_slot_sums(const MfUpdArgs& a, int l, int idx, int e, int s0,
                                             int sstep, float& g, float& ge) {
    const int nw = a.nw[l];
    const bool wt = idx < nw;
    const float* ep = a.seps + a.eoff[l] + (wt ? idx : (int64_t)a.S_total * nw + (idx - nw));
    const int64_t es = wt ? nw : a.dout[l];
    const size_t ss = (size_t)a.nz * a.n_tot;
    // two samples x the first kC chunks per round as unconditional loads at
    // clamped indices (all in flight together); the sums run in the order
    // s, then c = 0, 1, ... whatever the unroll
    constexpr int kC = 4;
    const int ncl = a.nz < kC ? a.nz : kC;
    g = 0.f;
    ge = 0.f;
    for (int s = s0; s < a.S_loc; s += 2 * sstep) {
        const int sb = s + sstep < a.S_loc ? s + sstep : s;
        float v[2][kC], ev[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int su = u ? sb : s;
            const float* q = a.slots + (size_t)su * ss + e;
#pragma unroll
            for (int c = 0; c < kC; ++c) v[u][c] = q[(size_t)min(c, a.nz - 1) * a.n_tot];
            ev[u] = ep[(int64_t)(a.s_goff + su) * es];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u && s + sstep >= a.S_loc) break;
            const float* q = a.slots + (size_t)(u ? sb : s) * ss + e;
            float gs = 0.f;
#pragma unroll
            for (int c = 0; c < kC; ++c)
                if (c < ncl) gs += v[u][c];
            for (int c = kC; c < a.nz; ++c) gs += q[(size_t)c * a.n_tot];
            g += gs;
            ge += gs * ev[u];
        }
    }
}

constexpr int kSlotGroups = 16;  // SLOTS: 16 parameters x 16 sample groups per block

template <bool GRAD>
__device__ __forceinline__ void mf_upd(const MfUpdArgs& a, int64_t pidx, float g) {
    if (GRAD) {
        a.grad_out[pidx] = g;
    } else {
        float mm = a.m[pidx], vv = a.v[pidx];
        a.params[pidx] = adam_apply(a.adam, a.params[pidx], g, mm, vv);
        a.m[pidx] = mm;
        a.v[pidx] = vv;
    }
}

// SLOTS: thread (group q, parameter lane) sums samples s = q (mod 16); the
// group partials meet in LDS and group 0 adds them in order q = 0..15.
template <bool GRAD, bool SLOTS>
__global__ __launch_bounds__(256) void mf_update_kernel(MfUpdArgs a) {
    __shared__ float red[8];
    __shared__ float sred[SLOTS ? 2 * 256 : 1];
    const int e = SLOTS ? blockIdx.x * kSlotGroups + (threadIdx.x & (kSlotGroups - 1))
                        : blockIdx.x * blockDim.x + threadIdx.x;
    const int grp = SLOTS ? threadIdx.x / kSlotGroups : 0;
    int l = 0;
    while (l + 1 < a.L && e >= a.woff[l + 1]) ++l;
    const int idx = e - a.woff[l];
    float sg_acc = 0.f, sge_acc = 0.f;
    if (SLOTS) {
        if (e < a.n_tot) mf_slot_sums(a, l, idx, e, grp, kSlotGroups, sg_acc, sge_acc);
        sred[threadIdx.x] = sg_acc;
        sred[256 + threadIdx.x] = sge_acc;
        __syncthreads();
        if (grp == 0) {
            sg_acc = 0.f;
            sge_acc = 0.f;
            for (int q = 0; q < kSlotGroups; ++q) {
                sg_acc += sred[q * kSlotGroups + threadIdx.x];
                sge_acc += sred[256 + q * kSlotGroups + threadIdx.x];
            }
        }
    }
    float klp = 0.f;
    if (e < a.n_tot && grp == 0) {
        const int64_t pmu = a.poff[l] + idx, prho = pmu + a.n[l];
        const float mu = a.params[pmu], rho = a.params[prho];
        const bool kl = a.include_kl && ((a.kl_mask >> l) & 1u);
        float sp, gmu, grho;
        diag_grad(mu, rho, SLOTS ? sg_acc : a.acc[e], SLOTS ? sge_acc : a.acc[a.n_tot + e], kl,
                  a.inv_s0sq, sp, gmu, grho);
        if (kl) {
            // _kl_normal_normal with q = N(0, s0): 0.5(vr + mu^2/s0^2 - 1 - log vr)
            const float vr = sp * sp * a.inv_s0sq;
            klp = 0.5f * (vr + mu * mu * a.inv_s0sq - 1.f - logf(vr));
        }
        mf_upd<GRAD>(a, pmu, gmu);
        mf_upd<GRAD>(a, prho, grho);
    }
    if (a.kl_out && a.include_kl) {
        const float tot = block_sum(klp, red);
        if (threadIdx.x == 0) atomicAdd(a.kl_out, (double)tot);
    }
}

// Reverse of one Adam step (nested trainer: reverse-mode through the unrolled
// inner loop, psvi_classes.py:549-560 differentiated by psvi_elbo.backward()).
// Forward (either variant, adam_apply):  m' = b1 m + (1-b1) g,
//   higher:    v' = b2 v + (1-b2) g^2,          p' = p - lr/bc1 m' / (sqrt(v'+1e-8)/sqrt(bc2) + eps)
//   hypergrad: v' = b2 v + (1-b2) g^2 + 1e-12,  p' = p - lr (m'/bc1) / (sqrt(v'/bc2) + eps)
// Given the adjoints lt, lm, lv of (p', m', v') and the step's m', v', g:
//   lg <- adjoint of g;  lm <- adjoint of m;  lv <- adjoint of v
// (p's adjoint is lt + H^T lg: psvi_hvp).
// The arithmetic is double, constants included.  lg is the difference of two
// nearly equal terms wherever the step barely depends on g's size (a fresh
// state: m' ~ g, v' ~ g^2, so m'/sqrt(v') ~ sign g; step 1 of every reverse
// pass cancels to ~1e-5 of either term), and fp32 rounding of the terms, or of
// 1 - beta, then costs lg up to 1e-2 of its value.  The kernel stays bound by
// its seven fp32 streams.
struct AdamAdjC {
    double lr, b1, b2, eps, omb1, omb2;
    double inv_bc1, inv_sqrt_bc2, inv_bc2;  // 1/(1-b1^t), 1/sqrt(1-b2^t), 1/(1-b2^t)
    int kind;
};

static AdamAdjC make_adam_adjoint(const psvi_adam_hp* hp) {
    AdamAdjC a{};
    a.lr = decimal_of(hp->lr);
    a.b1 = decimal_of(hp->beta1);
    a.b2 = decimal_of(hp->beta2);
    a.eps = decimal_of(hp->eps);
    a.omb1 = 1.0 - a.b1;
    a.omb2 = 1.0 - a.b2;
    const double bc2 = 1.0 - std::pow(a.b2, (double)hp->step);
    a.inv_bc1 = 1.0 / (1.0 - std::pow(a.b1, (double)hp->step));
    a.inv_sqrt_bc2 = 1.0 / std::sqrt(bc2);
    a.inv_bc2 = 1.0 / bc2;
    a.kind = hp->kind;
    return a;
}

__global__ __launch_bounds__(256) void adam_adjoint_kernel(int64_t n, const float* lt, float* lm,
                                                           float* lv, const float* m,
                                                           const float* v, const float* g,
                                                           float* lg, AdamAdjC a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double mm = m[i], vv = v[i], t = lt[i];
    double dm, dv;
    if (a.kind == PSVI_ADAM_HIGHER) {
        const double sq = sqrt(vv + 1e-8), D = sq * a.inv_sqrt_bc2 + a.eps;
        dm = -t * a.lr * a.inv_bc1 / D;
        dv = t * a.lr * a.inv_bc1 * mm / (D * D) * (0.5 * a.inv_sqrt_bc2 / sq);
    } else {
        const double q = sqrt(vv * a.inv_bc2), D = q + a.eps;
        dm = -t * a.lr * a.inv_bc1 / D;
        dv = t * a.lr * mm * a.inv_bc1 / (D * D) * (0.5 * a.inv_bc2 / fmax(q, 1e-30));
    }
    const double lm2 = lm[i] + dm, lv2 = lv[i] + dv;
    lg[i] = (float)(lm2 * a.omb1 + lv2 * 2.0 * a.omb2 * (double)g[i]);
    lm[i] = (float)(a.b1 * lm2);
    lv[i] = (float)(a.b2 * lv2);
}

hipError_t launch_adam_adjoint(int64_t n, const float* lt, float* lm, float* lv, const float* m,
                               const float* v, const float* g, float* lg,
                               const psvi_adam_hp* hp, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const AdamAdjC a = make_adam_adjoint(hp);
    hipLaunchKernelGGL(adam_adjoint_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n,
                       lt, lm, lv, m, v, g, lg, a);
    return hipGetLastError();
}

static void mf_slot_args(const psvi_plan& p, const float* eps, MfUpdArgs& a) {
    a.L = p.L;
    for (int l = 0; l < p.L; ++l) {
        a.woff[l] = p.lay[l].woff;
        a.poff[l] = p.lay[l].poff;
        a.n[l] = p.lay[l].n;
        a.eoff[l] = p.lay[l].eoff;
        a.nw[l] = p.lay[l].din * p.lay[l].dout;
        a.dout[l] = p.lay[l].dout;
    }
    a.woff[p.L] = p.n_tot;
    a.n_tot = p.n_tot;
    a.slots = p.mf_slots.dev;
    a.seps = eps;
    a.S_loc = p.s_cnt[p.rank];
    a.nz = p.mchunks;
    a.s_goff = p.s_off[p.rank];
    a.S_total = p.d.S;
}

// acc = [sum_s dW_s | sum_s dW_s eps_s] from the slots (psvi_mf_phase_accumulate:
// the all-reduced accumulator of the sample-sharded mean-field step)
__global__ __launch_bounds__(256) void mf_slot_acc_kernel(MfUpdArgs a, float* acc) {
    __shared__ float sred[2 * 256];
    const int e = blockIdx.x * kSlotGroups + (threadIdx.x & (kSlotGroups - 1));
    const int grp = threadIdx.x / kSlotGroups;
    int l = 0;
    while (l + 1 < a.L && e >= a.woff[l + 1]) ++l;
    float g = 0.f, ge = 0.f;
    if (e < a.n_tot) mf_slot_sums(a, l, e - a.woff[l], e, grp, kSlotGroups, g, ge);
    sred[threadIdx.x] = g;
    sred[256 + threadIdx.x] = ge;
    __syncthreads();
    if (grp == 0 && e < a.n_tot) {
        g = 0.f;
        ge = 0.f;
        for (int q = 0; q < kSlotGroups; ++q) {
            g += sred[q * kSlotGroups + threadIdx.x];
            ge += sred[256 + q * kSlotGroups + threadIdx.x];
        }
        acc[e] = g;
        acc[a.n_tot + e] = ge;
    }
}

hipError_t launch_mf_slot_acc(const psvi_plan& p, const float* eps, float* acc, hipStream_t st) {
    if (!p.mf_slots.dev) return hipErrorInvalidValue;
    MfUpdArgs a{};
    mf_slot_args(p, eps, a);
    hipLaunchKernelGGL(mf_slot_acc_kernel, dim3((p.n_tot + kSlotGroups - 1) / kSlotGroups),
                       dim3(256), 0, st, a, acc);
    return hipGetLastError();
}

hipError_t launch_mf_update(const psvi_plan& p, const MfUpdate& r, hipStream_t st) {
    const bool slots = r.acc == nullptr;
    if (slots && (!p.mf_slots.dev || !r.slot_eps)) return hipErrorInvalidValue;
    MfUpdArgs a{};
    mf_slot_args(p, r.slot_eps, a);
    a.woff[p.L] = p.n_tot;
    a.acc = r.acc;
    a.n_tot = p.n_tot;
    a.params = r.params;
    a.m = r.m;
    a.v = r.v;
    a.grad_out = r.grad_out;
    a.kl_out = r.kl_out;
    a.include_kl = r.include_kl;
    a.kl_mask = p.family == PSVI_FAMILY_LENET ? 0x1Cu : 0xFFu;
    const float s0 = p.d.prior_sd;
    a.inv_s0sq = 1.f / (s0 * s0);
    a.log_s0 = logf(s0);
    if (r.hp) a.adam = make_adam(r.hp);
    const int nb = slots ? (p.n_tot + kSlotGroups - 1) / kSlotGroups : (p.n_tot + 255) / 256;
    if (r.grad_out && slots)
        hipLaunchKernelGGL((mf_update_kernel<true, true>), dim3(nb), dim3(256), 0, st, a);
    else if (r.grad_out)
        hipLaunchKernelGGL((mf_update_kernel<true, false>), dim3(nb), dim3(256), 0, st, a);
    else if (slots)
        hipLaunchKernelGGL((mf_update_kernel<false, true>), dim3(nb), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((mf_update_kernel<false, false>), dim3(nb), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------- sampled KL (sparse-BBVI)
// VIMixin.sampled_nkl (neural_net.py:110-115) of every layer, per sample, and
// the gradient of -sum_s nkl_s (the reference's elbo, psvi/inference/utils.py:
// 85-91, subtracts the per-sample term; autograd gives the sums below):
//   nkl_s = sum_i [-theta_si^2 / (2 s0^2) - log s0 + log sigma_i + eps_si^2 / 2]
//   d / d mu_i  = sum_s theta_si / s0^2
//   d / d rho_i = (sum_s theta_si eps_si / s0^2 - S / sigma_i) sigmoid(rho_i)
// theta_si = mu_i + sigma_i eps_si, sigma = softplus(rho).
struct MfNklArgs {
    int L, S, n_tot;
    int woff[kMaxL + 1];
    int64_t poff[kMaxL], eoff[kMaxL];
    int n[kMaxL], nw[kMaxL], dout[kMaxL];
    float inv_s0sq;
    double log_s0;
    const float* params;
    const float* eps;
    double* nkl;   // [S]
    float* grad;   // [P], added into
};

// eps of sample s, element idx of layer l (weights [S][nw], then biases [S][dout])
__device__ __forceinline__ float mf_eps_at(const MfNklArgs& a, int l, int s, int idx) {
    const int nw = a.nw[l];
    return idx < nw ? a.eps[a.eoff[l] + (int64_t)s * nw + idx]
                    : a.eps[a.eoff[l] + (int64_t)a.S * nw + (int64_t)s * a.dout[l] + (idx - nw)];
}

// one workgroup per sample; thread t sums elements t, t + 256, ... of every
// layer in order, the 256 partials meet in a fixed tree
__global__ __launch_bounds__(256) void mf_nkl_kernel(MfNklArgs a) {
    __shared__ double red[256];
    const int s = blockIdx.x;
    double acc = 0.0;
    for (int l = 0; l < a.L; ++l) {
        const int n = a.n[l];
        for (int i = threadIdx.x; i < n; i += 256) {
            const float e = mf_eps_at(a, l, s, i);
            const float mu = a.params[a.poff[l] + i], rho = a.params[a.poff[l] + n + i];
            const float sp = softplus_f(rho);
            const float th = mu + e * sp;
            acc += -0.5 * (double)th * th * a.inv_s0sq + (double)logf(sp) + 0.5 * (double)e * e;
        }
    }
    acc = tree_sum<256>(acc, red);
    if (threadIdx.x == 0) a.nkl[s] = acc - (double)a.n_tot * a.log_s0;
}

// one thread per element: the sums over s in sample order, one writer per slot
__global__ __launch_bounds__(256) void mf_nkl_grad_kernel(MfNklArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n_tot) return;
    int l = 0;
    while (l + 1 < a.L && e >= a.woff[l + 1]) ++l;
    const int idx = e - a.woff[l];
    const int64_t pmu = a.poff[l] + idx, prho = pmu + a.n[l];
    const float mu = a.params[pmu], rho = a.params[prho];
    const float sp = softplus_f(rho);
    double gm = 0.0, gs = 0.0;
    for (int s = 0; s < a.S; ++s) {
        const float ev = mf_eps_at(a, l, s, idx);
        const float th = mu + ev * sp;
        gm += (double)th;
        gs += (double)th * ev;
    }
    a.grad[pmu] += (float)(gm * a.inv_s0sq);
    a.grad[prho] += (float)((gs * a.inv_s0sq - (double)a.S / sp) * sigmoid_f(rho));
}

hipError_t launch_mf_sampled_kl(const psvi_plan& p, const float* eps, const float* params,
                                double* nkl_out, float* grad_out, hipStream_t st) {
    if (p.family != PSVI_FAMILY_MEANFIELD || p.world != 1) return hipErrorInvalidValue;
    MfNklArgs a{};
    a.L = p.L;
    a.S = p.d.S;
    a.n_tot = p.n_tot;
    for (int l = 0; l < p.L; ++l) {
        a.woff[l] = p.lay[l].woff;
        a.poff[l] = p.lay[l].poff;
        a.eoff[l] = p.lay[l].eoff;
        a.n[l] = p.lay[l].n;
        a.nw[l] = p.lay[l].din * p.lay[l].dout;
        a.dout[l] = p.lay[l].dout;
    }
    a.woff[p.L] = p.n_tot;
    const double s0 = p.d.prior_sd;
    a.inv_s0sq = (float)(1.0 / (s0 * s0));
    a.log_s0 = std::log(s0);
    a.params = params;
    a.eps = eps;
    a.nkl = nkl_out;
    a.grad = grad_out;
    if (nkl_out) hipLaunchKernelGGL(mf_nkl_kernel, dim3(p.d.S), dim3(256), 0, st, a);
    if (grad_out)
        hipLaunchKernelGGL(mf_nkl_grad_kernel, dim3((p.n_tot + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------------ generic Adam
__global__ __launch_bounds__(256) void adam_kernel(int64_t n, float* __restrict__ p,
                                                   const float* __restrict__ g,
                                                   float* __restrict__ m,
                                                   float* __restrict__ v, AdamC a) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        float mm = m[i], vv = v[i];
        p[i] = adam_apply(a, p[i], g[i], mm, vv);
        m[i] = mm;
        v[i] = vv;
    }
}

hipError_t launch_adam(int64_t n, float* p, const float* g, float* m, float* v,
                       const psvi_adam_hp* hp, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int64_t nb = std::min<int64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)nb), dim3(256), 0, st, n, p, g, m, v,
                       make_adam(hp));
    return hipGetLastError();
}

// ----------------------------------------------------- Philox4x32-10 randn
// zero != nullptr: the same launch also clears zero[0, nzero) (the inner
// loop's per-step ELBO accumulators, which the first network launch adds into)
template <bool VEC>
__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, int64_t n,
                                                    uint64_t seed, uint64_t offset,
                                                    double* __restrict__ zero, int64_t nzero,
                                                    int64_t q_lo, int64_t q_hi) {
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = gid; i < nzero; i += gs) zero[i] = 0.0;
    for (int64_t q = q_lo + gid; q < q_hi; q += gs)
        randn_quad<VEC>(out, n, seed, offset, q);
}

// the same stream, also as the full-cov draw's three bf16 planes (EpsPlanes)
__global__ __launch_bounds__(256) void randn_planes_kernel(float* __restrict__ out, int64_t n,
                                                           uint64_t seed, uint64_t offset,
                                                           double* __restrict__ zero, int64_t nzero,
                                                           EpsPlanes P, uint16_t* __restrict__ planes,
                                                           int64_t q_lo, int64_t q_hi) {
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = gid; i < nzero; i += gs) zero[i] = 0.0;
    for (int64_t q = q_lo + gid; q < q_hi; q += gs) randn_quad_planes(out, n, seed, offset, q, P, planes);
}

hipError_t launch_randn(const RandnLaunch& r, hipStream_t st) {
    float* const out = r.out;
    const int64_t n = r.n;
    const uint64_t seed = r.seed, offset = r.offset;
    double* const zero = r.zero;
    if (n <= 0 && r.nzero <= 0) return hipSuccess;
    const int64_t nzero = zero ? r.nzero : 0;
    // the quads drawn: all of [0, ceil(n / 4)), or the caller's part of them
    const int64_t nqa = (std::max<int64_t>(n, 0) + 3) / 4;
    const int64_t q_hi = r.q_hi < 0 ? nqa : std::min(r.q_hi, nqa);
    const int64_t q_lo = std::max<int64_t>(r.q_lo, 0);
    if (q_hi <= q_lo && nzero <= 0) return hipSuccess;
    const int64_t nb = std::max<int64_t>(
        1, std::min<int64_t>(std::max(std::max<int64_t>(q_hi - q_lo, 0), nzero) / 256 + 1, 4096));
    if (r.planes && r.planes_desc) {
        if ((uintptr_t)out & 15) return hipErrorInvalidValue;
        hipLaunchKernelGGL(randn_planes_kernel, dim3((unsigned)nb), dim3(256), 0, st, out, n, seed,
                           offset, zero, nzero, *r.planes_desc, r.planes, q_lo, q_hi);
        return hipGetLastError();
    }
    if (((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL(randn_kernel<true>, dim3((unsigned)nb), dim3(256), 0, st, out, n, seed,
                           offset, zero, nzero, q_lo, q_hi);
    else
        hipLaunchKernelGGL(randn_kernel<false>, dim3((unsigned)nb), dim3(256), 0, st, out, n,
                           seed, offset, zero, nzero, q_lo, q_hi);
    return hipGetLastError();
}

// ------------------------------------------------- non-finite values flag
// flag[0] |= 1 when any of the n values is NaN or +-inf: the device-side check
// that stands in for torch.autograd.set_detect_anomaly (flow_psvi.py:50) on the
// HIP path; one int32 for the host to read once per outer step.
template <typename T>
__global__ __launch_bounds__(256) void nonfinite_kernel(const T* __restrict__ x, int64_t n,
                                                        int32_t* __restrict__ flag) {
    bool bad = false;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        bad |= !isfinite(x[i]);
    if (__any(bad) && (threadIdx.x & (kWave - 1)) == 0) atomicOr(flag, 1);
}

hipError_t launch_nonfinite(const void* x, int64_t n, int dtype, int32_t* flag, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int64_t nb = std::min<int64_t>((n + 255) / 256, 1024);
    if (dtype == 1)
        hipLaunchKernelGGL(nonfinite_kernel<double>, dim3((unsigned)nb), dim3(256), 0, st,
                           (const double*)x, n, flag);
    else
        hipLaunchKernelGGL(nonfinite_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st,
                           (const float*)x, n, flag);
    return hipGetLastError();
}

}  // namespace psvi
