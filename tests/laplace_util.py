"""fp64 torch restatement of the Laplace coreset baselines' core (reference
psvi/inference/baselines.py:35-70, 550-575, 617-635, 783-805 and
psvi/models/logreg.py:17-26, 95-107): the fit as Adam steps written out, the
diagonal precision and the samples, the centred log-likelihood scores, the
weight gradient, and opsvi's pseudo-input gradient by autograd.  Pinned to the
reference-generated fixtures q1-q3 by tests/test_laplace_cpu.py; the GPU tests
compare the kernels with it.  Rows are ordered core first, ll is [S][rows]."""
import math

import numpy as np
import torch


def t64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def loglik(f, y):
    """y f - softplus(f) = -BCEWithLogits for any float label, in its
    arrangement: a saturated logit on the label's side keeps its tiny term."""
    return -((1 - y) * f + torch.clamp(-f, min=0) + torch.log1p(torch.exp(-f.abs())))


def neg_log_joint(theta, x, y, w, mu0=0.0, sd0=1.0):
    prior = (-0.5 * ((theta - mu0) / sd0) ** 2 - math.log(sd0)
             - 0.5 * math.log(2 * math.pi)).sum()
    return -(w * loglik(x @ theta, y)).sum() - prior


def fit(theta0, x, y, w, T, lr, mu0=0.0, sd0=1.0, betas=(0.9, 0.999), eps=1e-8):
    """T steps of torch.optim.Adam (single-tensor arithmetic) from zero
    moments: (theta, losses before each step)."""
    th = theta0.clone()
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    losses = []
    for t in range(1, T + 1):
        f = x @ th
        losses.append(float(neg_log_joint(th, x, y, w, mu0, sd0)))
        g = -x.T @ (w * (y - torch.sigmoid(f))) + (th - mu0) / sd0 ** 2
        m = betas[0] * m + (1 - betas[0]) * g
        v = betas[1] * v + (1 - betas[1]) * g * g
        bc1, bc2 = 1 - betas[0] ** t, 1 - betas[1] ** t
        th = th - lr / bc1 * (m / (v.sqrt() / math.sqrt(bc2) + eps))
    return th, torch.tensor(losses, dtype=torch.float64)


def precision(theta, x, w):
    p = torch.sigmoid(x @ theta)
    return 1.0 + ((w * p * (1 - p))[:, None] * x ** 2).sum(0)


def samples(theta, prec, eps):
    return theta + prec ** -0.5 * eps


def ll_matrix(smp, rows, labels):
    """[S][rows]."""
    return loglik(smp @ rows.T, labels[None, :])


def scores(ll, w, n_core, sum_scaling):
    """(corr, corecorr, resid, grad_w) from ll [S][n_core + n_data]."""
    S = ll.shape[0]
    cll = ll - ll.mean(0, keepdim=True)
    core, data = cll[:, :n_core], cll[:, n_core:]
    resid = sum_scaling * data.sum(1) - core @ w
    corr = (data.T @ resid) / (data ** 2).sum(0).sqrt() / S
    corecorr = (core.T @ resid).abs() / (core ** 2).sum(0).sqrt() / S
    return corr, corecorr, resid, -(core.T @ resid) / S


def grad_u(smp, u, z, w, resid):
    """Autograd of u_function = -(1 / S) sum_s resid_s sum_m w_m cll_sm with
    respect to the core rows at constant resid, last column zeroed."""
    uu = u.clone().requires_grad_(True)
    ll = ll_matrix(smp, uu, z)
    cll = ll - ll.mean(0, keepdim=True)
    fn = ((cll @ -w) @ resid.detach()) / smp.shape[0]
    (g,) = torch.autograd.grad(fn, uu)
    g[:, -1] = 0
    return g


def grad_u_closed(smp, u, z, w, resid):
    """The closed form the kernel evaluates."""
    S = smp.shape[0]
    a = (resid - resid.mean())[:, None] * (z[None, :] - torch.sigmoid(smp @ u.T))   # [S][Nu]
    g = -(w[:, None] / S) * (a.T @ smp)
    g[:, -1] = 0
    return g
