"""fp64 torch restatement of the full-precision Laplace posterior (reference
psvi/models/logreg.py:95-107 with ``diagonal=False`` and
``MultivariateNormal(theta, precision_matrix=P).rsample``,
psvi/inference/baselines.py:64-70): P, the reverse Cholesky factor A (lower,
A^T A = P, so that torch's scale_tril is A^-1), the samples and log det P --
the arithmetic of psvi_laplace_sample_full written out -- and whole
``run_sparsevi`` / ``run_opsvi`` runs with ``diagonal=False`` on recorded noise
and minibatches.  Pinned to the reference-generated fixtures s1-s3 by
tests/test_laplace_full_cpu.py; the GPU tests compare the kernel with it."""
import numpy as np
import torch

import laplace_util as U

t64 = U.t64


def precision_full(theta, x, w):
    """I + x^T diag(w p (1 - p)) x."""
    p = torch.sigmoid(x @ theta)
    return torch.eye(theta.numel(), dtype=torch.float64) + (x.T * (w * p * (1 - p))) @ x


def reverse_cholesky(P):
    """The lower-triangular A with A^T A = P, eliminated from the last row and
    column upwards: pivot, scale row k, update the leading k x k block."""
    A = torch.tril(P).clone()
    for k in range(P.shape[0] - 1, -1, -1):
        A[k, k] = A[k, k].sqrt()
        A[k, :k] /= A[k, k]
        A[:k, :k] -= torch.outer(A[k, :k], A[k, :k])
    return torch.tril(A)


def samples_full(theta, A, eps):
    """theta + y_s with A y_s = eps_s, eps [S][d]."""
    return theta + torch.linalg.solve_triangular(A, eps.T, upper=False).T


def logdet(A):
    return 2.0 * A.diagonal().log().sum()


def fit_sample(theta0, x, y, w, T, lr, eps, diagonal):
    """One selection-loop fit: (theta, samples)."""
    theta, _ = U.fit(theta0, x, y, w, T, lr)
    if diagonal:
        return theta, U.samples(theta, U.precision(theta, x, w), eps)
    return theta, samples_full(theta, reverse_cholesky(precision_full(theta, x, w)), eps)


class Stream:
    """The recorded host draws, taken in order."""

    def __init__(self, flat):
        self.flat, self.o = t64(flat), 0

    def take(self, *shape):
        n = int(np.prod(shape))
        out = self.flat[self.o:self.o + n]
        assert out.numel() == n, "draw stream exhausted"
        self.o += n
        return out.reshape(shape)


def _aug(x):
    return torch.cat((t64(x), torch.ones(len(x), 1, dtype=torch.float64)), dim=1)


def run_sparsevi(f, diagonal=False):
    """baselines.py:426-648 on a fixture's data, draws and minibatches; the
    logging fit (its theta is discarded) only consumes its draws.  Returns the
    core and the weights after every epoch."""
    c = f["cfg"]
    x, y = _aug(f["x"]), t64(f["y"])
    N, d, S, B = c["N"], x.shape[1], c["S"], c["B"]
    st, batches = Stream(f["draws"]), iter(f["batches"])
    w = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    core, cores, ws = [], [], []
    for it in range(c["epochs"]):
        wc = w.detach()[core]
        if it % c["log_every"] == 0:
            st.take(d), st.take(S, d)
        sub = torch.as_tensor(next(batches))
        _, smp = fit_sample(st.take(d), x[core], y[core], wc, c["inner_it"], c["lr0net"],
                            st.take(S, d), diagonal)
        ll = U.ll_matrix(smp, torch.cat((x[core], x[sub])), torch.cat((y[core], y[sub])))
        corr, corecorr, _, _ = U.scores(ll, wc, len(core), N / B)
        if not core or corr.max() > corecorr.max():
            pt = int(sub[int(corr.argmax())])
            if pt not in core:
                core.append(pt)
        optim_w = torch.optim.Adam([w], c["lr0v"])
        theta = st.take(d)
        for _ in range(c["outer_it"]):
            wc = w.detach()[core]
            theta, smp = fit_sample(theta, x[core], y[core], wc, c["inner_it"], c["lr0net"],
                                    st.take(S, d), diagonal)
            sub = torch.as_tensor(next(batches))
            ll = U.ll_matrix(smp, torch.cat((x[core], x[sub])), torch.cat((y[core], y[sub])))
            gw = U.scores(ll, wc, len(core), N / B)[3]
            w.grad = torch.zeros_like(w)
            w.grad[core] = gw
            optim_w.step()
            with torch.no_grad():
                torch.clamp_(w, 0)
        cores.append(list(core))
        ws.append(w.detach().clone())
    assert st.o == st.flat.numel() and next(batches, None) is None
    return cores, torch.stack(ws)


def run_opsvi(f, u0, z, diagonal=False):
    """baselines.py:652-821 from the pseudo-points (u0 with the ones column, z);
    the logging fit trains the same theta and consumes its draws.  Returns the
    weights and the pseudo-inputs after every epoch."""
    c = f["cfg"]
    x, y = _aug(f["x"]), t64(f["y"])
    N, d, S, B, M = c["N"], x.shape[1], c["S"], c["B"], c["num_pseudo"]
    st, batches = Stream(f["draws"]), iter(f["batches"])
    w = (N / M * torch.ones(M, dtype=torch.float64)).requires_grad_(True)
    theta = st.take(d)
    u, z = t64(u0).clone().requires_grad_(True), t64(z)
    optim_u = torch.optim.Adam([u], c["lr0u"])
    optim_w = torch.optim.Adam([w], c["lr0v"] * N)
    ws, us = [], []
    for it in range(c["epochs"]):
        if it % c["log_every"] == 0:
            theta, _ = fit_sample(theta, u.detach(), z, w.detach(), c["inner_it"], c["lr0net"],
                                  st.take(S, d), True)
        theta, smp = fit_sample(theta, u.detach(), z, w.detach(), c["inner_it"], c["lr0net"],
                                st.take(S, d), diagonal)
        sub = torch.as_tensor(next(batches))
        ll = U.ll_matrix(smp, torch.cat((u.detach(), x[sub])), torch.cat((z, y[sub])))
        _, _, resid, gw = U.scores(ll, w.detach(), M, N / B)
        w.grad, u.grad = gw, U.grad_u(smp, u.detach(), z, w.detach(), resid)
        optim_w.step()
        optim_u.step()
        with torch.no_grad():
            torch.clamp_(w, 0)
        ws.append(w.detach().clone())
        us.append(u.detach().clone())
    assert st.o == st.flat.numel() and next(batches, None) is None
    return torch.stack(ws), torch.stack(us)
