"""fp64 torch restatement of the sparse black-box VI formulas (the sampled KL
term, the selection scores, the weight objective) and of the Bernoulli
network they sit on -- the tests' reference for shapes no fixture covers, and
itself checked against the reference-generated s1-s3 fixtures
(test_sbbvi_cpu.py)."""
import torch
import torch.nn.functional as F

DT = torch.float64


def t64(a):
    return torch.as_tensor(a, dtype=DT)


def sample_weights(params, layers, eps, S):
    """Per layer (W [S, out, in], b [S, out], views) in the library's parameter
    and eps layout: [mu_W, mu_b, rho_W, rho_b] per layer; eps_W (S, out, in)
    then eps_b (S, out) per layer."""
    out, po, eo = [], 0, 0
    for din, dout in layers:
        nw, n = din * dout, din * dout + dout
        mu, rho = params[po:po + n], params[po + n:po + 2 * n]
        e = torch.cat((eps[eo:eo + S * nw].reshape(S, nw),
                       eps[eo + S * nw:eo + S * n].reshape(S, dout)), 1)   # [S, n]
        th = mu + F.softplus(rho) * e
        out.append((th[:, :nw].reshape(S, dout, din), th[:, nw:], mu, rho, e, th))
        po += 2 * n
        eo += S * n
    return out


def logits(params, layers, eps, S, x):
    """f [S, M] of the one-output ReLU stack."""
    h = x.unsqueeze(0).expand(S, -1, -1)
    ws = sample_weights(params, layers, eps, S)
    for i, (W, b, *_) in enumerate(ws):
        h = h @ W.transpose(1, 2) + b.unsqueeze(1)
        if i + 1 < len(ws):
            h = F.relu(h)
    return h.squeeze(-1)


def loglik(f, z):
    """-NLL = z f - softplus(f), elementwise."""
    return z * f - F.softplus(f)


def sampled_kl(params, layers, eps, S, s0=1.0):
    """(nkl [S], d(-sum_s nkl_s) / d params) in closed form (item 2)."""
    nkl = torch.zeros(S, dtype=DT)
    grad = torch.zeros_like(params)
    po = 0
    for (_, _, mu, rho, e, th) in sample_weights(params, layers, eps, S):
        n = mu.numel()
        sg = F.softplus(rho)
        nkl += (-th ** 2 / (2 * s0 ** 2) + sg.log() + e ** 2 / 2).sum(1) - n * torch.log(t64(s0))
        grad[po:po + n] = th.sum(0) / s0 ** 2
        grad[po + n:po + 2 * n] = ((th * e).sum(0) / s0 ** 2 - S / sg) * torch.sigmoid(rho)
        po += 2 * n
    return nkl, grad


def elbo(params, layers, eps, S, u, z, w, s0=1.0):
    """The reference's inner objective (utils.elbo) and its gradient:
    (S * sum_{s,m} w_m NLL_sm) - sum_s nkl_s -- the scalar NLL sum broadcasts
    against the (S,) sampled KL, so it counts S times."""
    nkl, gk = sampled_kl(params, layers, eps, S, s0)
    if u.shape[0] == 0:
        return -nkl.sum(), gk
    p = params.clone().requires_grad_(True)
    nll = -(loglik(logits(p, layers, eps, S, u), z) @ w).sum()
    (gn,) = torch.autograd.grad(nll, p)
    return S * nll.detach() - nkl.sum(), S * gn + gk


def scores(ll, nkl, w, Nu, scale):
    """Item 4 from ll [S, Nu + B]: W, corr [B], corecorr [Nu]."""
    W = (ll[:, :Nu] @ w + nkl).softmax(-1)
    return scores_given_weights(ll, W, w, Nu, scale)


def scores_given_weights(ll, W, w, Nu, scale):
    """Item 4 with the sample weights W [S] given (any float dtype)."""
    S = ll.shape[0]
    core, data = ll[:, :Nu], ll[:, Nu:]
    cc, cd = core * (1 - W)[:, None], data * (1 - W)[:, None]
    resid = scale * cd.sum(1) - cc @ w
    corr = (cd.T @ resid) / cd.pow(2).sum(0).sqrt() / S
    corecorr = (cc.T @ resid).abs() / cc.pow(2).sum(0).sqrt() / S
    return W, corr, corecorr


def weight_objective(ll, nkl, w, N):
    """Item 5 from ll [S, Nu + B]: (loss, d loss / d w) in closed form."""
    S, Nu = ll.shape[0], w.numel()
    B = ll.shape[1] - Nu
    c, d = -ll[:, :Nu], -ll[:, Nu:].sum(1)
    a = N / Nu * (c @ w)
    lw = -a + nkl
    W = lw.softmax(-1)
    r = N / B * d - a
    rb = (W * r).sum()
    return rb - lw.mean(), N / Nu * (c.T @ (1.0 / S - W * (1 + r - rb)))
