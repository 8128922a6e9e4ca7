"""float64 restatement of the MFVI regression fit (psvi_mfvi_fit; the
reference's fit, psvi/inference/baselines.py:1283-1346) for the tests: the
Gaussian MFVI loss on a fixed batch, its hand-derived gradient and
torch.optim.Adam, T chained steps.  Parameters in parameters_to_vector order
(per layer mu_W, mu_b, rho_W, rho_b), eps in the library's layout (per layer
eps_W (S, out, in), then eps_b (S, out))."""
import math

import numpy as np


def layer_table(D, hidden, n_hidden_layers):
    dims = [D] + [hidden] * n_hidden_layers + [1]
    return [(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]


def counts(layers, S):
    n_tot = sum(i * o + o for i, o in layers)
    return 2 * n_tot, S * n_tot


def softplus(x):
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def split_params(layers, p):
    out, o = [], 0
    for i, j in layers:
        nw = i * j
        out.append((p[o:o + nw].reshape(j, i), p[o + nw:o + nw + j],
                    p[o + nw + j:o + 2 * nw + j].reshape(j, i), p[o + 2 * nw + j:o + 2 * (nw + j)]))
        o += 2 * (nw + j)
    return out


def split_eps(layers, eps, S):
    out, o = [], 0
    for i, j in layers:
        nw = i * j
        out.append((eps[o:o + S * nw].reshape(S, j, i), eps[o + S * nw:o + S * (nw + j)].reshape(S, j)))
        o += S * (nw + j)
    return out


def forward(layers, params, eps, S, x):
    """Sampled outputs f (S, B) and what the backward needs."""
    pl, el = split_params(layers, params), split_eps(layers, eps, S)
    h = np.broadcast_to(x, (S,) + x.shape)
    acts, Ws = [], []
    for l, ((mw, mb, rw, rb), (ew, ebb)) in enumerate(zip(pl, el)):
        W = mw + softplus(rw) * ew            # (S, out, in)
        b = mb + softplus(rb) * ebb           # (S, out)
        acts.append(h)
        Ws.append(W)
        a = np.einsum("sbi,sji->sbj", h, W) + b[:, None, :]
        h = np.maximum(a, 0.0) if l < len(layers) - 1 else a
    return h[..., 0], acts, Ws


def loss_grad(layers, params, eps, S, x, y, scale, tau, prior_sd=1.0):
    """loss = scale * sum_{s,b} NLL + KL and d loss / d params (float64)."""
    params = np.asarray(params, np.float64)
    eps = np.asarray(eps, np.float64)
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    f, acts, Ws = forward(layers, params, eps, S, x)
    d = f - y[None, :]
    loss = scale * np.sum(0.5 * tau * d * d + 0.5 * math.log(2.0 * math.pi / tau))
    delta = (scale * tau * d)[..., None]      # (S, B, 1)
    pl, el = split_params(layers, params), split_eps(layers, eps, S)
    grads = [None] * len(layers)
    s0sq = prior_sd * prior_sd
    for l in range(len(layers) - 1, -1, -1):
        mw, mb, rw, rb = pl[l]
        ew, ebb = el[l]
        dW = np.einsum("sbj,sbi->sji", delta, acts[l])
        db = delta.sum(1)
        if l > 0:
            delta = np.einsum("sbj,sji->sbi", delta, Ws[l]) * (acts[l] > 0.0)
        g = []
        for mu, rho, dv, e in ((mw, rw, dW, ew), (mb, rb, db, ebb)):
            sp = softplus(rho)
            sg = 1.0 / (1.0 + np.exp(-rho))
            vr = sp * sp / s0sq
            loss += np.sum(0.5 * (vr + mu * mu / s0sq - 1.0 - np.log(vr)))
            g.append((dv.sum(0) + mu / s0sq, ((dv * e).sum(0) + sp / s0sq - 1.0 / sp) * sg))
        (gmw, grw), (gmb, grb) = g
        grads[l] = np.concatenate([gmw.ravel(), gmb.ravel(), grw.ravel(), grb.ravel()])
    return float(loss), np.concatenate(grads)


def adam_torch(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v) / math.sqrt(1.0 - b2 ** step) + eps
    return p - lr / (1.0 - b1 ** step) * (m / denom), m, v


def fit(layers, S, x, y, scale, tau, params0, eps, lr, prior_sd=1.0, m0=None, v0=None, step0=0):
    """T = len(eps) chained steps; returns losses (T), params, m, v (float64)."""
    p = np.asarray(params0, np.float64).copy()
    m = np.zeros_like(p) if m0 is None else np.asarray(m0, np.float64).copy()
    v = np.zeros_like(p) if v0 is None else np.asarray(v0, np.float64).copy()
    losses = []
    for t, e in enumerate(eps):
        L, g = loss_grad(layers, p, e, S, x, y, scale, tau, prior_sd)
        losses.append(L)
        p, m, v = adam_torch(p, g, m, v, step0 + t + 1, lr)
    return np.array(losses), p, m, v


def predict(layers, params, eps, S, x, yt, tau, y_mean, y_std):
    """fit's logging step: mean prediction over the samples in original units,
    (rmse, mean log-density with scale 1 / sqrt(tau))."""
    f, _, _ = forward(layers, np.asarray(params, np.float64), np.asarray(eps, np.float64), S,
                      np.asarray(x, np.float64))
    yp = (f * y_std + y_mean).mean(0)
    yt = np.asarray(yt, np.float64)
    d = yp - yt
    ll = -0.5 * tau * d * d - 0.5 * math.log(2.0 * math.pi / tau)
    return float(np.sqrt(np.mean(d * d))), float(np.mean(ll))


def init_params(layers, init_sd, rng):
    """Parameters of the scale of nn.Linear's initialisation (the tests' own
    draw, not torch's): mu ~ U(-1/sqrt(in), 1/sqrt(in)), rho = softplus^-1(init_sd)."""
    out = []
    rho = math.log(math.expm1(init_sd))
    for i, j in layers:
        k = 1.0 / math.sqrt(i)
        out += [rng.uniform(-k, k, i * j + j), np.full(i * j + j, rho)]
    return np.concatenate(out).astype(np.float32)
