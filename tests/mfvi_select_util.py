"""float64 restatement of psvi_predict_scores (the MFVI selection's scoring
pass; reference psvi/inference/utils.py:342-387, 992-1084) and of the
forgetting update, in numpy: parameters and eps in the library's layouts
(include/psvi_hip.h), rows [k rpd, (k + 1) rpd) on eps block k."""
import numpy as np


def param_count(layers):
    return 2 * sum(i * o + o for i, o in layers)


def eps_count(layers, S):
    return S * sum(i * o + o for i, o in layers)


def _weights(layers, params, eps, S):
    """Per layer W (S, out, in) and b (S, out) = mu + softplus(rho) eps."""
    params, eps = np.asarray(params, np.float64), np.asarray(eps, np.float64)
    out, po, eo = [], 0, 0
    for din, dout in layers:
        nw, n = din * dout, din * dout + dout
        mu, rho = params[po:po + n], params[po + n:po + 2 * n]
        sd = np.logaddexp(0.0, rho)
        e = np.concatenate((eps[eo:eo + S * nw].reshape(S, nw),
                            eps[eo + S * nw:eo + S * n].reshape(S, dout)), axis=1)
        X = mu[None] + sd[None] * e
        out.append((X[:, :nw].reshape(S, dout, din), X[:, nw:]))
        po += 2 * n
        eo += S * n
    return out


def mean_logits(layers, S, params, eps, x, rows_per_draw):
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    ec = eps_count(layers, S)
    out = np.empty((x.shape[0], layers[-1][1]))
    for k, lo in enumerate(range(0, x.shape[0], rows_per_draw)):
        h = np.broadcast_to(x[lo:lo + rows_per_draw], (S,) + x[lo:lo + rows_per_draw].shape)
        Wb = _weights(layers, params, np.asarray(eps)[k * ec:(k + 1) * ec], S)
        for l, (W, b) in enumerate(Wb):
            h = np.einsum("sri,soi->sro", h, W) + b[:, None, :]
            if l < len(Wb) - 1:
                h = np.maximum(h, 0.0)
        out[lo:lo + rows_per_draw] = h.mean(0)
    return out


def scores(ml, z=None):
    """Every output of the kernel from the mean logits ml (n, C)."""
    ml = np.asarray(ml, np.float64)
    m = ml.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(ml - m).sum(1))
    p = np.exp(ml - lse[:, None])
    out = dict(mean_logits=ml, p=p, least_conf=1.0 - p.max(1),
               entropy=-(p * np.log(p + 1e-20)).sum(1), argmax=ml.argmax(1))
    if z is not None:
        z = np.asarray(z).astype(np.int64)
        onehot = np.eye(ml.shape[1])[z]
        out["el2n"] = np.sqrt(((p - onehot) ** 2).sum(1))
        out["correct"] = (out["argmax"] == z).astype(np.float64)
        out["stats"] = np.array([out["correct"].sum(), (lse - ml[np.arange(len(z)), z]).sum()])
    return out


def top2_gap(ml):
    s = np.sort(np.asarray(ml, np.float64), axis=1)
    return s[:, -1] - s[:, -2] if s.shape[1] > 1 else np.full(len(s), np.inf)


def forgetting_update(last_acc, forgetting, never_learnt, correct):
    """MeanFieldVI.after_epoch, in its order; returns the three new vectors."""
    forgetting = forgetting + (last_acc > correct)
    return correct.copy(), forgetting, np.minimum(never_learnt, 1.0 - correct)


def class_split(num_pseudo, nc):
    per = num_pseudo // nc
    return [per] * (nc - 1) + [num_pseudo - (nc - 1) * per]


def select(score, targets, num_pseudo, nc):
    """ScoreSelection.select: the top rows per class, the remainder on the last."""
    out = []
    for c, k in enumerate(class_split(num_pseudo, nc)):
        idx = np.arange(len(targets))[np.asarray(targets) == c]
        out += idx[np.argsort(-np.asarray(score)[idx], kind="stable")[:k]].tolist()
    return out
