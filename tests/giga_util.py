"""fp64 torch restatement of one geodesic-ascent step of GIGA (reference
psvi/inference/baselines.py:306-322, 362-413) on ll [S][n_data], the samples'
log-likelihoods of the minibatch rows (laplace_util.ll_matrix).  Pinned to the
reference-generated fixtures k1 / k2 by tests/test_giga_cpu.py; the GPU tests
compare psvi_giga_step with it."""
import torch


def normalize(v, dim=0):
    """torch.nn.functional.normalize: v / max(|v|, 1e-12)."""
    return v / v.norm(dim=dim, keepdim=True).clamp(min=1e-12)


def step(ll, lw, pick=None):
    """One step from the coreset's unit vector lw [S] (zeros before the first).
    ``pick`` forces the selected column (default: the first argmax of score).
    Returns score [n_data], n, zeta0..2, gamma, den (gamma's denominator),
    lw (the new vector), scale (divides into the weight update: the norm is
    taken with the NEW lw, as the reference reassigns lw before forming it)
    and L."""
    cll = ll - ll.mean(0, keepdim=True)
    sum_lls = cll.sum(1)
    ell, elln = normalize(sum_lls), normalize(cll)
    d = normalize(ell - ell.dot(lw) * lw)
    dn = normalize(elln - (lw @ elln)[None, :] * lw[:, None])
    score = d @ dn
    n = int(score.argmax()) if pick is None else int(pick)
    star = elln[:, n]
    z0, z1, z2 = ell.dot(star), ell.dot(lw), star.dot(lw)
    den = z0 - z1 * z2 + z1 - z0 * z2
    gamma = (z0 - z1 * z2) / den
    new = normalize((1 - gamma) * lw + gamma * star)
    scale = 1.0 / ((1 - gamma) * new + gamma * star).norm()
    return dict(score=score, n=n, zeta0=z0, zeta1=z1, zeta2=z2, gamma=gamma, den=den, lw=new,
                scale=scale, L=sum_lls.norm())


def weights(w, pt, gamma, scale):
    """clamp(((1 - gamma) w + gamma e_pt) scale, 0) on the full w [N]."""
    w = (1 - gamma) * w
    w[pt] += gamma
    return (w * scale).clamp(min=0)


def top2_gap(score, sub):
    """The best score's margin over the best score of any OTHER data point
    (the minibatch is drawn with replacement: copies of the winner tie)."""
    n = int(score.argmax())
    other = score[torch.as_tensor(sub) != int(sub[n])]
    return float(score[n] - other.max()) if other.numel() else float("inf")
