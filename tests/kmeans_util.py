"""psvi_kmeans restated in numpy float64 from its description in
include/psvi_hip.h (no torch, no GPU), on philox_util.words.

  d(i,k) = sum_f (x_if - c_kf)^2, x widened from float32, centres float64.
  seed(x, K, seed, offset):  centre 0 = row floor(U_0 N) clamped; centre j:
      m_i = min over the chosen centres of d(i, .), C = cumsum(m) in index
      order, t = U_{4j} C[-1], the smallest i with C_i > t clamped to the last
      i with m_i > 0.  U_j = (word_j + 0.5) 2^-32, one quad of words per centre.
  lloyd(x, c0, max_iter, tol):  iteration t assigns against C_t (lowest k
      among equals); t == max_iter or (t > 0 and shift_{t-1} <= tol): final,
      n_iter = t; else t > 0 and no label changed: n_iter = t + 1; else
      C_{t+1,k} = mean of cluster k's rows, an empty cluster kept.
Both return a status (1 a non-finite input, 2 fewer than K distinct rows
reachable) with labels -1 when the rows admit no clustering.  lloyd also
returns the minimum over all iterations and rows of the relative margin
(d_second - d_best) / (d_best + d_second) (inf for K == 1): how far the
labels are from depending on the order of a sum.
"""
import numpy as np

import coreset_draw_util as CD


def dist2(x, c):
    """[N][K] squared distances, the differences squared and added."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float64)
    out = np.empty((x.shape[0], c.shape[0]))
    for k in range(c.shape[0]):
        diff = x - c[k]
        out[:, k] = (diff * diff).sum(axis=1)
    return out


def seed(x, K, seed, offset):
    """(centres [K][D] float64, seeds int32 [K], status)."""
    x32 = np.asarray(x, dtype=np.float32)
    N, D = x32.shape
    seeds = np.full(K, -1, dtype=np.int32)
    centres = np.zeros((K, D))
    U = CD.uniforms(CD.stream_words(seed, offset, 4 * K))
    i = min(int(U[0] * N), N - 1)
    seeds[0], centres[0] = i, x32[i].astype(np.float64)
    m = None
    for j in range(1, K):
        d = dist2(x32, centres[j - 1:j])[:, 0]
        if not np.isfinite(d).all():
            return centres, seeds, 1
        m = d if m is None else np.minimum(m, d)
        if not (m > 0).any():
            return centres, seeds, 2
        C = np.cumsum(m)
        i = int(np.searchsorted(C, U[4 * j] * C[-1], side="right"))
        i = min(i, int(np.nonzero(m > 0)[0][-1]))
        seeds[j], centres[j] = i, x32[i].astype(np.float64)
    return centres, seeds, 0


def consumed(K):
    return 4 * K


def assign(x, c):
    """(labels, d_best, relative margin per row)."""
    d = dist2(x, c)
    labels = np.argmin(d, axis=1).astype(np.int32)          # the first (lowest k) minimum
    best = d[np.arange(d.shape[0]), labels]
    if d.shape[1] == 1:
        return labels, best, np.full(d.shape[0], np.inf)
    d2 = d.copy()
    d2[np.arange(d.shape[0]), labels] = np.inf
    second = d2.min(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.where(best + second > 0, (second - best) / (best + second), 0.0)
    return labels, best, margin


def lloyd(x, c0, max_iter=300, tol=0.0):
    """dict(labels, centres, counts, inertia, n_iter, status, margin, shifts,
    min_count: the smallest cluster of any iteration)."""
    x32 = np.asarray(x, dtype=np.float32)
    x64 = x32.astype(np.float64)
    c = np.array(c0, dtype=np.float64, copy=True)
    N, K = x32.shape[0], c.shape[0]
    if not (np.isfinite(x32).all() and np.isfinite(c).all()):
        return dict(labels=np.full(N, -1, np.int32), centres=c, counts=np.zeros(K, np.int32),
                    inertia=0.0, n_iter=0, status=1, margin=0.0, shifts=[])
    old, shift, margin, shifts, t, min_count = None, None, np.inf, [], 0, N
    while True:
        labels, best, mg = assign(x64, c)
        margin = min(margin, float(mg.min()))
        min_count = min(min_count, int(np.bincount(labels, minlength=K).min()))
        if t == max_iter or (t > 0 and shift <= tol):
            n_iter = t
            break
        if t > 0 and np.array_equal(labels, old):
            n_iter = t + 1
            break
        new = c.copy()
        for k in range(K):
            rows = x64[labels == k]
            if len(rows) > 0:
                new[k] = rows.sum(axis=0) / len(rows)
        shift = float(((new - c) ** 2).sum())
        shifts.append(shift)
        c, old, t = new, labels, t + 1
    return dict(labels=labels, centres=c, counts=np.bincount(labels, minlength=K).astype(np.int32),
                inertia=float(best.sum()), n_iter=n_iter, status=0, margin=margin, shifts=shifts,
                min_count=min_count)


def kmeans(x, K, seed_=0, offset=0, centres=None, max_iter=300, tol=0.0):
    """The whole call: seeding (unless centres are given), then Lloyd."""
    x32 = np.asarray(x, dtype=np.float32)
    if centres is None:
        if not np.isfinite(x32).all():
            st = 1
        else:
            centres, seeds, st = seed(x32, K, seed_, offset)
        if st:
            return dict(labels=np.full(x32.shape[0], -1, np.int32), counts=np.zeros(K, np.int32),
                        inertia=0.0, n_iter=0, status=st, margin=0.0, consumed=4 * K)
        used = 4 * K
    else:
        seeds, used = np.full(K, -1, np.int32), 0
    out = lloyd(x32, centres, max_iter, tol)
    out.update(seeds=seeds, consumed=used)
    return out
