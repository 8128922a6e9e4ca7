"""psvi_coreset_draw restated in numpy float64 from its description in
include/psvi_hip.h (no torch, no GPU), on philox_util.words.

Word j of the stream (seed, offset) is element j % 4 of the Philox quad
offset / 4 + j / 4; U_j = (word_j + 0.5) 2^-32 (exact in float64).

  replace(w, n, ...):    C = cumsum(w) in index order, t_j = U_j C[-1], the
                         smallest i with C_i > t_j, clamped to the last
                         positive weight; consumes 4 ceil(n / 4) words.
  noreplace(w, n, ...):  key_i = log(U_i) / w_i (w_i > 0; -inf for w_i == 0),
                         the n largest keys in descending order, equal keys
                         by the lower index; consumes 4 ceil(M / 4) words.
Both return -1 indices and a status (1 negative / non-finite weight, 2 zero
sum, 3 fewer than n positive weights) when the weights admit no draw.
"""
import numpy as np

import philox_util as PX


def stream_words(seed, offset, count):
    """Words [0, count) of the stream as a uint64 vector."""
    return PX.words(seed, offset, (int(count) + 3) // 4).reshape(-1)[:int(count)]


def uniforms(words):
    return (np.asarray(words, dtype=np.uint64).astype(np.float64) + 0.5) * 2.0 ** -32


def status_of(w, n=None):
    w = np.asarray(w, dtype=np.float32)
    if (~np.isfinite(w)).any() or (w < 0).any():
        return 1
    if not (w > 0).any():
        return 2
    if n is not None and int((w > 0).sum()) < n:
        return 3
    return 0


def consumed(M, n, replacement):
    return 4 * (((n if replacement else M) + 3) // 4)


def replace(w, n, seed, offset, words=None, detail=False):
    """(idx int32 (n), status).  detail=True also returns (t, C)."""
    w = np.asarray(w, dtype=np.float32)
    st = status_of(w)
    if st:
        out = np.full(n, -1, dtype=np.int32)
        return (out, st, None, None) if detail else (out, st)
    C = np.cumsum(w.astype(np.float64))
    wd = stream_words(seed, offset, n) if words is None else np.asarray(words)[:n]
    t = uniforms(wd) * C[-1]
    idx = np.searchsorted(C, t, side="right")          # the smallest i with C_i > t
    idx = np.minimum(idx, int(np.nonzero(w > 0)[0][-1])).astype(np.int32)
    return (idx, 0, t, C) if detail else (idx, 0)


def keys(w, seed, offset, words=None):
    w = np.asarray(w, dtype=np.float32)
    M = w.shape[0]
    wd = stream_words(seed, offset, M) if words is None else np.asarray(words)[:M]
    k = np.full(M, -np.inf)
    pos = w > 0
    k[pos] = np.log(uniforms(wd)[pos]) / w[pos].astype(np.float64)
    return k


def noreplace(w, n, seed, offset, words=None, detail=False):
    """(idx int32 (n), status).  detail=True also returns the sorted keys of
    all M rows (descending, the order the rows would be drawn in)."""
    w = np.asarray(w, dtype=np.float32)
    st = status_of(w, n)
    if st:
        out = np.full(n, -1, dtype=np.int32)
        return (out, st, None) if detail else (out, st)
    k = keys(w, seed, offset, words)
    order = np.lexsort((np.arange(k.shape[0]), -k))     # key descending, then index ascending
    idx = order[:n].astype(np.int32)
    return (idx, 0, k[order]) if detail else (idx, 0)


def replace_unsafe(t, C, tol=1e-12):
    """Draws whose t lies within tol C[-1] of a prefix value: a prefix summed
    in another association may decide them differently."""
    j = np.searchsorted(C, t)
    lo = np.abs(t - C[np.clip(j - 1, 0, C.shape[0] - 1)])
    hi = np.abs(t - C[np.clip(j, 0, C.shape[0] - 1)])
    return np.minimum(lo, hi) < tol * C[-1]


def noreplace_unsafe(sorted_keys, n, tol=1e-12):
    """True when two adjacent keys among the top n + 1 differ by less than tol
    relative: a logarithm rounded otherwise may order them differently."""
    k = sorted_keys[:n + 1]
    k = k[np.isfinite(k)]
    return bool((np.abs(np.diff(k)) < tol * np.abs(k[1:])).any())
