"""psvi_coreset_draw on the device against tests/coreset_draw_util.py, the
float64 restatement of include/psvi_hip.h's description on philox_util.words.

  * exact weights (integer multiples of 2^-12: every fp64 sum is exact in any
    order): idx_out and the status word equal the restatement's, for every M
    around the run / wave / workgroup sizes and the LDS limit, every n around
    the quad, and offsets that carry the Philox counter into its second word;
  * generic fp32 weights: with replacement, the draws whose t lies within
    1e-12 C_{M-1} of a prefix value are left out (at most 0.1 % of them), the
    others are equal; without, no committed case has two adjacent keys within
    1e-12 relative among its top n + 1, and all are equal;
  * the gather is bitwise rows[idx] / targets[idx]; the words around every
    output survive;
  * statuses 1, 2, 3 leave -1 indices and untouched outputs; the wrapper
    raises ValueError, repeats itself bit for bit and reports the consumed
    stream length."""
import ctypes

import numpy as np
import pytest
import torch

import coreset_draw_util as CD

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 2**32 * 77 + 20261020          # both halves of the key in use
OFFSETS = [0, 4, 4 * 2**32 + 8]       # the last: counter 2^32 + 2, the carry word
MS = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096]
NS = [1, 3, 4, 5, 257, 10_000]
SENT = -7777


def _raw(w, n, replacement, seed, offset, rows=None, targets=None, pad=4):
    """psvi_coreset_draw through the C ABI with sentinels around (and, on a
    failed draw, inside) every output: (idx, rows_out, targets_out, status)
    as host arrays, after the sentinels were checked."""
    from psvi.runtime import _lib
    from psvi.runtime.engine import _ptr, _stream

    M = int(w.numel())
    ibuf = torch.full((n + 2 * pad,), SENT, dtype=torch.int32, device=DEV)
    status = torch.full((1,), SENT, dtype=torch.int32, device=DEV)
    D, rbuf, tbuf = 0, None, None
    if rows is not None:
        D = int(rows.shape[1])
        rbuf = torch.full(((n + 2) * max(D, 1),), float(SENT), device=DEV)
    if targets is not None:
        tbuf = torch.full((n + 2,), SENT, dtype=torch.int32, device=DEV)
    rows_on = rows is not None and D > 0
    req = _lib.CoresetDrawReq(
        _ptr(w), M, n, _lib.DRAW_REPLACE if replacement else _lib.DRAW_NOREPLACE,
        seed, offset, _ptr(rows) if rows_on else None, D, _ptr(targets), _ptr(ibuf[pad:]),
        _ptr(rbuf[D:]) if rows_on else None, _ptr(tbuf[1:]) if targets is not None else None,
        _ptr(status))
    rc = _lib.load().psvi_coreset_draw(ctypes.byref(req), _stream())
    assert rc == 0, _lib.load().psvi_last_error()
    torch.cuda.synchronize()
    ib = ibuf.cpu().numpy()
    assert (ib[:pad] == SENT).all() and (ib[pad + n:] == SENT).all(), "idx_out overrun"
    st = int(status.item())
    r_out = t_out = None
    if rows is not None:
        rb = rbuf.cpu().numpy()
        if rows_on:
            assert (rb[:D] == SENT).all() and (rb[(n + 1) * D:] == SENT).all(), "rows_out overrun"
        r_out = rb[D:(n + 1) * D].reshape(n, D) if rows_on else np.zeros((n, 0), np.float32)
        if st or not rows_on:
            assert (rb == SENT).all(), "rows_out written"
    if targets is not None:
        tb = tbuf.cpu().numpy()
        assert tb[0] == SENT and tb[-1] == SENT, "targets_out overrun"
        t_out = tb[1:-1]
        if st:
            assert (tb == SENT).all(), "targets_out written on a failed draw"
    return ib[pad:pad + n], r_out, t_out, st


def _exact_weights(M, zeros):
    rng = np.random.default_rng(1000 + M)
    k = rng.integers(1, 4096, size=M)
    if zeros and M > 1:
        k[rng.random(M) < 0.25] = 0
        k[rng.integers(0, M)] = 4095          # at least one positive weight
        k[-1] = 0                             # the clamp's row
    return (k / 4096.0).astype(np.float32)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("replacement", [True, False])
def test_exact_weights_equal_the_restatement(M, replacement):
    """Exact sums: every index (and the status of a draw that cannot be made)
    equals the restatement's.  The first offset runs on a 4-byte-aligned
    idx_out (the scalar stores), the others on a 16-byte-aligned one."""
    for zeros in (True, False):
        w = _exact_weights(M, zeros)
        wd = torch.tensor(w, device=DEV)
        for n in NS:
            n = n if replacement else min(n, M)
            for k, off in enumerate(OFFSETS):
                ref, st_ref = (CD.replace if replacement else CD.noreplace)(w, n, SEED, off)
                got, _, _, st = _raw(wd, n, replacement, SEED, off, pad=1 if k == 0 else 4)
                assert st == st_ref, (M, n, off, zeros)
                assert np.array_equal(got, ref), (M, n, off, zeros)
                if st == 0:
                    assert (w[got] > 0).all()


REPLACE_SEEDS = [11, 12, 13]
NOREPLACE_SEEDS = [21, 22, 23, 24]


def _generic_weights(M, seed):
    rng = np.random.default_rng(seed)
    w = (rng.random(M) ** 3).astype(np.float32)    # several orders of magnitude
    w[rng.random(M) < 0.1] = 0.0
    w[0] = 0.5
    return w


@pytest.mark.parametrize("seed", REPLACE_SEEDS)
@pytest.mark.parametrize("M", [257, 4096])
def test_generic_weights_replace(M, seed):
    w = _generic_weights(M, seed)
    n = 10_000
    ref, st, t, C = CD.replace(w, n, seed, 8, detail=True)
    unsafe = CD.replace_unsafe(t, C)
    assert st == 0 and unsafe.mean() <= 1e-3
    got, _, _, st = _raw(torch.tensor(w, device=DEV), n, True, seed, 8)
    assert st == 0
    assert np.array_equal(got[~unsafe], ref[~unsafe])
    assert (w[got] > 0).all()


@pytest.mark.parametrize("seed", NOREPLACE_SEEDS)
@pytest.mark.parametrize("M", [257, 4096])
def test_generic_weights_noreplace(M, seed):
    w = _generic_weights(M, seed)
    npos = int((w > 0).sum())
    wd = torch.tensor(w, device=DEV)
    for n in (1, npos // 2, npos):
        ref, st, ks = CD.noreplace(w, n, seed, 12, detail=True)
        assert st == 0 and not CD.noreplace_unsafe(ks, n), "pick another seed"
        got, _, _, st = _raw(wd, n, False, seed, 12)
        assert st == 0 and np.array_equal(got, ref), (M, n)
        assert np.unique(got).size == n


@pytest.mark.parametrize("D", [0, 1, 3, 4, 66])
@pytest.mark.parametrize("replacement", [True, False])
def test_gather_is_bitwise(D, replacement):
    M, n = 300, 301 if replacement else 299
    rng = np.random.default_rng(D)
    w = _exact_weights(M, zeros=False)
    rows = torch.tensor(rng.standard_normal((M, D)).astype(np.float32), device=DEV)
    for targets in (torch.tensor(rng.integers(0, 10, M).astype(np.int32), device=DEV),
                    torch.tensor(rng.standard_normal(M).astype(np.float32), device=DEV)):
        idx, r_out, t_out, st = _raw(torch.tensor(w, device=DEV), n, replacement, SEED, 0,
                                     rows=rows, targets=targets)
        assert st == 0
        assert np.array_equal(idx, (CD.replace if replacement else CD.noreplace)(w, n, SEED, 0)[0])
        assert np.array_equal(r_out.view(np.int32), rows.cpu().numpy()[idx].view(np.int32))
        assert np.array_equal(t_out, targets.cpu().numpy().view(np.int32)[idx])


@pytest.mark.parametrize("case,status,replacement",
                         [(c, s, r) for c, s in (("negative", 1), ("nan", 1), ("inf", 1),
                                                 ("zero", 2)) for r in (True, False)]
                         + [("few", 3, False)])     # status 3 is a draw without replacement
def test_statuses(case, status, replacement):
    M, n = 70, 9
    w = _exact_weights(M, zeros=False)
    if case == "negative":
        w[M - 1] = -0.25
    elif case == "nan":
        w[3] = np.nan
    elif case == "inf":
        w[64] = np.inf
    elif case == "zero":
        w[:] = 0.0
    else:
        w[n - 1:] = 0.0                      # n - 1 positive weights
    rows = torch.ones(M, 5, device=DEV)
    targets = torch.arange(M, dtype=torch.int32, device=DEV)
    idx, _, _, st = _raw(torch.tensor(w, device=DEV), n, replacement, SEED, 0, rows=rows,
                         targets=targets)           # _raw asserts the outputs untouched
    assert st == status == (CD.replace(w, n, SEED, 0) if replacement
                            else CD.noreplace(w, n, SEED, 0))[1]
    assert (idx == -1).all()


def test_wrapper():
    from psvi.runtime import coreset_draw

    M, D = 130, 6
    w = torch.tensor(_exact_weights(M, zeros=True), device=DEV)
    rows = torch.randn(M, D, device=DEV)
    z = torch.arange(M, dtype=torch.float32, device=DEV)
    for replacement, n, used in ((True, 1001, 1004), (False, 40, 132)):
        a = coreset_draw(w, n, replacement, 5, 16, rows=rows, targets=z)
        b = coreset_draw(w, n, replacement, 5, 16, rows=rows, targets=z)
        assert a[3] == b[3] == used == CD.consumed(M, n, replacement)
        for x, y in zip(a[:3], b[:3]):
            assert x.dtype == y.dtype and torch.equal(x, y)
        ref = (CD.replace if replacement else CD.noreplace)(w.cpu().numpy(), n, 5, 16)[0]
        assert np.array_equal(a[0].cpu().numpy(), ref)
        assert torch.equal(a[1], rows[a[0].long()]) and torch.equal(a[2], z[a[0].long()])
        c = coreset_draw(w, n, replacement, 6, 16)
        assert c[1] is None and c[2] is None and not torch.equal(c[0], a[0])
    for bad, what in ((torch.zeros(M, device=DEV), "sum to zero"),
                      (-torch.ones(M, device=DEV), "negative")):
        with pytest.raises(ValueError, match=what):
            coreset_draw(bad, 3, True, 0, 0)
    few = torch.zeros(M, device=DEV)
    few[:2] = 1.0
    with pytest.raises(ValueError, match="fewer positive"):
        coreset_draw(few, 3, False, 0, 0)
    with pytest.raises(ValueError):
        coreset_draw(w, M + 1, False, 0, 0)


# --------------------------------------------------------------------------
# Past the first trip of the capped launches: the draws run on at most 512
# workgroups x 256 threads x 4 draws (a second pass from n > 524,288), the
# gather's row loop on at most 4096 workgroups x 4 waves (n > 16,384), its
# targets loop on 4096 x 256 threads (n > 1,048,576); the float4 row copy's
# lane loop takes a second trip from D / 4 > 64.  _raw keeps the sentinel pad
# around every output and asserts it intact.
N_DRAW2 = 524_288 + 5
N_ROWS2 = 16_384 + 3
N_TARGETS2 = 1_048_576 + 7


def test_replace_second_pass_exact_weights():
    """Exact weights: every index equals the restatement's, on a 16-byte
    aligned idx_out (int4 stores) and on one offset by one int (the scalar
    stores of the launcher's vec == false path)."""
    M, n = 257, N_DRAW2
    w = _exact_weights(M, zeros=True)
    wd = torch.tensor(w, device=DEV)
    ref, st_ref = CD.replace(w, n, SEED, OFFSETS[2])
    assert st_ref == 0
    for pad in (4, 1):
        got, _, _, st = _raw(wd, n, True, SEED, OFFSETS[2], pad=pad)
        assert st == 0 and np.array_equal(got, ref), pad


def test_replace_second_pass_generic_weights():
    M, n, seed = 257, N_DRAW2, REPLACE_SEEDS[0]
    w = _generic_weights(M, seed)
    ref, st, t, C = CD.replace(w, n, seed, 8, detail=True)
    unsafe = CD.replace_unsafe(t, C)
    assert st == 0 and unsafe.mean() <= 1e-3
    got, _, _, st = _raw(torch.tensor(w, device=DEV), n, True, seed, 8)
    assert st == 0
    assert np.array_equal(got[~unsafe], ref[~unsafe])
    assert (w[got] > 0).all()


@pytest.mark.parametrize("D", [3, 260, 257])
def test_gather_rows_second_pass(D):
    """More rows than the gather's 16,384 waves: D = 3 the scalar copy, 260 the
    float4 copy at 65 float4 per row (a second lane trip), 257 the scalar copy
    at five lane trips."""
    M, n = 300, N_ROWS2
    rng = np.random.default_rng(D)
    w = _exact_weights(M, zeros=False)
    rows = torch.tensor(rng.standard_normal((M, D)).astype(np.float32), device=DEV)
    targets = torch.tensor(rng.integers(-2**31, 2**31 - 1, M).astype(np.int32), device=DEV)
    idx, r_out, t_out, st = _raw(torch.tensor(w, device=DEV), n, True, SEED, 0, rows=rows,
                                 targets=targets)
    assert st == 0
    assert np.array_equal(idx, CD.replace(w, n, SEED, 0)[0])
    assert np.array_equal(r_out.view(np.int32), rows.cpu().numpy()[idx].view(np.int32))
    assert np.array_equal(t_out, targets.cpu().numpy()[idx])


def test_gather_targets_second_pass():
    """More targets than the gather's 1,048,576 threads; no rows."""
    M, n = 300, N_TARGETS2
    rng = np.random.default_rng(9)
    w = _exact_weights(M, zeros=False)
    targets = torch.tensor(rng.integers(-2**31, 2**31 - 1, M).astype(np.int32), device=DEV)
    idx, r_out, t_out, st = _raw(torch.tensor(w, device=DEV), n, True, SEED, 4, targets=targets)
    assert st == 0 and r_out is None
    assert np.array_equal(idx, CD.replace(w, n, SEED, 4)[0])
    assert np.array_equal(t_out, targets.cpu().numpy()[idx])
