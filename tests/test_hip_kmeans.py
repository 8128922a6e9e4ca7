"""psvi_kmeans on the device against tests/kmeans_util.py, the float64
restatement of include/psvi_hip.h's rules, and against the sklearn results
recorded in tests/golden/x*_kmeans_*.npz.

  * the fixtures (minimum relative margin >= 1e-6, no empty cluster): labels,
    counts and n_iter equal, centres and inertia within 1e-9 relative -- fp64
    order effects are ~ D 2^-53 ~ 1e-13;
  * seeding on small-integer data (every sum exact in fp64): seeds_out equals
    the restatement's, consumed = 4 K;
  * max_iter 0 / 1, tol, ties (lowest k), an empty cluster (kept), K = 1, the
    D-tiled and the second-pass-sums shapes (from psvi_kmeans_query), two
    workspace sizes, statuses 1 and 2, two runs bitwise equal;
  * every output sits between sentinels;
  * end to end: CoresetSelect(clustering="hip") and run_selection_with_mfvi.
"""
import ctypes

import numpy as np
import pytest
import torch

import kmeans_util as KM
from golden_util import load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 2**32 * 77 + 20261021
SENT = -7777
FIXTURES = ["x1_kmeans_n257_d3_k2", "x2_kmeans_n1000_d70_k7", "x3_kmeans_n2051_d784_k5",
            "x4_kmeans_n64_d5_k64"]
REL = 1e-9


def _raw(x, K, seed=SEED, offset=0, centres=None, max_iter=300, tol=0.0, ws_bytes=None,
         seeds=True):
    """psvi_kmeans through the C ABI with sentinels around every output; a dict
    of host arrays after the sentinels were checked."""
    from psvi.runtime import _lib, kmeans_query
    from psvi.runtime.engine import _ptr, _stream

    xd = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=DEV)
    N, D = xd.shape
    full, least, _, _ = kmeans_query(N, D, K)
    ws_bytes = full if ws_bytes is None else ws_bytes
    cin = None if centres is None else torch.as_tensor(np.ascontiguousarray(centres, np.float64),
                                                       device=DEV)
    P = 4
    cbuf = torch.full((K * D + 2 * P,), float(SENT), dtype=torch.float64, device=DEV)
    lbuf = torch.full((N + 2 * P,), SENT, dtype=torch.int32, device=DEV)
    kbuf = torch.full((K + 2 * P,), SENT, dtype=torch.int32, device=DEV)
    sbuf = torch.full((K + 2 * P,), SENT, dtype=torch.int32, device=DEV)
    ibuf = torch.full((3,), float(SENT), dtype=torch.float64, device=DEV)
    nbuf = torch.full((6,), SENT, dtype=torch.int32, device=DEV)     # . n_iter . . status .
    ws = torch.empty(ws_bytes + 512, dtype=torch.uint8, device=DEV)
    ws[ws_bytes:] = 0xA5
    req = _lib.KmeansReq(_ptr(xd), N, D, K, _ptr(cin), seed, offset, max_iter, tol,
                         _ptr(cbuf[P:]), _ptr(lbuf[P:]), _ptr(kbuf[P:]),
                         _ptr(sbuf[P:]) if seeds else None, _ptr(ibuf[1:]), _ptr(nbuf[1:]),
                         _ptr(nbuf[4:]), _ptr(ws), ws_bytes)
    rc = _lib.load().psvi_kmeans(ctypes.byref(req), _stream())
    assert rc == 0, _lib.load().psvi_last_error()
    torch.cuda.synchronize()
    assert (ws[ws_bytes:] == 0xA5).all(), "workspace overrun"
    out = {}
    for key, buf, n in (("centres", cbuf, K * D), ("labels", lbuf, N), ("counts", kbuf, K),
                        ("seeds", sbuf, K)):
        b = buf.cpu().numpy()
        assert (b[:P] == SENT).all() and (b[P + n:] == SENT).all(), key + " overrun"
        out[key] = b[P:P + n]
    if not seeds:
        assert (out["seeds"] == SENT).all()
    out["centres"] = out["centres"].reshape(K, D)
    ib, nb = ibuf.cpu().numpy(), nbuf.cpu().numpy()
    assert ib[0] == SENT and ib[2] == SENT and (nb[[0, 2, 3, 5]] == SENT).all()
    out.update(inertia=float(ib[1]), n_iter=int(nb[1]), status=int(nb[4]))
    return out


def _close(got, ref):
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got) - ref).max() <= REL * max(np.abs(ref).max(), 1e-300)


def _same(got, ref, what=""):
    assert got["status"] == 0 and ref["status"] == 0, what
    assert np.array_equal(got["labels"], ref["labels"]), what
    assert np.array_equal(got["counts"], np.bincount(ref["labels"], minlength=len(got["counts"]))), what
    assert got["n_iter"] == ref["n_iter"], what
    assert _close(got["centres"], ref["centres"]), what
    assert abs(got["inertia"] - ref["inertia"]) <= REL * max(ref["inertia"], 1e-300), what


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_equal_sklearn(name):
    f = load_fixture(name)
    x = f["x"].astype(np.float32)
    got = _raw(x, f["cfg"]["K"], centres=f["c0"])
    ref = dict(labels=f["labels"], centres=f["centres"], inertia=float(f["inertia"]),
               n_iter=int(f["n_iter"]), status=0)
    _same(got, ref, name)
    assert (got["seeds"] == -1).all()
    # the same through the wrapper, and a second run bit for bit
    from psvi.runtime import kmeans

    xd = torch.as_tensor(x, device=DEV)
    a = kmeans(xd, f["cfg"]["K"], centres=torch.as_tensor(f["c0"], device=DEV))
    b = kmeans(xd, f["cfg"]["K"], centres=torch.as_tensor(f["c0"], device=DEV))
    assert a["consumed"] == 0 and a["n_iter"] == int(f["n_iter"])
    assert np.array_equal(a["labels"].cpu().numpy(), f["labels"])
    for k in ("centres", "labels", "counts"):
        assert torch.equal(a[k], b[k]), k
    assert a["inertia"] == b["inertia"]


def _integer_rows(N, D, seed, hi=9):
    return np.random.default_rng(seed).integers(0, hi, (N, D)).astype(np.float32)


@pytest.mark.parametrize("N,D,K", [(257, 3, 2), (1000, 70, 7), (2051, 784, 5), (64, 5, 64),
                                   (130, 17, 1)])
def test_seeding_on_exact_data_equals_the_restatement(N, D, K):
    """Small integers: every distance and every prefix sum is exact in any
    order, so the seeds -- and, with max_iter = 0, the labels -- are equal."""
    from psvi.runtime import kmeans

    x = _integer_rows(N, D, 100 + N)
    for off in (0, 4 * 2**32 + 8):
        ref = KM.kmeans(x, K, SEED, off, max_iter=0)
        got = _raw(x, K, SEED, off, max_iter=0)
        assert got["status"] == 0 and ref["status"] == 0
        assert np.array_equal(got["seeds"], ref["seeds"]), (N, D, K, off)
        assert np.array_equal(got["centres"], x[ref["seeds"]].astype(np.float64))
        assert np.array_equal(got["labels"], ref["labels"]) and got["n_iter"] == 0
        assert got["inertia"] == ref["inertia"]
    w = kmeans(torch.as_tensor(x, device=DEV), K, SEED, 0, max_iter=0)
    assert w["consumed"] == 4 * K == KM.consumed(K)
    assert np.array_equal(w["seeds"].cpu().numpy(), KM.kmeans(x, K, SEED, 0, max_iter=0)["seeds"])
    # seeds_out is nullable
    assert _raw(x, K, SEED, 0, max_iter=0, seeds=False)["status"] == 0


def test_max_iter_and_tol_stop_where_the_restatement_stops():
    f = load_fixture("x1_kmeans_n257_d3_k2")
    x, c0 = f["x"], f["c0"]
    full = KM.lloyd(x, c0, 300, 0.0)
    assert full["n_iter"] == int(f["n_iter"]) >= 4
    for mi in (0, 1, 3):
        ref = KM.lloyd(x, c0, mi, 0.0)
        assert ref["n_iter"] == mi
        _same(_raw(x, 2, centres=c0, max_iter=mi), ref, f"max_iter {mi}")
    # a tol between two shifts: the stop is at that update, well clear of rounding
    sh = full["shifts"]
    j = next(i for i in range(1, len(sh)) if sh[i] < 0.5 * sh[i - 1])
    tol = float(np.sqrt(sh[j] * sh[j - 1]))
    ref = KM.lloyd(x, c0, 300, tol)
    assert ref["n_iter"] == j + 1 < full["n_iter"]
    _same(_raw(x, 2, centres=c0, tol=tol), ref, "tol")


def test_ties_go_to_the_lowest_k_and_an_empty_cluster_keeps_its_centre():
    # duplicated rows, centres 1 and 2 equal and equidistant with centre 0 from the rows at 1
    x = np.array([[0, 0], [2, 0], [2, 0], [1, 0], [1, 0], [0, 0]], np.float32)
    c0 = np.array([[0, 0], [2, 0], [2, 0], [500, 500]], np.float64)
    got = _raw(x, 4, centres=c0, max_iter=0)
    assert got["labels"].tolist() == [0, 1, 1, 0, 0, 0] and got["counts"].tolist() == [4, 2, 0, 0]
    ref = KM.lloyd(x, c0, 300, 0.0)
    got = _raw(x, 4, centres=c0)
    _same(got, ref, "ties")
    assert got["counts"][2] == 0 and got["counts"][3] == 0
    assert np.array_equal(got["centres"][2:], c0[2:])          # kept bit for bit


def test_statuses_leave_minus_one_labels():
    from psvi.runtime import kmeans

    x = _integer_rows(200, 6, 5)
    bad = x.copy()
    bad[137, 4] = np.nan
    for kw in (dict(), dict(centres=x[:3].astype(np.float64))):
        got = _raw(bad, 3, **kw)
        assert got["status"] == 1 and (got["labels"] == -1).all() and (got["counts"] == 0).all()
        assert got["n_iter"] == 0 and got["inertia"] == 0.0
    c_bad = x[:3].astype(np.float64)
    c_bad[1, 0] = np.inf
    assert _raw(x, 3, centres=c_bad)["status"] == 1
    same = np.tile(np.array([[3, 1, 4]], np.float32), (70, 1))
    got = _raw(same, 2)
    assert got["status"] == 2 and (got["labels"] == -1).all() and got["seeds"][1] == -1
    assert KM.kmeans(same, 2, SEED, 0)["status"] == 2 and KM.kmeans(bad, 3, SEED, 0)["status"] == 1
    with pytest.raises(ValueError, match="distinct rows"):
        kmeans(torch.as_tensor(same, device=DEV), 2, SEED)
    with pytest.raises(ValueError, match="not finite"):
        kmeans(torch.as_tensor(bad, device=DEV), 3, SEED)
    # one distinct row fewer than K, the duplicates last: the clamp never takes a zero distance
    two = np.concatenate([np.array([[0, 0, 0], [50, 50, 50]], np.float32), same[:40]])
    got = _raw(two, 3)
    assert got["status"] == 0 and len(set(got["seeds"].tolist())) == 3


def _blobs(N, D, K, seed):
    rng = np.random.default_rng(seed)
    mu = 6.0 * rng.standard_normal((K, D))
    return (mu[rng.integers(0, K, N)] + rng.standard_normal((N, D))).astype(np.float32)


def test_tiled_columns_second_pass_sums_and_two_workspaces():
    """Shapes chosen from psvi_kmeans_query: D above the LDS tile, more row
    tiles than assignment workgroups hold one each, and workspaces on both
    sides of the one-pass size."""
    from psvi.runtime import kmeans_query

    # (N, D, K): K = 40 makes the tile narrower than D; N = 1100 leaves a ragged last tile
    for N, D, K in ((1100, 300, 40), (700, 33, 3), (33000, 8, 4)):
        x = _blobs(N, D, K, N + D)
        full, least, DT, G = kmeans_query(N, D, K)
        assert least < full
        if D == 300:
            assert DT < D
        if N == 33000:
            assert G < (N + 63) // 64                 # several row tiles per workgroup
        c0, _, st = KM.seed(x, K, 3, 0)
        ref = KM.lloyd(x, c0, 300, 0.0)
        assert st == 0 and ref["margin"] >= 1e-6, (N, D, K, ref["margin"])
        one = _raw(x, K, centres=c0, ws_bytes=full)
        part = (full - least) // max(G - 1, 1)
        for ws_bytes in (least, least + 2 * part + 8):    # one partial; three (or all)
            two = _raw(x, K, centres=c0, ws_bytes=ws_bytes)
            _same(two, ref, f"second pass {N, D, K, ws_bytes}")
            assert np.array_equal(two["labels"], one["labels"])
        _same(one, ref, f"one pass {N, D, K}")


def test_short_workspace_is_refused_on_the_device_path():
    from psvi.runtime import _lib, kmeans, kmeans_query

    x = torch.zeros(100, 4, device=DEV)
    with pytest.raises(_lib.PsviError, match="PSVI_ENOSPC"):
        kmeans(x, 3, ws_bytes=kmeans_query(100, 4, 3)[1] - 1)


# ------------------------------------------------------------------ end to end
def _blob_dataset(n=240, seed=0):
    from psvi.experiments.experiments_utils import SynthDataset

    g = torch.Generator().manual_seed(seed)
    mu = torch.tensor([[-6.0, 0.0], [6.0, 0.0], [0.0, 9.0]])
    y = torch.arange(n) % 3
    return SynthDataset(mu[y] + torch.randn(n, 2, generator=g), y)


@pytest.mark.parametrize("method", ["kmeans", "scored_kmeans_entropy", "weighted_kmeans"])
def test_coreset_select_with_device_clustering(method):
    from psvi.inference import CoresetSelect

    ds = _blob_dataset()
    np.random.seed(0)
    cs = CoresetSelect(train_dataset=ds, test_dataset=ds, num_pseudo=30, nc=3, D=2, seed=3,
                       score_method=method, pretrain_epochs=1, loaded_from_psvi=False,
                       clustering="hip", mc_samples=2, n_hidden=8, init_sd=1e-3)
    cs.select_data()
    idx = [int(k) for k in cs.wt_index]
    assert len(idx) == 30 == len(set(idx)) and min(idx) >= 0 and max(idx) < len(ds)
    w = np.array(list(cs.wt_index.values()), np.float64)
    assert np.isfinite(w).all() and abs(w.sum() - len(ds)) <= 1e-3 * len(ds)
    # 30 clusters of one point each, ten per class (num_pseudo 30 -> 30 clusters)
    y = np.asarray(ds.targets)[idx]
    assert np.bincount(y, minlength=3).tolist() == [10, 10, 10]
    item = cs.chosen_dataset[0]
    assert len(item) == 4


def test_run_selection_with_mfvi_on_kmeans():
    from psvi.inference import run_selection_with_mfvi

    ds = _blob_dataset()
    res = run_selection_with_mfvi(
        train_dataset=ds, test_dataset=ds, N=len(ds), D=2, nc=3, num_pseudo=30, seed=1,
        mc_samples=2, data_minibatch=64, num_epochs=2, log_every=1, architecture="fn",
        n_hidden=8, init_sd=1e-3, mfvi_selection_method="kmeans", clustering="hip",
        pretrain_epochs=1, loaded_from_psvi=False)
    assert isinstance(res, dict) and len(res["accs"]) > 0
    assert np.isfinite(np.asarray(res["accs"], np.float64)).all()
    assert np.isfinite(np.asarray(res["nlls"], np.float64)).all()
