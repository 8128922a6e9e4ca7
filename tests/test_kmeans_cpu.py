"""psvi_kmeans and the k-means selection classes, without a GPU.

  * the float64 restatement of the header's rules (tests/kmeans_util.py)
    reproduces the sklearn results recorded in tests/golden/x*_kmeans_*.npz --
    labels and n_iter equal, centres and inertia within 1e-9 relative (four
    orders over fp64 order noise ~ D 2^-53, far below the recorded margin
    >= 1e-6) -- and live sklearn when it imports;
  * the C boundary: header struct against the ctypes fields, the SIGNATURES
    entries, every refusal with a NULL stream and no device, the query;
  * the host classes with psvi.runtime.kmeans replaced by the restatement: the
    cluster-count rules, get_arbitrary_pts' split, _combine_kmeans_score both
    ways, the WeightedKmeansSelection weights, _set_num_clusters' ValueError,
    clustering=None refusing and "hip" dispatching every opened name.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import kmeans_util as KM
from golden_util import load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "psvi_hip.h")
FIXTURES = ["x1_kmeans_n257_d3_k2", "x2_kmeans_n1000_d70_k7", "x3_kmeans_n2051_d784_k5",
            "x4_kmeans_n64_d5_k64"]
REL = 1e-9


# ------------------------------------------------------------ the restatement
@pytest.fixture(scope="module", params=FIXTURES)
def solved(request):
    f = load_fixture(request.param)
    return f, KM.lloyd(f["x"], f["c0"], max_iter=300, tol=0.0)


def test_restatement_reproduces_the_recorded_sklearn_run(solved):
    f, r = solved
    assert tuple(f["x"].shape) == (f["cfg"]["N"], f["cfg"]["D"])
    assert r["status"] == 0 and r["min_count"] > 0          # no cluster ever empty
    assert r["margin"] >= 1e-6 and r["margin"] == float(f["margin"]) == f["cfg"]["margin"]
    assert np.array_equal(r["labels"], f["labels"]) and r["n_iter"] == int(f["n_iter"])
    assert np.abs(r["centres"] - f["centres"]).max() <= REL * np.abs(f["centres"]).max()
    assert abs(r["inertia"] - float(f["inertia"])) <= REL * float(f["inertia"])
    assert np.array_equal(r["counts"], np.bincount(f["labels"], minlength=f["cfg"]["K"]))


def test_restatement_against_live_sklearn(solved):
    cluster = pytest.importorskip("sklearn.cluster")
    f, r = solved
    km = cluster.KMeans(f["cfg"]["K"], init=f["c0"], n_init=1, algorithm="lloyd", max_iter=300,
                        tol=0).fit(f["x"].astype(np.float32).astype(np.float64))
    assert np.array_equal(km.labels_, r["labels"]) and km.n_iter_ == r["n_iter"]
    assert np.abs(km.cluster_centers_ - r["centres"]).max() <= REL * np.abs(r["centres"]).max()
    assert abs(km.inertia_ - r["inertia"]) <= REL * max(r["inertia"], 1e-300)


def test_restatement_rules():
    x = np.array([[0, 0], [2, 0], [2, 0], [1, 0], [1, 0], [0, 0]], np.float32)
    c0 = np.array([[0, 0], [2, 0], [2, 0], [500, 500]], np.float64)
    r = KM.lloyd(x, c0, 0)
    assert r["labels"].tolist() == [0, 1, 1, 0, 0, 0] and r["n_iter"] == 0      # lowest k
    r = KM.lloyd(x, c0, 300)
    assert r["counts"].tolist() == [4, 2, 0, 0] and np.array_equal(r["centres"][2:], c0[2:])
    assert r["n_iter"] == 2 and r["inertia"] == 1.0
    # seeding: distinct rows, a quad of words per centre, statuses
    rows = np.random.default_rng(0).integers(0, 9, (50, 4)).astype(np.float32)
    c, seeds, st = KM.seed(rows, 6, 7, 8)
    assert st == 0 and len(set(seeds.tolist())) == 6 and np.array_equal(c, rows[seeds])
    assert np.array_equal(KM.seed(rows, 3, 7, 8)[1], seeds[:3])
    assert KM.seed(np.ones((5, 2), np.float32), 2, 0, 0)[2] == 2
    bad = rows.copy()
    bad[3, 1] = np.inf
    assert KM.kmeans(bad, 2, 0, 0)["status"] == 1 and KM.consumed(6) == 24


# --------------------------------------------------------------- the boundary
WANT = ["x", "N", "D", "K", "centres_in", "seed", "offset", "max_iter", "tol", "centres_out",
        "labels_out", "counts_out", "seeds_out", "inertia_out", "n_iter_out", "status_out", "ws",
        "ws_bytes"]


def test_header_and_binding_declare_kmeans():
    from psvi.runtime import _lib

    text = open(HEADER).read()
    m = re.search(r"typedef struct psvi_kmeans_req \{(.*?)\} psvi_kmeans_req;", text, re.S)
    assert m, "request struct missing"
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert names == WANT
    assert [f[0] for f in _lib.KmeansReq._fields_] == WANT
    kinds = dict(_lib.KmeansReq._fields_)
    assert kinds["tol"] is ctypes.c_double and kinds["seed"] is ctypes.c_uint64
    assert kinds["ws_bytes"] is ctypes.c_size_t and kinds["max_iter"] is ctypes.c_int32
    assert re.search(r"int psvi_kmeans\(const psvi_kmeans_req\* req, void\* stream\);", text)
    assert re.search(r"int psvi_kmeans_query\(int32_t N, int32_t D, int32_t K, int64_t\* out\);", text)
    res, args = _lib.SIGNATURES["psvi_kmeans"]
    assert res is ctypes.c_int32 and args[0]._type_ is _lib.KmeansReq and len(args) == 2
    assert len(_lib.SIGNATURES["psvi_kmeans_query"][1]) == 4
    for phrase in ("lowest k", "keeps its centre", "one quad per centre", "no atomic"):
        assert phrase in text, phrase


def test_host_side_refusals_and_query_need_no_device():
    from psvi.runtime import _lib, kmeans_query

    lib = _lib.load()
    buf = (ctypes.c_int32 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    full, least, DT, G = kmeans_query(100, 8, 4)
    assert least < full and DT == 8 and G == 2

    def call(**kw):
        a = dict(x=p, N=100, D=8, K=4, centres_in=None, seed=1, offset=0, max_iter=3, tol=0.0,
                 centres_out=p, labels_out=p, counts_out=p, seeds_out=None, inertia_out=p,
                 n_iter_out=p, status_out=p, ws=p, ws_bytes=full)
        a.update(kw)
        return lib.psvi_kmeans(ctypes.byref(_lib.KmeansReq(**a)), None)

    EINVAL, ENOSPC, EUNSUP = -1, -2, -3
    assert [_lib.ERRORS[e] for e in (EINVAL, ENOSPC, EUNSUP)] == ["PSVI_EINVAL", "PSVI_ENOSPC",
                                                                  "PSVI_EUNSUP"]
    for kw in (dict(x=None), dict(centres_out=None), dict(labels_out=None), dict(counts_out=None),
               dict(inertia_out=None), dict(n_iter_out=None), dict(status_out=None), dict(N=0),
               dict(D=0), dict(K=0), dict(K=101), dict(offset=6), dict(max_iter=-1),
               dict(tol=-1e-9), dict(tol=float("inf")), dict(tol=float("nan"))):
        assert call(**kw) == EINVAL, kw
        assert lib.psvi_last_error()
    assert lib.psvi_kmeans(None, None) == EINVAL
    for kw in (dict(N=1000, K=129), dict(D=4097), dict(N=2**24 + 1)):
        assert call(**kw) == EUNSUP, kw
    for kw in (dict(ws=None), dict(ws_bytes=least - 1), dict(ws_bytes=0)):
        assert call(**kw) == ENOSPC, kw
    # the query: the same ranges, numbers that follow the shape
    out = (ctypes.c_int64 * 4)()
    assert lib.psvi_kmeans_query(0, 8, 4, out) == EINVAL
    assert lib.psvi_kmeans_query(100, 8, 101, out) == EINVAL
    assert lib.psvi_kmeans_query(1000, 8, 129, out) == EUNSUP
    assert lib.psvi_kmeans_query(100, 8, 4, None) == EINVAL
    assert kmeans_query(60000, 784, 50)[2] < 784          # fp64 centres past the LDS: D tiled
    assert kmeans_query(6000, 784, 5)[2] < 784
    assert kmeans_query(2**24, 4096, 128)[3] == 512
    one, two = kmeans_query(1000, 16, 8), kmeans_query(1000, 16, 9)
    assert two[1] > one[1] and (one[0] - one[1]) % (one[3] - 1) == 0


# ------------------------------------------------------------ the host classes
class _Toy(torch.utils.data.Dataset):
    def __init__(self, n=120, nc=3, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.targets = torch.arange(n) % nc
        mu = torch.tensor([[-6.0, 0.0], [6.0, 0.0], [0.0, 9.0]])[:nc]
        self.data = mu[self.targets] + torch.randn(n, 2, generator=g)

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


@pytest.fixture
def fake_kmeans(monkeypatch):
    """psvi.runtime.kmeans replaced by the restatement; records its calls."""
    import psvi.runtime as R

    calls = []

    def fake(x, K, seed=0, offset=0, centres=None, max_iter=300, tol=0.0, ws_bytes=None):
        calls.append(dict(N=int(x.shape[0]), K=K, seed=seed, offset=offset, max_iter=max_iter,
                          tol=tol, x=x.cpu().numpy().copy()))
        out = KM.kmeans(x.cpu().numpy(), K, seed, offset, max_iter=max_iter, tol=tol)
        assert out["status"] == 0
        return dict(labels=torch.as_tensor(out["labels"]), centres=torch.as_tensor(out["centres"]),
                    counts=torch.as_tensor(out["counts"]), seeds=torch.as_tensor(out["seeds"]),
                    inertia=out["inertia"], n_iter=out["n_iter"], consumed=out["consumed"])

    monkeypatch.setattr(R, "kmeans", fake)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # the rows stay where they are
    return calls


def test_kmeans_cluster_counts_streams_and_split(fake_kmeans):
    from psvi.inference import KmeansCluster

    ds = _Toy()
    kc = KmeansCluster(ds.data, ds.targets, num_classes=3, seed=11)
    kc.set_num_clusters(4)
    assert kc.pts_per_class == 2                          # max(floor(4 / 3), 2)
    kc.set_num_clusters(12)
    assert kc.pts_per_class == 4 and kc.num_clusters == 12
    kc.run_kmeans()
    assert [c["K"] for c in fake_kmeans] == [4, 4, 4] and [c["N"] for c in fake_kmeans] == [40] * 3
    assert [c["offset"] for c in fake_kmeans] == [0, 16, 32] and fake_kmeans[0]["seed"] == 11
    x0 = ds.data[ds.targets == 0].double()
    assert fake_kmeans[0]["max_iter"] == 300
    assert fake_kmeans[0]["tol"] == pytest.approx(1e-4 * float(x0.var(0, unbiased=False).mean()),
                                                  rel=1e-6)
    # every row once, in its own class's dict; centres per class
    assert len(kc.kmeans_dict) == 3 and [c.shape for c in kc.cluster_centers] == [(4, 2)] * 3
    for c, d in enumerate(kc.kmeans_dict):
        rows = sorted(i for v in d.values() for i in v)
        assert rows == [i for i in range(120) if i % 3 == c]
    # the split: total // K each, the remainder on the last; an empty cluster is skipped
    kc.kmeans_dict = [{j: list(range(40 * c + 10 * j, 40 * c + 10 * j + 10)) for j in range(4)}
                      for c in range(3)]
    kc.kmeans_dict[1][9] = []
    np.random.seed(0)
    pts = kc.get_arbitrary_pts(29)
    assert len(pts) == 29 == len(set(pts))
    sizes = [sum(p in set(v) for p in pts) for d in kc.kmeans_dict for v in d.values() if v]
    assert sizes == [2] * 11 + [7]
    # unbalanced: one clustering of all rows; 3-d rows flattened; cosine rows unit length
    fake_kmeans.clear()
    ku = KmeansCluster(ds.data.reshape(120, 1, 2), ds.targets, num_classes=3, balance=False, seed=2,
                       dist="cosine")
    ku.set_num_clusters(5)
    ku.run_kmeans()
    assert len(fake_kmeans) == 1 and fake_kmeans[0]["K"] == 5 and fake_kmeans[0]["x"].shape == (120, 2)
    assert np.allclose(np.linalg.norm(fake_kmeans[0]["x"], axis=1), 1.0, atol=1e-6)
    kz = KmeansCluster(torch.zeros(4, 2), torch.zeros(4), dist="cosine")
    assert torch.equal(kz._rows(), torch.zeros(4, 2))     # a zero row stays zero
    with pytest.raises(ValueError, match="valid dist"):
        KmeansCluster(ds.data, ds.targets, dist="manhattan")


def test_set_num_clusters_table_and_its_value_error():
    from psvi.inference import KmeansScoreSelection, KmeansSelection

    ds = _Toy()
    for cls in (KmeansSelection, KmeansScoreSelection):
        for n, k in ((30, 30), (50, 50), (80, 20), (100, 20)):
            assert cls(ds, n, 3, 0)._set_num_clusters() == k
        assert cls(ds, 37, 3, 0, multiple_pts=False)._set_num_clusters() == 37
        with pytest.raises(ValueError, match="returns None"):
            cls(ds, 37, 3, 0)._set_num_clusters()
    with pytest.raises(NotImplementedError, match="embedding"):
        KmeansSelection(ds, 30, 3, 0, embedding_flag=True, loaded=False).select()


def test_kmeans_selection_and_loaded_rows(fake_kmeans, tmp_path):
    from psvi.inference import KmeansSelection

    ds = _Toy()
    np.random.seed(1)
    sel = KmeansSelection(ds, 30, 3, seed=4, loaded=False)
    idx = sel.select()
    assert len(idx) == 30 == len(set(idx)) and all(isinstance(i, int) for i in idx)
    assert np.bincount(ds.targets.numpy()[idx]).tolist() == [10, 10, 10]
    assert [c["K"] for c in fake_kmeans] == [10, 10, 10]
    # loaded: the embedding file's rows when it exists, the dataset's otherwise
    fake_kmeans.clear()
    KmeansSelection(ds, 30, 3, seed=4, loaded=True, data_folder=str(tmp_path), dnm="toy").select()
    assert np.array_equal(fake_kmeans[0]["x"], ds.data[ds.targets == 0].numpy())
    emb = np.random.default_rng(0).standard_normal((120, 3))
    np.savetxt(tmp_path / "embedding_toy_4.csv", emb, delimiter=",")
    fake_kmeans.clear()
    KmeansSelection(ds, 30, 3, seed=4, loaded=True, data_folder=str(tmp_path), dnm="toy").select()
    assert np.array_equal(fake_kmeans[0]["x"], emb[ds.targets.numpy() == 0].astype(np.float32))


def test_combine_kmeans_score_both_ways(fake_kmeans):
    from psvi.inference import KmeansScoreSelection

    ds = _Toy()
    # one row per cluster carries all the mass: it is the row drawn (choose_difficult),
    # or the one row never drawn (not choose_difficult, two rows per cluster)
    for difficult in (True, False):
        sel = KmeansScoreSelection(ds, 80 if not difficult else 100, 3, seed=4,
                                   score_type="entropy", choose_difficult=difficult)
        sel.kmeans_cluster = type("C", (), {})()
        clusters = [list(range(6 * j, 6 * j + 6)) for j in range(20)]
        sel.kmeans_cluster.kmeans_dict = [{j: clusters[j] for j in range(10)},
                                          {j: clusters[10 + j] for j in range(10)}, {7: []}]
        heavy = [c[2] for c in clusters]
        score = np.full(120, 1e-12)
        score[heavy] = 1.0
        sel.score_arr = torch.as_tensor(score)
        np.random.seed(3)
        got = sel._combine_kmeans_score()
        per = 5 if difficult else 4                       # int(num_pseudo / 20)
        assert len(got) == 20 * per and all(g // 6 == i // per for i, g in enumerate(got))
        assert len(set(got)) == len(got)
        if difficult:
            assert set(heavy) <= set(got)                 # the top count is always among the k
        else:
            assert not set(heavy) & set(got)
    # alpha flattens the draw: with a large alpha the heavy row is no longer certain
    sel = KmeansScoreSelection(ds, 100, 3, seed=4, score_type="entropy", alpha=1e6)
    assert sel.alpha == 1e6 and sel.multiple_pts and sel.choose_difficult


def test_weighted_kmeans_weights(fake_kmeans, monkeypatch):
    from psvi.inference import WeightedKmeansSelection, WeightedSubset

    ds = _Toy()
    sel = WeightedKmeansSelection(ds, 30, 3, seed=4)
    assert sel.score_type == "entropy" and sel.loaded is False
    score = torch.linspace(0.1, 2.0, 120, dtype=torch.float64)
    monkeypatch.setattr(sel, "_get_uncertainty_score", lambda: score)
    np.random.seed(2)
    sub = sel.get_weighted_subset()
    idx = sel.core_idc
    assert isinstance(sub, WeightedSubset) and sub.indices is idx and len(idx) == 30 == len(set(idx))
    want = 120 * score[idx] / score[idx].sum()
    assert torch.allclose(sel.wt_vec, want, rtol=1e-12) and abs(float(sel.wt_vec.sum()) - 120) < 1e-9
    assert sub[3][0] == 3 and torch.equal(sub[3][1], ds.data[idx[3]])
    assert float(sub[3][3]) == float(sel.wt_vec[3])


def test_clustering_keyword_refuses_and_dispatches(fake_kmeans, monkeypatch):
    import psvi.inference.utils as U
    from psvi.experiments import flow_psvi
    from psvi.inference.baselines import MfviSelect, run_selection_with_mfvi

    ds = _Toy()
    opened = {"kmeans": U.KmeansSelection, "weighted_kmeans": U.WeightedKmeansSelection,
              **{f"scored_kmeans_{s}": U.KmeansScoreSelection
                 for s in ("el2n", "entropy", "least_confidence", "forgetting")}}
    kw = dict(train_dataset=ds, test_dataset=ds, num_pseudo=30, nc=3, architecture="fn", D=2,
              loaded_from_psvi=False)
    for m in opened:
        with pytest.raises(NotImplementedError, match="k-means|submodular"):
            U.CoresetSelect(score_method=m, **kw).select_data()
        with pytest.raises(NotImplementedError, match="k-means|submodular"):
            U.CoresetSelect(score_method=m, clustering=None, **kw).select_data()
    for m in ("kmeans_gradient", "submodular"):
        with pytest.raises(NotImplementedError, match="k-means|submodular"):
            U.CoresetSelect(score_method=m, clustering="hip", **kw).select_data()
    with pytest.raises(ValueError, match="clustering"):
        U.CoresetSelect(score_method="kmeans", clustering="sklearn", **kw)
    with pytest.raises(NotImplementedError, match="incremental"):
        run_selection_with_mfvi(train_dataset=ds, test_dataset=ds, clustering="hip",
                                mfvi_selection_method="incremental")
    # "hip": every opened name builds its class and runs it
    seen = []
    monkeypatch.setattr(U.Selection, "pretrain", lambda self, **k: seen.append(type(self)))
    monkeypatch.setattr(U.ScoreSelection, "_get_uncertainty_score",
                        lambda self: torch.linspace(0.5, 1.5, 120, dtype=torch.float64))
    for m, cls in opened.items():
        seen.clear()
        np.random.seed(0)
        cs = U.CoresetSelect(score_method=m, clustering="hip", **kw)
        cs.select_data()
        assert len(cs.wt_index) == 30 and isinstance(cs.chosen_dataset, U.WeightedSubset), m
        assert abs(sum(cs.wt_index.values()) - 120) < 1e-3, m
        want_pretrain = [] if m == "kmeans" else [cls]
        assert seen == want_pretrain, m
        if m.startswith("scored_kmeans_"):
            assert cls is U.KmeansScoreSelection
    # the keyword travels from the driver through run_selection_with_mfvi and MfviSelect
    got = {}
    monkeypatch.setattr(MfviSelect, "_setup", lambda self: None)
    monkeypatch.setattr(MfviSelect, "evaluate_coreset", lambda self: {"wt_index": self.wt_index})
    real = U.CoresetSelect

    def spy(**k):
        got.update(k)
        return real(**k)

    monkeypatch.setattr(U, "CoresetSelect", spy)
    np.random.seed(0)
    res = run_selection_with_mfvi(train_dataset=ds, test_dataset=ds, num_pseudo=30, nc=3, D=2,
                                  architecture="fn", clustering="hip", loaded_from_psvi=False)
    assert got["clustering"] == "hip" and got["score_method"] == "kmeans" and len(res["wt_index"]) == 30
    sent = {}
    monkeypatch.setitem(flow_psvi.extended_inf_dict, "mfvi_selection",
                        lambda **k: sent.update(k) or {})
    args = dict(mc_samples=4, num_epochs=1, data_minibatch=8, log_every=1, lr0net=1e-3,
                init_sd=1e-3, num_trials=1, coreset_sizes=[30], architecture="fn", test_ratio=0.2,
                inner_it=1, trainer="nested", lr0u=1e-3, lr0v=1e-2)
    flow_psvi.experiment_driver(["halfmoon"], ["mfvi_selection"], dict(args, clustering="hip"),
                                write=False)
    assert sent["clustering"] == "hip" and sent["mfvi_selection_method"] == "kmeans"
    flow_psvi.experiment_driver(["halfmoon"], ["mfvi_selection"], args, write=False)
    assert sent["clustering"] is None
