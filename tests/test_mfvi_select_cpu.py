"""MFVI selection by predictive scores, off the device: the float64 restatement
(tests/mfvi_select_util.py) against what the reference computed (fixtures z1,
z2: tools/gen_golden_mfvi_select.py), the argument checks of
psvi_predict_scores that need no device, and the host classes' plumbing."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mfvi_select_util as R
from golden_util import load_fixture, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUP, ESTATE = -1, -3, -4


def test_restatement_matches_reference_scores():
    f = load_fixture("z1_scores")
    c = f["cfg"]
    for st, key in (("least_confidence", "least_conf"), ("entropy", "entropy")):
        ml = R.mean_logits(c["layers"], c["S"], f["params"], f["eps_" + st], f["x"],
                           c["rows_per_draw"])
        assert R.top2_gap(ml).min() >= 1e-3
        got = R.scores(ml, f["y"])
        assert rel(got[key], f["score_" + st]) < 1e-5
        if st == "least_confidence":
            assert rel(got["el2n"], f["score_el2n"]) < 1e-5
        ml = R.mean_logits(c["layers"], c["S"], f["params"], f["eps_select_" + st], f["x"],
                           c["rows_per_draw"])
        chosen = R.select(R.scores(ml)[key], f["y"], c["num_pseudo"], c["nc"])
        assert chosen == f["select_" + st].tolist()
    assert len(f["eps_entropy"]) == 2 * R.eps_count(c["layers"], c["S"])


def test_restatement_replays_forgetting_events():
    """Fixture z2: MeanFieldVI(forgetting_score_flag=True).run().  Its draws come
    per iteration as the train steps' blocks, after_epoch's blocks (one per
    minibatch of the unshuffled loader) and, where a test ran, one test block;
    the restatement on each epoch's parameters and after_epoch's draws must give
    the reference's state vectors exactly, and on the final parameters and the
    last test's draw its accuracy and NLL."""
    f = load_fixture("z2_forgetting")
    c = f["cfg"]
    n, mb, T = len(f["x"]), c["data_minibatch"], c["num_epochs"]
    nb, ec = -(-n // mb), R.eps_count(c["layers"], c["S"])
    la, fg, nl = np.zeros(n), np.zeros(n), np.ones(n)
    o = 0
    for it in range(T):
        o += nb * ec  # the train steps
        ml = R.mean_logits(c["layers"], c["S"], f["epoch_params"][it], f["draws"][o:o + nb * ec],
                           f["x"], mb)
        o += nb * ec
        assert R.top2_gap(ml).min() >= 1e-3
        la, fg, nl = R.forgetting_update(la, fg, nl, R.scores(ml, f["y"])["correct"])
        if it % c["log_every"] == 0 or it == T - 1:
            test_eps = f["draws"][o:o + ec]
            o += ec
    assert o == len(f["draws"])
    assert np.array_equal(f["epoch_params"][-1], f["params"])  # nothing trains after the last epoch
    assert np.array_equal(la, f["last_acc"]) and np.array_equal(nl, f["never_learnt"])
    assert np.array_equal(np.maximum(T * nl, fg), f["forgetting"])
    assert (fg > 0).any() and 0 < nl.sum() < n  # events of both kinds
    nt = len(f["yt"])
    assert nt <= mb  # one test batch: its shuffle does not matter
    st = R.scores(R.mean_logits(c["layers"], c["S"], f["params"], test_eps, f["xt"], nt),
                  f["yt"])["stats"]
    assert st[0] == round(f["accs"][-1] * nt) and abs(st[1] / nt - f["nlls"][-1]) < 1e-5 * f["nlls"][-1]
    assert len(f["elbos"]) == T * nb


def test_forgetting_update_rule():
    la, fg, nl = np.zeros(4), np.zeros(4), np.ones(4)
    for correct in ([1, 0, 1, 0], [0, 0, 1, 1], [1, 0, 0, 1]):
        la, fg, nl = R.forgetting_update(la, fg, nl, np.array(correct, float))
    assert la.tolist() == [1, 0, 0, 1] and fg.tolist() == [1, 0, 1, 0] and nl.tolist() == [0, 1, 0, 0]


def _req(lib_mod, the_plan, **kw):
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused first
    base = dict(plan=the_plan.handle, n_rows=5, rows_per_draw=2, x=fake, z=fake, eps=fake, params=fake,
                mean_logits=fake)
    base.update(kw)
    return lib_mod.PredictScoresReq(**base)


def test_predict_scores_argument_checks():
    from psvi.runtime import InnerLoopPlan, _lib

    lib = _lib.load()
    call = lambda r: lib.psvi_predict_scores(ctypes.byref(r), None)
    plan = InnerLoopPlan("meanfield", [(5, 4), (4, 3)], 3, 7)
    fake = ctypes.c_void_p(0x1000)
    assert lib.psvi_predict_scores(None, None) == EINVAL
    assert call(_req(_lib, plan, plan=None)) == EINVAL
    for bad in (dict(n_rows=0), dict(rows_per_draw=0), dict(x=None), dict(eps=None),
                dict(params=None), dict(mean_logits=None),
                dict(last_acc=fake), dict(last_acc=fake, forgetting=fake),
                dict(z=None, el2n=fake), dict(z=None, correct=fake), dict(z=None, stats_out=fake),
                dict(z=None, last_acc=fake, forgetting=fake, never_learnt=fake)):
        assert call(_req(_lib, plan, **bad)) == EINVAL, bad
        assert lib.psvi_last_error()
    for fam, layers, kw in (("fullcov", [(5, 3)], {}), ("lenet", None, {}),
                            ("meanfield", [(5, 4), (4, 1)], dict(likelihood=("gaussian", 2.0))),
                            ("meanfield", [(5, 4), (4, 1)], dict(likelihood="bernoulli")),
                            ("meanfield", [(5, 4), (4, 3)], dict(world=2, rank=1))):
        layers = layers or [(25, 6), (150, 16), (400, 120), (120, 84), (84, 10)]
        p = InnerLoopPlan(fam, layers, 4, 7, **kw)
        assert call(_req(_lib, p)) == ESTATE, fam
    # PSVI_EUNSUP (one unit's weights and one row beyond the 160 KiB of LDS) needs a
    # layer that plan creation itself refuses today, with the same code
    with pytest.raises(_lib.PsviError, match="PSVI_EUNSUP"):
        InnerLoopPlan("meanfield", [(30000, 2)], 1, 1)
    # a valid request gets as far as the device check (or runs, on a GPU machine)
    if not torch.cuda.is_available():
        assert call(_req(_lib, plan)) == ESTATE


def test_wrapper_checks():
    from psvi.runtime import InnerLoopPlan, predict_scores

    plan = InnerLoopPlan("meanfield", [(5, 4), (4, 3)], 3, 7)
    x = torch.zeros(4, 5)
    with pytest.raises(ValueError, match="unknown outputs"):
        predict_scores(plan, x, None, x, x, 2, want=("margin",))
    with pytest.raises(ValueError, match="rows_per_draw"):
        predict_scores(plan, x, None, x, x, 0)
    with pytest.raises(ValueError, match="device tensor"):
        predict_scores(plan, x, None, x, x, 2)
    with pytest.raises(ValueError):
        predict_scores(None, x, None, x, x, 2)


def test_predict_query_reports_the_tiles():
    """psvi_predict_query: a small net runs every layer in one tile; 64 rows of
    350 inputs leave a tile 28 of the first layer's 50 units (whole groups of
    four, the tile's rows and biases within tile_floats); its refusals."""
    from psvi.runtime import InnerLoopPlan, _lib, predict_query

    lib = _lib.load()
    small = InnerLoopPlan("meanfield", [(5, 4), (4, 3)], 3, 7)
    assert predict_query(small, 1) == dict(rows_per_group=1, tile_floats=24, units_per_tile=[4, 3])
    assert predict_query(small, 100)["rows_per_group"] == 50      # even shares of at most 64 rows
    wide = InnerLoopPlan("meanfield", [(350, 50), (50, 3)], 2, 3)
    q = predict_query(wide, 64)
    assert q["rows_per_group"] == 64 and q["units_per_tile"] == [28, 3]
    assert q["tile_floats"] == 28 * 351
    assert predict_query(wide, 1)["units_per_tile"] == [50, 3]
    out = (ctypes.c_int64 * 10)()
    assert lib.psvi_predict_query(None, 1, out) == EINVAL
    assert lib.psvi_predict_query(small.handle, 1, None) == EINVAL
    assert lib.psvi_predict_query(small.handle, 0, out) == EINVAL
    assert lib.psvi_predict_query(InnerLoopPlan("fullcov", [(5, 3)], 4, 7).handle, 1, out) == ESTATE
    with pytest.raises(ValueError):
        predict_query(None, 1)


def test_header_and_request_struct_agree():
    from psvi.runtime import _lib

    h = open(os.path.join(ROOT, "include", "psvi_hip.h")).read()
    assert re.search(r"\bint psvi_predict_scores\(const psvi_predict_scores_req\* req, void\* stream\);", h)
    body = re.search(r"typedef struct psvi_predict_scores_req \{(.*?)\} psvi_predict_scores_req;", h,
                     re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r".*[ *]", "", v.strip()) for decl in body.split(";") if decl.strip()
              for v in decl.split(",")]
    assert fields == [n for n, _ in _lib.PredictScoresReq._fields_]
    assert _lib.SIGNATURES["psvi_predict_scores"][1][0]._type_ is _lib.PredictScoresReq


class _Rows(torch.utils.data.Dataset):
    def __init__(self, x, y):
        self.data, self.targets = x, y

    def __len__(self):
        return len(self.data)

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


def _toy(n=23, nc=3):
    g = torch.Generator().manual_seed(0)
    return _Rows(torch.randn(n, 2, generator=g), (torch.arange(n) % nc).float())


def test_weighted_subset_items():
    from torch.utils.data import DataLoader

    from psvi.inference.utils import WeightedSubset

    ds = _toy()
    ws = WeightedSubset(ds, [4, 9, 2], torch.tensor([1.5, 2.5, 3.5]))
    idx, data, target, wt = ws[1]
    assert idx == 1 and torch.equal(data, ds.data[9]) and target == ds.targets[9] and wt == 2.5
    assert len(ws) == 3
    (bi, bx, by, bw), = list(DataLoader(ws, batch_size=128))
    assert bi.tolist() == [0, 1, 2] and torch.equal(bx, ds.data[[4, 9, 2]])
    assert bw.tolist() == [1.5, 2.5, 3.5]
    with pytest.raises(AssertionError):
        WeightedSubset(ds, [1, 2], torch.ones(3))


def test_per_class_split(monkeypatch):
    from psvi.inference.utils import RandomSelection, ScoreSelection

    ds = _toy(23, 3)
    sel = ScoreSelection(ds, 11, 3, 0, score_type="entropy")
    score = torch.arange(23.0)
    monkeypatch.setattr(sel, "_get_uncertainty_score", lambda: score)
    idx = sel.select()
    y = ds.targets.numpy()
    assert [int((y[idx] == c).sum()) for c in range(3)] == [3, 3, 5] == R.class_split(11, 3)
    assert idx == R.select(score.numpy(), y, 11, 3)
    assert idx[:3] == [21, 18, 15]  # the largest scores of class 0, in order
    np.random.seed(0)
    ridx = RandomSelection(ds, 7, 3, 0).select()
    assert len(set(ridx)) == 7 and [int((y[ridx] == c).sum()) for c in range(3)] == [2, 2, 3]
    with pytest.raises(ValueError):
        ScoreSelection(ds, 4, 3, 0, score_type="margin")
    # get_weighted_subset: permuted with numpy's generator, weights n_train / n_coreset
    np.random.seed(5)
    perm = list(np.random.permutation(idx))
    np.random.seed(5)
    sub = sel.get_weighted_subset()
    assert sel.core_idc == perm and sorted(sel.core_idc) == sorted(idx)
    assert torch.equal(sel.wt_vec, 23 / 11 * torch.ones(11)) and len(sub) == 11
    assert sub[0][0] == 0 and torch.equal(sub[0][1], ds.data[perm[0]])


def test_forgetting_through_coreset_select_is_all_zero(monkeypatch):
    """Selection.pretrain passes forgetting_flag=, which MeanFieldVI swallows:
    no events are counted and top-k picks among equal (zero) scores."""
    import psvi.inference.utils as U

    seen = {}

    def fake_run(self):
        seen["flag"] = self.forgetting_score_flag
        self.forgetting_events = torch.zeros(len(self.train_dataset))
        self.net = None

    monkeypatch.setattr(U.MeanFieldVI, "run", fake_run)
    ds = _toy(23, 3)
    cs = U.CoresetSelect(train_dataset=ds, test_dataset=ds, num_pseudo=6, nc=3, architecture="fn",
                         D=2, n_hidden=4, score_method="forgetting", loaded_from_psvi=False)
    cs.select_data()
    assert seen["flag"] is False
    # equal scores: each class's rows as torch.topk orders a constant vector
    y = ds.targets.numpy()
    want = []
    for c in range(3):
        idx_c = np.arange(23)[y == c]
        want += idx_c[torch.topk(torch.zeros(len(idx_c)), 2).indices.numpy()].tolist()
    assert sorted(int(k) for k in cs.wt_index) == sorted(want)
    assert np.allclose(list(cs.wt_index.values()), 23 / 6)
    idx, _, _, wt = cs.chosen_dataset[0]
    assert idx == 0 and abs(float(wt) - 23 / 6) < 1e-6
    assert U.MeanFieldVI(forgetting_score_flag=True, architecture="fn").forgetting_score_flag


def test_csv_fallback(tmp_path, monkeypatch):
    from psvi.inference.utils import ScoreSelection

    ds = _toy(9, 3)
    computed = torch.arange(9.0)
    sel = ScoreSelection(ds, 3, 3, 1, score_type="entropy", data_folder=str(tmp_path), dnm="toy",
                         loaded=True)
    monkeypatch.setattr(sel, "_get_uncertainty_score", lambda: computed)
    assert sel.select() == [6, 7, 8]  # no file: computed (and saved)
    assert np.allclose(np.loadtxt(tmp_path / "entropy_toy_10_1.csv"), computed.numpy())
    with open(tmp_path / "score_psvi_toy_1.csv", "w") as fh:
        fh.write("least_confidence,entropy\n" + "\n".join(f"0.5,{9 - i}" for i in range(9)) + "\n")
    assert sel.select() == [0, 1, 2]  # the file's entropy column
    # no folder: nothing read or written
    sel = ScoreSelection(ds, 3, 3, 1, score_type="entropy", data_folder=None, loaded=True)
    monkeypatch.setattr(sel, "_get_uncertainty_score", lambda: computed)
    assert sel.select() == [6, 7, 8]


def test_refusals_name_the_missing_piece():
    from psvi.inference.baselines import MfviSelect, run_selection_with_mfvi
    from psvi.inference.utils import CoresetSelect, MeanFieldVI

    ds = _toy()
    for m in ("kmeans", "kmeans_gradient", "submodular", "weighted_kmeans", "scored_kmeans_el2n",
              "scored_kmeans_forgetting", "scored_kmeans_entropy", "scored_kmeans_least_confidence"):
        with pytest.raises(NotImplementedError, match="k-means|submodular"):
            CoresetSelect(train_dataset=ds, test_dataset=ds, score_method=m, architecture="fn",
                          nc=3).select_data()
    with pytest.raises(ValueError):
        CoresetSelect(train_dataset=ds, test_dataset=ds, score_method="margin", architecture="fn",
                      nc=3).select_data()
    with pytest.raises(NotImplementedError, match="incremental"):
        run_selection_with_mfvi(train_dataset=ds, test_dataset=ds, mfvi_selection_method="incremental")
    with pytest.raises(NotImplementedError, match="lenet"):
        MfviSelect(train_dataset=ds, test_dataset=ds, architecture="lenet")
    with pytest.raises(NotImplementedError, match="lenet"):
        MeanFieldVI(architecture="lenet")
    with pytest.raises(NotImplementedError, match="log_pseudodata"):
        MfviSelect(train_dataset=ds, test_dataset=ds, architecture="fn", log_pseudodata=True)


def test_driver_table():
    """"mfvi_selection" is the extended driver's (psvi_experiments.py) method: it
    sits in extended_inf_dict, which experiment_driver also reads; inf_dict
    stays flow_psvi.py's table."""
    import psvi.inference as I
    from psvi.experiments import experiment_driver, extended_inf_dict, inf_dict
    from psvi.inference.baselines import run_selection_with_mfvi

    assert extended_inf_dict["mfvi_selection"] is run_selection_with_mfvi
    assert I.run_selection_with_mfvi is run_selection_with_mfvi
    assert "mfvi_selection" not in inf_dict
    with pytest.raises(NotImplementedError, match="el2n_ensemble"):
        experiment_driver(["halfmoon"], ["el2n_ensemble"], dict(test_ratio=0.2), write=False)
