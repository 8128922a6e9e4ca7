"""Coreset draws and the continual-learning host logic, without a GPU.

  * the float64 restatement of psvi_coreset_draw (tests/coreset_draw_util.py)
    has the laws the header claims: frequencies proportional to the weights,
    distinct rows and the right first-draw marginal without replacement, no
    row of zero weight, equal keys ordered by the lower index;
  * the C boundary: the header declares the entry and its request struct, the
    binding lists it, and the host-side refusals return their codes with no
    device in sight;
  * PSVI takes the reference's keywords (this file's constructor test fails on
    a tree that still refuses them); weight_reset and increment_coreset
    reproduce the reference's results recorded in tests/golden/t1_*.npz; the
    combinations that stay unsupported raise NotImplementedError."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import coreset_draw_util as CD
from golden_util import load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "psvi_hip.h")


# ------------------------------------------------------------ the restatement
def _within(counts, p, n):
    """Each count within 5 sd of its binomial mean."""
    return (np.abs(counts - n * p) <= 5.0 * np.sqrt(n * p * (1.0 - p))).all()


@pytest.mark.parametrize("seed", [3, 2**40 + 5])
def test_replace_frequencies_follow_the_weights(seed):
    w = np.array([0.5, 0.0, 2.0, 1.0, 0.25, 3.0, 0.0], np.float32)
    n = 200_000
    idx, st = CD.replace(w, n, seed, 16)
    assert st == 0 and idx.min() >= 0 and idx.max() < 7
    counts = np.bincount(idx, minlength=7)
    assert counts[1] == 0 and counts[6] == 0
    assert _within(counts, w.astype(np.float64) / w.sum(dtype=np.float64), n)


def test_noreplace_is_distinct_and_first_draw_is_proportional():
    w = np.array([0.5, 0.0, 2.0, 1.0, 0.25, 3.0, 0.0], np.float32)
    p = w.astype(np.float64) / w.sum(dtype=np.float64)
    n_off = 20_000
    first = np.empty(n_off, np.int64)
    for k in range(n_off):
        idx, st = CD.noreplace(w, 5, 17, 8 * k)      # 8 words per draw: disjoint streams
        assert st == 0 and np.unique(idx).size == 5 and (w[idx] > 0).all()
        first[k] = idx[0]
    assert _within(np.bincount(first, minlength=7), p, n_off)
    assert CD.noreplace(w, 6, 17, 0)[1] == 3          # five positive weights only


def test_equal_keys_go_to_the_lower_index():
    M = 12
    w = np.full(M, 0.375, np.float32)
    words = CD.stream_words(5, 0, M).copy()
    words[9] = words[2] = words.min() // 2 + 1        # two equal words -> two equal keys
    idx, st, ks = CD.noreplace(w, M, 5, 0, words=words, detail=True)
    pos2, pos9 = int(np.nonzero(idx == 2)[0][0]), int(np.nonzero(idx == 9)[0][0])
    assert st == 0 and pos9 == pos2 + 1 and ks[pos2] == ks[pos9]
    assert (np.diff(ks) <= 0).all() and sorted(idx.tolist()) == list(range(M))


def test_restatement_statuses_and_consumed_lengths():
    assert CD.replace(np.array([1.0, -1.0], np.float32), 3, 0, 0)[1] == 1
    assert CD.replace(np.array([1.0, np.inf], np.float32), 3, 0, 0)[1] == 1
    assert CD.noreplace(np.array([np.nan, 1.0], np.float32), 1, 0, 0)[1] == 1
    assert CD.replace(np.zeros(4, np.float32), 3, 0, 0)[1] == 2
    assert (CD.replace(np.zeros(4, np.float32), 3, 0, 0)[0] == -1).all()
    assert CD.consumed(4096, 60_000, True) == 60_000 and CD.consumed(4095, 7, False) == 4096
    assert CD.consumed(10, 5, True) == 8
    # a draw is a prefix of a longer one, and the offset moves along one stream
    w = np.array([1, 2, 3, 4], np.float32)
    a, b = CD.replace(w, 64, 9, 0)[0], CD.replace(w, 32, 9, 32)[0]
    assert np.array_equal(a[32:], b) and np.array_equal(CD.replace(w, 7, 9, 0)[0], a[:7])


# --------------------------------------------------------------- the boundary
def test_header_and_binding_declare_the_draw():
    from psvi.runtime import _lib

    text = open(HEADER).read()
    m = re.search(r"typedef struct psvi_coreset_draw_req \{(.*?)\} psvi_coreset_draw_req;", text,
                  re.S)
    assert m, "request struct missing"
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    want = ["w", "M", "n", "mode", "seed", "offset", "rows", "D", "targets", "idx_out", "rows_out",
            "targets_out", "status_out"]
    assert names == want
    assert [f[0] for f in _lib.CoresetDrawReq._fields_] == want
    assert re.search(r"int psvi_coreset_draw\(const psvi_coreset_draw_req\* req, void\* stream\);",
                     text)
    assert "PSVI_DRAW_REPLACE" in text and "PSVI_DRAW_NOREPLACE" in text
    assert "lower index" in text           # the tie rule is part of the contract
    assert "psvi_coreset_draw" in _lib.SIGNATURES


def test_host_side_refusals_need_no_device():
    from psvi.runtime import _lib

    lib = _lib.load()
    buf = (ctypes.c_int32 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(**kw):
        a = dict(w=p, M=8, n=4, mode=_lib.DRAW_REPLACE, seed=1, offset=0, rows=None, D=0,
                 targets=None, idx_out=p, rows_out=None, targets_out=None, status_out=p)
        a.update(kw)
        return lib.psvi_coreset_draw(ctypes.byref(_lib.CoresetDrawReq(**a)), None)

    EINVAL, EUNSUP = -1, -3
    assert _lib.ERRORS[EINVAL] == "PSVI_EINVAL" and _lib.ERRORS[EUNSUP] == "PSVI_EUNSUP"
    for kw in (dict(w=None), dict(idx_out=None), dict(status_out=None), dict(offset=6),
               dict(n=0), dict(n=9, mode=_lib.DRAW_NOREPLACE), dict(n=2**24 + 1),
               dict(rows=p, D=2), dict(targets=p), dict(mode=2), dict(M=0)):
        assert call(**kw) == EINVAL, kw
        assert lib.psvi_last_error()
    assert call(M=4097) == EUNSUP
    assert call(M=4097, n=4097, mode=_lib.DRAW_NOREPLACE) == EUNSUP
    assert lib.psvi_coreset_draw(None, None) == EINVAL


# -------------------------------------------------------------- the host logic
def _dataset(n=40, classes=3, seed=0):
    from psvi.experiments.experiments_utils import SynthDataset

    g = torch.Generator().manual_seed(seed)
    return SynthDataset(torch.randn(n, 2, generator=g),
                        torch.arange(n) % classes)


def _kw(**extra):
    ds = _dataset()
    kw = dict(N=40, D=2, num_pseudo=8, nc=3, mc_samples=4, seed=0, train_dataset=ds,
              test_dataset=ds)
    kw.update(extra)
    return kw


def test_constructor_takes_the_reference_keywords():
    """Fails on a tree whose PSVI.__init__ still refuses the switches."""
    from psvi.inference import PSVI, PSVIAFixedU, PSVIAV

    ps = PSVI(**_kw(prune=True, prune_interval=2, prune_sizes=[4]))
    assert ps.prune and ps.prune_interval == 2 and ps.prune_sizes == [4]
    assert ps.num_pseudo == 8 and ps.v.numel() == 8
    ps = PSVIAFixedU(**_kw(prune=True, prune_interval=2, prune_sizes=[6, 4], reset=True,
                           reset_interval=3, retrain_on_coreset=True))
    assert ps.reset and ps.reset_interval == 3 and ps.retrain_on_coreset
    ps = PSVIAV(**_kw(increment=True, increment_interval=2, increment_sizes=[4, 6, 8]))
    assert ps.increment and ps.num_pseudo == 4 and ps.v.numel() == 4   # starts at sizes[0]
    plain = PSVI(**_kw())
    assert not (plain.prune or plain.increment or plain.reset or plain.retrain_on_coreset)


def test_unsupported_combinations_raise():
    from psvi.inference import (PSVI, PSVIAV, PSVI_regressor, PSVIAV_regressor, PSVIFixedU,
                                PSVILearnV)

    # a class that learns u cannot prune: the call and the run both say so
    for cls in (PSVI, PSVILearnV, PSVIAV):
        ps = cls(**_kw(prune=True, prune_interval=2, prune_sizes=[4]))
        with pytest.raises(NotImplementedError, match="PSVIFixedU / PSVIAFixedU"):
            ps.prune_coreset(4)
        with pytest.raises(NotImplementedError, match="PSVIFixedU / PSVIAFixedU"):
            ps.run_psvi(data_minibatch=8, num_epochs=1)
    with pytest.raises(NotImplementedError, match="learn_z"):
        PSVI(**_kw(increment=True, increment_interval=2, increment_sizes=[4, 6], learn_z=True))
    switches = (dict(prune=True, prune_interval=2, prune_sizes=[4]),
                dict(increment=True, increment_interval=2, increment_sizes=[4, 6]),
                dict(reset=True, reset_interval=2), dict(retrain_on_coreset=True))
    for sw in switches:
        with pytest.raises(NotImplementedError, match="world > 1"):
            PSVIFixedU(**_kw(world=2, comm=object(), **sw))
        for cls in (PSVI_regressor, PSVIAV_regressor):
            with pytest.raises(NotImplementedError, match="regressors"):
                cls(**_kw(nc=1, **sw))
    # a dataset without subset_where cannot be cut into tasks
    from torch.utils.data import TensorDataset

    ds = TensorDataset(torch.randn(12, 2), torch.arange(12) % 3)
    ps = PSVIAV(**_kw(increment=True, increment_interval=2, increment_sizes=[4, 6],
                      train_dataset=ds, test_dataset=ds))
    with pytest.raises(NotImplementedError, match="subset_where"):
        ps.run_psvi(data_minibatch=4, num_epochs=1)
    with pytest.raises(ValueError, match="prune_interval"):
        PSVIFixedU(**_kw(prune=True))


@pytest.mark.parametrize("arch", ["logreg", "fn", "fn2"])
def test_weight_reset_matches_the_reference(arch):
    """Same generator calls in the same order: the parameters after
    set_up_model + weight_reset agree to 1e-7; a full-covariance layer refuses
    the reset as the reference's does."""
    from psvi.inference import PSVI

    f = load_fixture("t1_reset_" + arch)
    cfg = f["cfg"]
    ps = PSVI(**_kw(nc=cfg["nc"], mc_samples=cfg["mc_samples"]))
    ps.device = torch.device("cpu")
    for k in ("logistic_regression", "architecture", "n_hidden", "n_layers", "init_sd"):
        setattr(ps, k, cfg[k])
    torch.manual_seed(cfg["seed"])
    ps.set_up_model()
    vec = lambda: nn.utils.parameters_to_vector(ps.model.parameters()).detach().numpy()
    assert np.abs(vec() - f["built"]).max() <= 1e-7
    if cfg["raises"]:
        with pytest.raises(NotImplementedError):
            ps.weight_reset()
        return
    ps.weight_reset()
    assert np.abs(vec() - f["after"]).max() <= 1e-7
    assert np.abs(f["after"] - f["built"]).max() > 1e-3      # the reset drew new means
    sd = [np.log1p(np.exp(p.detach().numpy())) for n, p in ps.model.named_parameters()
          if n.endswith("_sd")]
    assert all(np.allclose(s, cfg["init_sd"], rtol=1e-5) for s in sd)


@pytest.mark.parametrize("name", ["t1_increment", "t1_increment_av"])
def test_increment_coreset_matches_the_reference(name):
    from psvi import inference
    from psvi.experiments.experiments_utils import SynthDataset
    from torch.utils.data import DataLoader

    f = load_fixture(name)
    cfg = f["cfg"]
    ds = SynthDataset(torch.tensor(f["x"]), torch.tensor(f["y"]))
    ps = getattr(inference, cfg["cls"])(**_kw(
        num_pseudo=cfg["M"], train_dataset=ds, test_dataset=ds, increment=True,
        increment_interval=2, increment_sizes=[cfg["M"], cfg["to_size"]]))
    ps.device = torch.device("cpu")
    ps.u = torch.tensor(f["u0"]).requires_grad_(True)
    ps.z = torch.tensor(f["z0"])
    ps.v = torch.tensor(f["v0"]).requires_grad_(True)
    ps.init_args = "random"
    ps.train_loader = DataLoader(ds, batch_size=16, shuffle=False)
    ps.model = nn.Linear(2, 3)
    old = {k: getattr(ps, k, None) for k in ("optim_v", "optim_u", "optim_net", "optim_alpha")}
    torch.manual_seed(cfg["seed"])
    ps.increment_coreset(to_size=cfg["to_size"], lr0v=1e-2, lr0u=1e-3, lr0net=1e-3,
                         new_class=cfg["new_class"], increment_idx=1)
    assert ps.num_pseudo == cfg["num_pseudo"] == cfg["to_size"]
    assert np.array_equal(ps.v.detach().numpy(), f["v"])
    assert np.array_equal(ps.z.numpy(), f["z"])
    assert tuple(ps.u.shape) == tuple(f["u_shape"])
    assert np.array_equal(ps.u.detach().numpy()[:cfg["M"]], f["u0"])
    assert ps.u.requires_grad == cfg["u_requires_grad"]
    assert ps.v.requires_grad == cfg["v_requires_grad"]
    assert ps.optim_v.param_groups[0]["params"][0] is ps.v
    assert ps.optim_u.param_groups[0]["params"][0] is ps.u
    rebuilt = ["optim_v", "optim_u", "optim_net"] + (["optim_alpha"] if "AV" in cfg["cls"] else [])
    assert all(getattr(ps, k) is not old[k] for k in rebuilt)


def test_driver_forwards_the_switches(monkeypatch):
    from psvi.experiments import flow_psvi

    seen = {}

    def fake(**kw):
        seen.update(kw)
        return {}

    monkeypatch.setitem(flow_psvi.inf_dict, "psvi_alpha_fixed_u", fake)
    args = dict(mc_samples=4, num_epochs=1, data_minibatch=8, inner_it=1, trainer="nested",
                log_every=1, lr0u=1e-3, lr0net=1e-3, lr0v=1e-2, init_sd=1e-3, num_trials=1,
                coreset_sizes=[4], architecture="logreg", prune=True, prune_interval=3,
                prune_sizes=[3, 2], lr0joint=5e-3, test_ratio=0.2)
    flow_psvi.experiment_driver(["halfmoon"], ["psvi_alpha_fixed_u"], args, write=False)
    assert seen["prune"] is True and seen["prune_interval"] == 3 and seen["prune_sizes"] == [3, 2]
    assert seen["lr0joint"] == 5e-3 and seen["increment"] is False and seen["reset"] is False
    assert seen["retrain_on_coreset"] is False and seen["increment_sizes"] is None
