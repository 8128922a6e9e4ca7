"""The GIGA baseline without a GPU: the fp64 restatement (giga_util) against the
reference-generated fixtures k1 / k2, the fixtures' margins, the wiring of
``run_giga`` and the C header's declaration of psvi_giga_step."""
import os
import re

import numpy as np
import pytest
import torch

from golden_util import load_fixture
import giga_util as G
import laplace_util as U

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
STEPS = ["k1_step_first", "k1_step_mid"]
RUNS = ["k2_run_log1", "k2_run_log2"]


def margins_hold(c):
    """What the generator searched its seeds for, from the recorded numbers."""
    return c["top2"] > 100 * 4 * c["tol_score"] and c["den"] > 100 * 4 * c["tol_score"]


@pytest.mark.parametrize("name", STEPS)
def test_restated_step_matches_reference(name):
    f = load_fixture(name)
    c = f["cfg"]
    assert margins_hold(c)
    assert (c["S"], c["n_data"], c["d"]) == (50, 32, 3)
    assert bool(f["lw_in"].any()) == (name == "k1_step_mid")
    ll = U.ll_matrix(U.t64(f["samples"]), U.t64(f["rows"]), U.t64(f["labels"]))
    assert np.abs(ll.numpy() - f["ll64"]).max() <= 1e-12
    r = G.step(ll, U.t64(f["lw_in"]))
    # the restatement is the fp64 run to rounding, so inside the fp32 run's gap
    assert np.abs(r["score"].numpy() - f["score64"]).max() <= 1e-9 + 1e-3 * c["tol_score"]
    assert r["n"] == c["argmax"] and int(f["sub"][r["n"]]) == int(f["pt_idx64"]) == int(f["pt_idx32"])
    for k in ("zeta0", "zeta1", "zeta2", "gamma", "scale"):
        assert abs(float(r[k]) - float(f[k + "64"])) <= 1e-10, k
    assert np.abs(r["lw"].numpy() - f["lw64"]).max() <= 1e-10
    w = G.weights(torch.zeros(c["N"], dtype=torch.float64), int(f["pt_idx64"]), r["gamma"],
                  r["scale"])
    assert np.abs(w.numpy() - f["w64"]).max() <= 1e-10
    assert G.top2_gap(r["score"], f["sub"]) == pytest.approx(c["top2"], rel=1e-6)
    assert abs(float(r["den"])) == pytest.approx(c["den"], rel=1e-6)
    # the recorded gaps are the reference's own fp32-against-fp64 differences
    assert np.abs(f["score32"] - f["score64"]).max() == c["tol_score"]
    assert abs(float(f["gamma32"]) - float(f["gamma64"])) == c["tol_gamma"]
    assert np.abs(f["lw32"] - f["lw64"]).max() == c["tol_lw"]


@pytest.mark.parametrize("name", RUNS)
def test_restated_run_reproduces_the_index_sequence(name):
    """The step needs data rows alone: the restatement, which never sees a core
    row, follows the reference's picks, gammas, lw and w through a whole run,
    also where the picked point is already in the core."""
    f = load_fixture(name)
    c = f["cfg"]
    assert margins_hold(c)
    assert (np.abs(f["top2s"]).min(), np.abs(f["dens"]).min()) == (c["top2"], c["den"])
    assert (np.abs(f["probs64"] - 0.5) > 100 * 4 * np.abs(f["probs32"] - f["probs64"])).all()
    assert (c["N"], c["D"], c["B"], c["subset_size"], c["epochs"]) == (200, 2, 32, 40, 6)
    x = np.concatenate((f["x"], np.ones((c["N"], 1), np.float32)), axis=1)
    smp = U.t64(f["samples"])
    lw = torch.zeros(c["S"], dtype=torch.float64)
    w = torch.zeros(c["N"], dtype=torch.float64)
    core, k = [], 0
    for it in range(c["epochs"]):
        if it % c["log_every"]:
            continue
        sub = f["batches"][it]
        assert int((w > 0).sum()) == f["csizes"][k]
        r = G.step(U.ll_matrix(smp, U.t64(x[sub]), U.t64(f["y"][sub])), lw)
        pt = int(sub[r["n"]])
        assert pt == f["pt_idx"][k]
        if pt not in core:
            core.append(pt)
        lw, w = r["lw"], G.weights(w, pt, r["gamma"], r["scale"])
        # fp32 samples here, the fp64 run's own there: within the fp32 run's gap
        assert abs(float(r["gamma"]) - f["gamma"][k]) <= 4 * c["tol_gamma"]
        assert np.abs(lw.numpy() - f["lw"][k]).max() <= 4 * c["tol_lw"]
        assert np.abs(w.numpy() - f["w"][k]).max() <= 4 * c["tol_w"]
        k += 1
    assert k == len(f["pt_idx"]) and core == f["core_idcs"].tolist()


def test_coreset_grows_on_logging_iterations_only():
    a, b = load_fixture("k2_run_log1"), load_fixture("k2_run_log2")
    assert a["cfg"]["seed"] == b["cfg"]["seed"] and np.array_equal(a["x"], b["x"])
    assert len(a["pt_idx"]) == 6 and len(b["pt_idx"]) == 3
    assert 2 * len(b["core_idcs"]) == len(a["core_idcs"])


def test_run_giga_is_wired():
    import psvi.inference as I
    from psvi.experiments.flow_psvi import inf_dict
    from psvi.inference.baselines import run_giga

    assert I.run_giga is run_giga
    # registering it in the driver waits on test_laplace_cpu.test_methods_are_wired
    assert sorted(inf_dict) == sorted([
        "psvi", "psvi_ablated", "psvi_learn_v", "psvi_alpha_v", "psvi_no_iw", "psvi_free_v",
        "psvi_no_rescaling", "psvi_fixed_u", "psvi_alpha_fixed_u", "mfvi", "mfvi_subset",
        "sparsebbvi", "random", "sparsevi", "opsvi"])
    with pytest.raises(NotImplementedError, match="mcmc"):
        run_giga(mcmc=True, x=torch.randn(4, 2), y=torch.tensor([0., 1., 1., 0.]),
                 xt=torch.randn(3, 2), yt=torch.tensor([0., 1., 0.]), N=4, D=2, num_epochs=1)


def test_header_and_request_struct_agree():
    from psvi.runtime import _lib

    with open(os.path.join(ROOT, "include", "psvi_hip.h")) as fh:
        h = fh.read()
    assert re.search(r"\bint psvi_giga_step\(const psvi_giga_step_req\* req, void\* stream\);", h)
    body = re.search(r"typedef struct psvi_giga_step_req \{(.*?)\} psvi_giga_step_req;", h,
                     re.S).group(1)
    fields = [re.sub(r".*[ *]", "", v.strip()) for decl in body.split(";") if decl.strip()
              for v in decl.split(",")]
    assert fields == [n for n, _ in _lib.GigaStepReq._fields_]
    assert _lib.SIGNATURES["psvi_giga_step"][1][0]._type_ is _lib.GigaStepReq
