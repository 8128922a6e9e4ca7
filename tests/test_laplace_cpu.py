"""The Laplace coreset baselines without a GPU: the fp64 restatement
(laplace_util) against the reference-generated fixtures q1-q3, the fixtures'
margins, the host functions' argument checks, the wiring of ``random``,
``sparsevi`` and ``opsvi``, and the C header's declarations."""
import os
import re

import numpy as np
import pytest
import torch

from golden_util import load_fixture
import laplace_util as U

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
FITS = [f"q1_fit_T{T}_nu{Nu}" for T in (1, 10, 200) for Nu in (0, 5)]
RUNS = ["q4_run_random", "q4_run_sparsevi", "q4_run_opsvi"]


def _close(a, b, tol=1e-10):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    if a.size == 0:
        return
    assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1.0), np.abs(a - b).max()


@pytest.mark.parametrize("name", FITS)
def test_restated_fit_matches_reference(name):
    f = load_fixture(name)
    c = f["cfg"]
    x, y, w = U.t64(f["x"]), U.t64(f["y"]), U.t64(f["w"])
    theta, losses = U.fit(U.t64(f["theta0"]), x, y, w, c["T"], c["lr"])
    prec = U.precision(theta, x, w)
    _close(theta, f["theta64"])
    _close(losses[0], f["loss0_64"])
    _close(prec, f["prec64"])
    _close(U.samples(theta, prec, U.t64(f["eps"]).reshape(c["S"], c["d"])), f["samples64"])
    if c["Nu"] == 0:
        assert np.array_equal(f["prec64"], np.ones(c["d"]))
    # the reference's own fp32 run stays well inside half a step of the fp64 one
    assert np.abs(f["theta32"] - f["theta64"]).max() == c["gap"] < 0.5 * c["lr"]


def _ll(f):
    rows = U.t64(np.concatenate((f["xc"], f["xb"])))
    labels = U.t64(np.concatenate((f["yc"], f["yb"])))
    return U.ll_matrix(U.t64(f["samples"]), rows, labels)


@pytest.mark.parametrize("name", ["q2_scores_nu0", "q2_scores_nu7"])
def test_restated_scores_match_reference(name):
    f = load_fixture(name)
    c = f["cfg"]
    ll = _ll(f)
    _close(ll, f["ll64"])
    corr, corecorr, resid, _ = U.scores(ll, U.t64(f["w"]), c["Nu"], c["N"] / c["B"])
    _close(corr, f["corr64"])
    _close(corecorr, f["corecorr64"])
    _close(resid, f["resid64"])
    assert int(corr.argmax()) == c["argmax"]
    assert (c["Nu"] == 0 or bool(corr.max() > corecorr.max())) == c["attach"]
    assert np.abs(f["corr32"] - f["corr64"]).max() <= c["tol_corr"]
    # the reference's own decision and argmax are well clear of rounding
    assert c["gap"] > 100 * 4 * c["tol_corr"] and c["top2"] > 100 * 4 * c["tol_corr"]


def test_restated_weight_gradient_matches_reference():
    f = load_fixture("q3_gradw_nu7")
    c = f["cfg"]
    _, _, _, gw = U.scores(_ll(f), U.t64(f["w"]), c["Nu"], c["N"] / c["B"])
    _close(gw, f["gradw64"])


def test_restated_u_gradient_matches_reference_and_closed_form():
    f = load_fixture("q3_gradu_nu6")
    c = f["cfg"]
    smp, u, z, w = U.t64(f["samples"]), U.t64(f["xc"]), U.t64(f["yc"]), U.t64(f["w"])
    _, _, resid, _ = U.scores(_ll(f), w, c["Nu"], c["N"] / c["B"])
    g = U.grad_u(smp, u, z, w, resid)
    _close(g, f["gradu64"])
    _close(U.grad_u_closed(smp, u, z, w, resid), f["gradu64"])
    assert np.abs(f["gradu64"][:, :-1]).min() > 0 and not f["gradu64"][:, -1].any()


@pytest.mark.parametrize("name", RUNS)
def test_whole_run_fixtures_have_clear_margins(name):
    f = load_fixture(name)
    c = f["cfg"]
    assert c["gap"] > 100 * 4 * c["tol_corr"] and c["top2"] > 100 * 4 * c["tol_corr"]
    assert c["N"] <= 60 and 3 <= c["epochs"] <= 4 and c["inner_it"] <= 20
    assert c["outer_it"] == 2 and c["S"] <= 8 and c["B"] <= 20


def _xy(y=(0., 1., 1., 0.)):
    return dict(x=torch.randn(4, 2), y=torch.tensor(y), xt=torch.randn(3, 2),
                yt=torch.tensor([0., 1., 0.]), N=4, D=2, num_epochs=1)


def test_argument_checks():
    from psvi.inference import run_opsvi, run_random, run_sparsevi

    for fn in (run_random, run_sparsevi, run_opsvi):
        with pytest.raises(NotImplementedError, match="mcmc"):
            fn(mcmc=True, **_xy())
    for fn in (run_sparsevi, run_opsvi):
        with pytest.raises(NotImplementedError, match="diagonal"):
            fn(diagonal=False, **_xy())
    for fn in (run_random, run_sparsevi):
        for bad in ((0., 2., 1., 0.), (0.5, 1., 0., 1.)):
            with pytest.raises(ValueError):
                fn(**_xy(bad))


def test_process_wt_index():
    from psvi.inference import process_wt_index

    assert process_wt_index([[], [2, 0]], [[0., 0., 0.], [1.5, 0., 2.5]]) == \
        [{}, {2: 2.5, 0: 1.5}]


def test_methods_are_wired():
    from psvi.experiments.flow_psvi import inf_dict
    from psvi.inference import run_opsvi, run_random, run_sparsevi

    assert inf_dict["random"] is run_random
    assert inf_dict["sparsevi"] is run_sparsevi
    assert inf_dict["opsvi"] is run_opsvi
    assert "giga" not in inf_dict


def test_header_declares_the_entries():
    with open(os.path.join(ROOT, "include", "psvi_hip.h")) as fh:
        h = fh.read()
    for name in ("psvi_laplace_fit", "psvi_laplace_scores"):
        assert re.search(r"\bint %s\(const %s_req\* req, void\* stream\);" % (name, name), h)
        assert re.search(r"typedef struct %s_req \{" % name, h)


def test_request_structs_match_the_header():
    """The ctypes request structs list the header's fields in its order."""
    from psvi.runtime import _lib

    with open(os.path.join(ROOT, "include", "psvi_hip.h")) as fh:
        h = fh.read()
    for name, cls in (("psvi_laplace_fit_req", _lib.LaplaceFitReq),
                      ("psvi_laplace_scores_req", _lib.LaplaceScoresReq)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [v.strip(" *") for v in decl.split(",")]
                fields[-len(decl.split(",")):] = [re.sub(r".*[ *]", "", v)
                                                  for v in fields[-len(decl.split(",")):]]
        assert fields == [n for n, _ in cls._fields_], (fields, cls._fields_)
