"""Sparse black-box VI without a GPU: the Bernoulli plan's host side, the
wiring of ``sparsebbvi``, the fp64 restatement of the new formulas against the
reference-generated fixtures s1-s3, and the build resources of the new
kernels."""
import ctypes
import os

import numpy as np
import pytest
import torch

from golden_util import load_fixture
import sbbvi_util as U
from test_build_resources import CSRC, HIPCC, _resources, _scratch_users


def _create(family, dims, S, M, world, kind):
    from psvi.runtime import _lib

    lib = _lib.load()
    d = _lib.NetDesc()
    d.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        d.dims[i] = v
    d.S, d.M, d.prior_sd = S, M, 1.0
    h = ctypes.c_void_p()
    lik = _lib.Likelihood(kind, 0.0)
    rc = lib.psvi_plan_create_lik(family, ctypes.byref(d), world, 0, ctypes.byref(lik),
                                  ctypes.byref(h))
    msg = lib.psvi_last_error().decode() if rc else ""
    return rc, msg, h, lib


def test_bernoulli_plan_counts_match_categorical():
    from psvi.runtime import InnerLoopPlan, _lib

    assert _lib.LIK_BERNOULLI == 2
    for layers in ([(3, 1)], [(3, 10), (10, 1)], [(2, 7), (7, 5), (5, 1)]):
        b = InnerLoopPlan("meanfield", layers, 5, 9, likelihood="bernoulli")
        c = InnerLoopPlan("meanfield", layers, 5, 9)
        assert b.likelihood == "bernoulli" and b.tau is None
        for k in ("param_count", "eps_count", "ws_bytes", "acc_count", "loop_ws_bytes",
                  "net_mchunks"):
            assert getattr(b, k) == getattr(c, k), k
    assert InnerLoopPlan("meanfield", [(3, 1)], 5, 9, likelihood=("bernoulli", None)).likelihood \
        == "bernoulli"


def test_bernoulli_plan_refusals():
    from psvi.runtime import _lib

    B = _lib.LIK_BERNOULLI
    for args, code in (((_lib.FAMILY_FULLCOV, [3, 10, 1], 3, 5, 1, B), -3),
                       ((_lib.FAMILY_LENET, [3, 10, 1], 3, 5, 1, B), -3),
                       ((_lib.FAMILY_MEANFIELD, [3, 10, 1], 4, 5, 2, B), -3),
                       ((_lib.FAMILY_MEANFIELD, [3, 10, 2], 3, 5, 1, B), -1)):
        rc, msg, h, _ = _create(*args)
        assert rc == code and msg and not h.value, (args, rc, msg)
    rc, _, h, lib = _create(_lib.FAMILY_MEANFIELD, [3, 10, 1], 3, 5, 1, B)
    assert rc == 0 and h.value
    lib.psvi_plan_destroy(h)


def test_sparsebbvi_is_wired():
    from psvi.experiments.flow_psvi import inf_dict
    from psvi.inference import run_sparsevi_with_bb_elbo

    assert inf_dict["sparsebbvi"] is run_sparsevi_with_bb_elbo
    with pytest.raises(NotImplementedError):
        run_sparsevi_with_bb_elbo(scatterplot_coreset=True)


def test_check_binary():
    from psvi.runtime import check_binary

    check_binary(torch.tensor([0., 1., 1.]))
    for bad in ([0., 2.], [0.5, 1.], [-1, 0]):
        with pytest.raises(ValueError):
            check_binary(torch.tensor(bad))


def _close(a, b, tol=1e-10):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    if a.size == 0:
        return
    assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1.0), np.abs(a - b).max()


@pytest.mark.parametrize("name", ["s1_elbo_nu0", "s1_elbo_nu5"])
def test_restated_elbo_matches_reference(name):
    f = load_fixture(name)
    c = f["cfg"]
    nkl, _ = U.sampled_kl(U.t64(f["params"]), c["layers"], U.t64(f["eps"]), c["S"])
    loss, grad = U.elbo(U.t64(f["params"]), c["layers"], U.t64(f["eps"]), c["S"], U.t64(f["u"]),
                        U.t64(f["z"]), U.t64(f["w"]))
    _close(nkl, f["nkl64"])
    _close(loss, f["loss64"])
    _close(grad, f["grad64"])


@pytest.mark.parametrize("name", ["s2_scores_nu0", "s2_scores_nu7"])
def test_restated_scores_match_reference(name):
    f = load_fixture(name)
    c = f["cfg"]
    rows, lab = np.concatenate((f["u"], f["xb"])), np.concatenate((f["z"], f["yb"]))
    ll = U.loglik(U.logits(U.t64(f["params"]), c["layers"], U.t64(f["eps"]), c["S"], U.t64(rows)),
                  U.t64(lab))
    _close(ll, f["ll64"])
    W, corr, corecorr = U.scores(U.t64(f["ll64"]), U.t64(f["nkl64"]), U.t64(f["w"]), c["Nu"],
                                 c["N"] / c["B"])
    _close(W, f["W64"])
    _close(corr, f["corr64"])
    _close(corecorr, f["corecorr64"])
    assert int(corr.argmax()) == c["argmax"]
    assert (c["Nu"] == 0 or bool(corr.max() > corecorr.max())) == c["attach"]
    assert np.abs(f["corr32"] - f["corr64"]).max() <= c["tol_corr"]
    # the reference's own decision is well clear of rounding
    assert c["gap"] > 100 * 4 * c["tol_corr"]


@pytest.mark.parametrize("name", ["s3_weights_nu7", "s3_weights_logreg"])
def test_restated_weight_objective_matches_reference(name):
    f = load_fixture(name)
    c = f["cfg"]
    P, E = U.t64(f["params"]), U.t64(f["eps"])
    rows, lab = np.concatenate((f["u"], f["xb"])), np.concatenate((f["z"], f["yb"]))
    ll = U.loglik(U.logits(P, c["layers"], E, c["S"], U.t64(rows)), U.t64(lab))
    nkl, _ = U.sampled_kl(P, c["layers"], E, c["S"])
    loss, gw = U.weight_objective(ll, nkl, U.t64(f["w"]), c["N"])
    _close(loss, f["loss64"])
    _close(gw, f["gradw64"])


@pytest.mark.parametrize("name", ["s4_run_logreg", "s4_run_fn"])
def test_whole_run_fixtures_have_clear_margins(name):
    c = load_fixture(name)["cfg"]
    assert c["gap"] > 100 * 4 * c["tol_corr"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_select_kernels_no_scratch_no_spills(tmp_path):
    src = os.path.join(CSRC, "kernels_select.hip")
    kernels = _resources(src, tmp_path)
    assert {k for k in kernels if "select_" in k}, kernels.keys()
    touching = _scratch_users(src, tmp_path)
    bad = {k: v for k, v in kernels.items()
           if (v.get("ScratchSize", 0) and k in touching)
           or (v.get("VGPRs Spill", 0) and v.get("Occupancy", 2) > 1)}
    assert not bad, bad


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_bernoulli_and_sampled_kl_kernels_present_and_clean(tmp_path):
    """The Bernoulli net_kernel instantiation (LIK = 2: ...ILi0ELi2EE...) and
    the sampled-KL kernels exist and use no scratch."""
    net = _resources(os.path.join(CSRC, "kernels_net.hip"), tmp_path)
    bern = [k for k in net if "net_kernel" in k and k.endswith("Li0ELi2EEEvNS_7NetArgsE")]
    assert len(bern) == 1, [k for k in net if "net_kernel" in k]
    assert net[bern[0]].get("ScratchSize", 0) == 0 and net[bern[0]].get("VGPRs Spill", 0) == 0
    mf = _resources(os.path.join(CSRC, "kernels_mf.hip"), tmp_path)
    nk = [k for k in mf if "mf_nkl" in k]
    assert len(nk) == 2, mf.keys()
    for k in nk:
        assert mf[k].get("ScratchSize", 0) == 0 and mf[k].get("VGPRs Spill", 0) == 0
