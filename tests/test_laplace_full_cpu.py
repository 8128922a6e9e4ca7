"""The full-precision Laplace posterior without a GPU: the fp64 restatement
(laplace_full_util) against the reference-generated fixtures s1-s3, the C
header's declaration and its ctypes mirror, the host functions' imports and the
public sparsevi / opsvi keyword that stays closed."""
import os
import re

import numpy as np
import pytest
import torch

from golden_util import load_fixture
import laplace_full_util as F
import laplace_util as U

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
S1 = ["s1_full_nu0_d5", "s1_full_nu1_d2", "s1_full_nu5_d3", "s1_full_nu40_d17",
      "s1_full_nu100_d65", "s1_full_nu300_d128", "s1_full_nu40_d17_w1e4"]


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    err = np.abs(a - b).max()
    assert err <= tol * np.abs(b).max(), err


def _restate(f):
    c = f["cfg"]
    x, w, theta = U.t64(f["x"]), U.t64(f["w"]), U.t64(f["theta"])
    P = F.precision_full(theta, x, w)
    A = F.reverse_cholesky(P)
    return P, A, F.samples_full(theta, A, U.t64(f["eps"]).reshape(c["S"], c["d"])), F.logdet(A)


@pytest.mark.parametrize("name", S1)
def test_restatement_matches_reference(name):
    f = load_fixture(name)
    c = f["cfg"]
    P, A, smp, ld = _restate(f)
    _close(P, f["prec64"])
    _close(A, f["factor64"])
    _close(smp, f["samples64"])
    assert abs(float(ld) - float(f["logdet64"][0])) <= 1e-12
    # A^-1 is the scale_tril MultivariateNormal(precision_matrix=P) holds
    eye = torch.eye(c["d"], dtype=torch.float64)
    _close(torch.linalg.solve_triangular(A, eye, upper=False), f["scale_tril64"])
    assert not torch.triu(A, 1).any()
    assert c["n_zero"] == c["Nu"] // 4 == int((f["w"] == 0).sum())
    if c["Nu"] == 0:
        assert np.array_equal(f["prec64"], np.eye(c["d"])) and f["logdet64"][0] == 0
        assert np.array_equal(smp.numpy(), f["theta"].astype(np.float64)
                              + f["eps"].astype(np.float64).reshape(c["S"], c["d"]))


def test_fixture_cases():
    cfgs = [load_fixture(n)["cfg"] for n in S1]
    assert [(c["Nu"], c["d"], c["S"]) for c in cfgs] == [(0, 5, 4), (1, 2, 1), (5, 3, 8), (40, 17, 8),
                                          (100, 65, 8), (300, 128, 8), (40, 17, 8)]
    assert load_fixture(S1[-1])["w"].max() > 1e4


def test_restated_run_laplace_matches_reference():
    f = load_fixture("s2_run_laplace_full")
    c = f["cfg"]
    assert (c["T"], c["Nu"], c["d"]) == (10, 5, 3)
    x, y, w = U.t64(f["x"]), U.t64(f["y"]), U.t64(f["w"])
    theta, smp = F.fit_sample(U.t64(f["theta0"]), x, y, w, c["T"], c["lr"],
                              U.t64(f["eps"]).reshape(c["S"], c["d"]), diagonal=False)
    _close(theta, f["theta64"])
    _close(F.precision_full(theta, x, w), f["prec64"])
    _close(smp, f["samples64"])
    assert np.abs(f["theta32"] - f["theta64"]).max() == c["gap"] < 0.5 * c["lr"]


@pytest.mark.parametrize("method", ["sparsevi", "opsvi"])
def test_whole_run_fixtures_have_clear_margins(method):
    f = load_fixture(f"s3_run_{method}_full")
    c = f["cfg"]
    assert c["diagonal"] is False
    assert c["gap"] > 100 * 4 * c["tol_corr"] and c["top2"] > 100 * 4 * c["tol_corr"]
    q = load_fixture("q4_run_" + method)["cfg"]
    for k in ("N", "S", "B", "epochs", "inner_it", "outer_it", "num_pseudo", "log_every",
              "lr0net", "lr0v", "lr0u"):
        assert c[k] == q[k], k


def test_restated_sparsevi_follows_reference_step_for_step():
    f = load_fixture("s3_run_sparsevi_full")
    cores, ws = F.run_sparsevi(f, diagonal=False)
    assert cores[-1] == f["core_idcs"].tolist()
    assert [len(c) for c in cores] == f["core_sizes"].tolist()
    assert all(c == cores[-1][:len(c)] for c in cores)
    # the reference ran in fp32: within half a weight step at every epoch
    err = np.abs(ws.numpy() - f["w_steps"]).max()
    print("sparsevi max|dw|", err)
    assert err < 0.5 * f["cfg"]["lr0v"]
    # and the diagonal path attaches other weights: the fixture pins the full one
    _, wd = F.run_sparsevi(f, diagonal=True)
    assert np.abs(wd.numpy() - f["w_steps"]).max() > err


def test_restated_opsvi_follows_reference_step_for_step():
    f = load_fixture("s3_run_opsvi_full")
    c = f["cfg"]
    ws, us = F.run_opsvi(f, f["u0"], f["z"], diagonal=False)
    ew = np.abs(ws.numpy() - f["w_steps"]).max()
    eu = np.abs(us.numpy() - f["u_steps"]).max()
    print("opsvi max|dw|", ew, "max|du|", eu)
    assert ew < 0.5 * c["lr0v"] * c["N"] and eu < 0.5 * c["lr0u"]
    assert np.array_equal(f["w_steps"][-1], f["w"]) and np.array_equal(f["u_steps"][-1], f["u"])


def test_header_declares_the_entry_and_ctypes_mirrors_it():
    from psvi.runtime import _lib

    with open(os.path.join(ROOT, "include", "psvi_hip.h")) as fh:
        h = fh.read()
    name = "psvi_laplace_sample_full"
    assert re.search(r"\bint %s\(const %s_req\* req, void\* stream\);" % (name, name), h)
    body = re.search(r"typedef struct %s_req \{(.*?)\} %s_req;" % (name, name), h, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S).strip()
        if decl:
            fields += [re.sub(r".*[ *]", "", v.strip()) for v in decl.split(",")]
    assert fields == ["n_core", "d", "S", "x_core", "w_core", "theta", "eps", "prec_out",
                      "factor_out", "samples_out", "logdet_out"]
    assert fields == [n for n, _ in _lib.LaplaceSampleFullReq._fields_]
    assert "psvi_laplace_sample_full" in _lib.SIGNATURES
    # psvi_laplace_fit's request is untouched
    assert [n for n, _ in _lib.LaplaceFitReq._fields_][:4] == ["n_core", "d", "S", "T"]


def test_host_functions_import():
    import inspect

    from psvi.inference import run_laplace
    from psvi.runtime import laplace_sample_full

    p = inspect.signature(run_laplace).parameters
    assert list(p)[:4] == ["x_core", "y_core", "w_core", "theta"]
    assert p["diagonal"].default is True and p["inner_it"].default == 1000
    q = inspect.signature(laplace_sample_full).parameters
    assert list(q) == ["x_core", "w_core", "theta", "eps", "want_prec", "want_factor",
                       "want_logdet"]
    from psvi.inference import baselines as B

    for fn in (B._run_sparsevi, B._run_opsvi, B._Laplace.fit):
        assert inspect.signature(fn).parameters["diagonal"].default is True


def test_public_sparsevi_and_opsvi_keep_refusing_diagonal_false():
    from psvi.inference import run_opsvi, run_sparsevi

    kw = dict(x=torch.randn(4, 2), y=torch.tensor([0., 1., 1., 0.]), xt=torch.randn(3, 2),
              yt=torch.tensor([0., 1., 0.]), N=4, D=2, num_epochs=1)
    for fn in (run_sparsevi, run_opsvi):
        with pytest.raises(NotImplementedError, match="diagonal"):
            fn(diagonal=False, **kw)
