"""The full-precision Laplace posterior on the GPU: psvi_laplace_sample_full
against the reference-generated fixtures s1-s3 and, at the shape edges, against
the fp64 restatement (laplace_full_util, itself pinned to the fixtures on the
CPU).

Tolerances.  The kernel is fp64 inside and rounds each output to float once, so
against the reference's fp64 values on the same float inputs it must be at
least as close as the reference's own fp32 run: per output
max(gap32, 4 * 2^-24 * max |value|), gap32 recorded in the fixture, the floor
being float rounding of the output.  Against the restatement (fp64 on both
sides; the factorisation's own error is ~1e-15 x cond) only the floor applies.
A whole fit (s2) adds the Adam chain: 4 x the reference's own fp32-against-fp64
gap, as tests/test_hip_laplace.py takes for q1.  Whole runs (s3) take q4's
bounds: the same indices, weights within half a step.

Every call here goes through buffers with sentinels behind each output."""
import ctypes

import numpy as np
import pytest
import torch

from golden_util import load_fixture
import laplace_full_util as F
import laplace_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
S1 = ["s1_full_nu0_d5", "s1_full_nu1_d2", "s1_full_nu5_d3", "s1_full_nu40_d17",
      "s1_full_nu100_d65", "s1_full_nu300_d128", "s1_full_nu40_d17_w1e4"]
FLOOR = 4 * 2.0 ** -24
PAD, MARK = 64, -777.0


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _raw(x, w, theta, eps, want=("prec", "factor", "logdet"), samples=True):
    """psvi_laplace_sample_full through the C ABI with PAD sentinels behind
    every output: (rc, outputs on the host)."""
    from psvi.runtime import _lib

    d = int(np.asarray(theta).size)
    n_core = 0 if x is None else int(x.shape[0])
    S = 0 if eps is None else int(eps.shape[0])
    sizes = {"prec": d * d, "factor": d * d, "samples": S * d, "logdet": 1}
    on = set(want) | ({"samples"} if samples and S else set())
    buf = {k: torch.full((sizes[k] + PAD,), MARK, device=DEV,
                         dtype=torch.float64 if k == "logdet" else torch.float32) for k in on}
    X, W = (dev(x), dev(w)) if n_core else (None, None)
    TH, E = dev(theta), dev(eps) if S else None
    req = _lib.LaplaceSampleFullReq(
        n_core, d, S, _ptr(X), _ptr(W), _ptr(TH), _ptr(E),
        _ptr(buf.get("prec")), _ptr(buf.get("factor")), _ptr(buf.get("samples")),
        _ptr(buf.get("logdet")))
    rc = _lib.load().psvi_laplace_sample_full(
        ctypes.byref(req), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = {}
    for k, b in buf.items():
        b = b.cpu()
        assert (b[sizes[k]:] == MARK).all(), f"{k}: sentinel overwritten"
        out[k] = b[:sizes[k]].reshape({"prec": (d, d), "factor": (d, d), "samples": (S, d),
                                       "logdet": (1,)}[k])
    return rc, out


def _run(x, w, theta, eps, **kw):
    rc, out = _raw(x, w, theta, eps, **kw)
    assert rc == 0
    return out


def _structure(out):
    assert torch.equal(out["prec"], out["prec"].T)
    assert not torch.triu(out["factor"], 1).any()
    assert all(torch.isfinite(v).all() for v in out.values())


def _dev_of(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(got.double().numpy() - ref).max()), float(np.abs(ref).max())


@pytest.mark.parametrize("name", S1)
def test_matches_reference(name):
    from psvi.runtime import laplace_fit

    f = load_fixture(name)
    c = f["cfg"]
    eps = f["eps"].reshape(c["S"], c["d"])
    out = _run(f["x"], f["w"], f["theta"], eps)
    _structure(out)
    for k in ("prec", "factor", "samples", "logdet"):
        err, top = _dev_of(out[k], f[k + "64"])
        tol = max(c["gap32_" + k], FLOOR * top)
        print(name, k, "max dev", err, "tol", tol, "gap32", c["gap32_" + k])
        assert err <= tol, (k, err, tol)
    # the diagonal is the precision psvi_laplace_fit reports at the same theta
    Nu = c["Nu"]
    fit = laplace_fit(dev(f["x"]) if Nu else None, torch.zeros(Nu, device=DEV) if Nu else None,
                      dev(f["w"]) if Nu else None, dev(f["theta"]), 0, 1e-3)
    diag = f["prec64"].diagonal()
    err, top = _dev_of(fit["prec"].cpu(), diag)
    assert err <= max(c["gap32_prec"], FLOOR * top)
    err = float((out["prec"].diagonal().double() - fit["prec"].cpu().double()).abs().max())
    assert err <= max(c["gap32_prec"], FLOOR * top)


def _problem(Nu, d, S, seed, wzero=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.cat((torch.randn(Nu, d - 1, generator=g), torch.ones(Nu, 1)), dim=1)
    w = torch.zeros(Nu) if wzero else 0.5 + 2 * torch.rand(Nu, generator=g)
    theta = torch.randn(d, generator=g) / d ** 0.5
    eps = torch.randn(S, d, generator=g)
    return x.numpy(), w.numpy(), theta.numpy(), eps.numpy()


def _against_restatement(x, w, theta, eps, out):
    P = F.precision_full(U.t64(theta), U.t64(x), U.t64(w))
    A = F.reverse_cholesky(P)
    ref = {"prec": P, "factor": A, "logdet": F.logdet(A).reshape(1)}
    if len(eps):
        ref["samples"] = F.samples_full(U.t64(theta), A, U.t64(eps))
    for k, r in ref.items():
        if k in out:
            err, top = _dev_of(out[k], r.numpy())
            assert err <= FLOOR * top, (k, err, FLOOR * top)


@pytest.mark.parametrize("Nu,wzero", [(0, False), (9, True)])
def test_no_likelihood_term_leaves_the_prior(Nu, wzero):
    """n_core == 0 and all weights zero: P = I, samples = theta + eps bitwise."""
    x, w, theta, eps = _problem(Nu, 5, 7, 11, wzero)
    out = _run(x if Nu else None, w if Nu else None, theta, eps)
    assert torch.equal(out["samples"], torch.tensor(theta) + torch.tensor(eps))
    assert out["logdet"].item() == 0.0
    assert torch.equal(out["prec"], torch.eye(5)) and torch.equal(out["factor"], torch.eye(5))


@pytest.mark.parametrize("Nu,d,S", [(257, 2, 3), (7, 3, 300), (33, 128, 260), (600, 64, 2)])
def test_edge_shapes_against_restatement(Nu, d, S):
    """More rows than threads, more samples than threads, more samples than
    columns that fit in LDS at d = 128, and an even dimension."""
    prob = _problem(Nu, d, S, 100 * Nu + d + S)
    out = _run(*prob)
    _structure(out)
    _against_restatement(*prob, out)


def test_precision_only():
    """S = 0 with prec_out alone."""
    x, w, theta, _ = _problem(12, 6, 0, 5)
    out = _run(x, w, theta, None, want=("prec",))
    assert set(out) == {"prec"} and torch.equal(out["prec"], out["prec"].T)
    _against_restatement(x, w, theta, np.zeros((0, 6)), out)


def test_wrapper_and_bitwise_repeat():
    from psvi.runtime import laplace_sample_full

    x, w, theta, eps = _problem(100, 65, 70, 3)
    call = lambda: laplace_sample_full(dev(x), dev(w), dev(theta), eps=dev(eps), want_prec=True,
                                       want_factor=True, want_logdet=True)
    a, b = call(), call()
    assert set(a) == {"samples", "prec", "factor", "logdet"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    raw = _run(x, w, theta, eps)
    for k in a:
        assert torch.equal(a[k].cpu(), raw[k]), k
    bare = laplace_sample_full(dev(x), dev(w), dev(theta), eps=dev(eps))
    assert bare["prec"] is None and bare["factor"] is None and bare["logdet"] is None
    assert torch.equal(bare["samples"], a["samples"])
    assert laplace_sample_full(None, None, dev(theta), want_prec=True)["samples"] is None


def test_out_of_range_arguments_return_einval():
    from psvi.runtime import PsviError, _lib, laplace_sample_full

    def call(Nu=3, d=3, S=2, w=None):
        x, w0, theta, eps = _problem(Nu, d, S, 3)
        return laplace_sample_full(dev(x) if Nu else None,
                                   dev(w0 if w is None else w) if Nu else None, dev(theta),
                                   eps=dev(eps) if S else None)

    call()
    bad = [lambda: call(d=1), lambda: call(d=129), lambda: call(S=2049), lambda: call(Nu=4097),
           lambda: call(w=np.array([1.0, -1e-3, 1.0], np.float32)),
           lambda: call(w=np.array([1.0, np.nan, 1.0], np.float32))]
    for i, fn in enumerate(bad):
        with pytest.raises(PsviError, match=r"PSVI_EINVAL\): \S") as e:
            fn()
            pytest.fail(f"case {i} was accepted")
        print(i, e.value)
    # S > 0 with NULL samples_out
    x, w, theta, eps = _problem(3, 3, 2, 3)
    rc, _ = _raw(x, w, theta, eps, want=("prec",), samples=False)
    assert rc == -1 and b"samples_out" in _lib.load().psvi_last_error()


def test_run_laplace_full_matches_reference():
    from psvi.inference import run_laplace

    f = load_fixture("s2_run_laplace_full")
    c = f["cfg"]
    theta = dev(f["theta0"])
    flat = torch.tensor(f["eps"])
    smp = run_laplace(dev(f["x"]), dev(f["y"]), dev(f["w"]), theta, inner_it=c["T"],
                      lr0net=c["lr"], diagonal=False, mc_samples=c["S"],
                      noise_source=lambda n: flat[:n])
    et = np.abs(theta.cpu().numpy() - f["theta64"]).max()
    es, top = _dev_of(smp.cpu(), f["samples64"])
    tol = max(4 * c["gap32_samples"], 4 * c["gap"], FLOOR * top)
    print("run_laplace full: max|dtheta|", et, "4 x gap", 4 * c["gap"], "samples dev", es,
          "tol", tol)
    assert smp.shape == (c["S"], c["d"])
    assert et <= 4 * c["gap"] and es <= tol
    # the diagonal path gives other samples from the same draws
    th2 = dev(f["theta0"])
    diag = run_laplace(dev(f["x"]), dev(f["y"]), dev(f["w"]), th2, inner_it=c["T"],
                       lr0net=c["lr"], mc_samples=c["S"], noise_source=lambda n: flat[:n])
    assert torch.equal(th2, theta) and (diag - smp).abs().max() > 100 * tol


class _Stream:
    def __init__(self, flat):
        self.flat, self.o = torch.tensor(flat), 0

    def take(self, n):
        out = self.flat[self.o:self.o + n]
        assert out.numel() == n, "draw stream exhausted"
        self.o += n
        return out


@pytest.mark.parametrize("method", ["sparsevi", "opsvi"])
def test_whole_run_replays_reference(method):
    from psvi.inference import baselines as B

    f = load_fixture(f"s3_run_{method}_full")
    c = f["cfg"]
    assert c["gap"] > 100 * 4 * c["tol_corr"] and c["top2"] > 100 * 4 * c["tol_corr"]
    st, batches, state = _Stream(f["draws"]), iter(f["batches"]), {}
    kw = dict(x=torch.tensor(f["x"]), y=torch.tensor(f["y"]), xt=torch.tensor(f["xt"]),
              yt=torch.tensor(f["yt"]), mc_samples=c["S"], data_minibatch=c["B"],
              num_epochs=c["epochs"], log_every=c["log_every"], seed=c["seed"],
              lr0net=c["lr0net"], inner_it=c["inner_it"], diagonal=False, noise_source=st.take,
              batch_source=lambda: next(batches), state_out=state)
    if method == "sparsevi":
        res = B._run_sparsevi(outer_it=c["outer_it"], lr0v=c["lr0v"], **kw)
    else:
        res = B._run_opsvi(num_pseudo=c["num_pseudo"], lr0u=c["lr0u"], lr0v=c["lr0v"],
                           register_elbos=True, **kw)
    assert st.o == st.flat.numel() and next(batches, None) is None
    lr_w = c["lr0v"] * c["N"] if method == "opsvi" else c["lr0v"]
    print(method, "core", state["core_idcs"], "max|dw|", np.abs(state["w"] - f["w"]).max(),
          "max|dtheta|", np.abs(state["theta"] - f["theta"]).max(), "nlls", res["nlls"], f["nlls"])
    assert state["core_idcs"] == f["core_idcs"].tolist()
    assert res["csizes"] == f["csizes"].tolist()
    nt = len(f["yt"])
    assert np.array_equal(np.round(np.array(res["accs"]) * nt), np.round(f["accs"] * nt))
    assert np.allclose(res["nlls"], f["nlls"], rtol=1e-4)
    assert np.abs(state["w"] - f["w"]).max() < 0.5 * lr_w
    assert np.abs(state["theta"] - f["theta"]).max() < 0.5 * c["lr0net"]
    if method == "opsvi":
        assert np.abs(state["u"] - f["u"]).max() < 0.5 * c["lr0u"]
        assert np.array_equal(np.array(res["elbos"])[:, 0], f["elbos"][:, 0])
        assert np.abs(np.array(res["elbos"])[:, 1] - f["elbos"][:, 1]).max() <= \
            1e-4 * np.abs(f["elbos"][:, 1]).max()
