"""The Laplace coreset baselines on the GPU: psvi_laplace_fit and
psvi_laplace_scores against the reference-generated fixtures q1-q4 and, at the
shape edges, against the fp64 restatement (laplace_util, itself pinned to the
fixtures on the CPU).

Tolerances: 1e-4 relative (the project's parity bound) for one step, the
precision, the samples, the objectives and the gradients; a longer fit within
4x the reference's own fp32-against-fp64 gap recorded in its fixture; corr /
corecorr within 4x the recorded gap too.  The kernels' sums are fp64 with
float outputs, so against the restatement applied to the GPU's own ll they
agree to float rounding (1e-6 relative)."""
import json

import numpy as np
import pytest
import torch

from golden_util import load_fixture, rel
import laplace_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _fit_fixture(f, want_loss=True):
    from psvi.runtime import laplace_fit

    c = f["cfg"]
    theta = dev(f["theta0"])
    out = laplace_fit(dev(f["x"]), dev(f["y"]), dev(f["w"]), theta, c["T"], c["lr"],
                      eps=dev(f["eps"]).reshape(c["S"], c["d"]), want_loss=want_loss)
    return theta.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items() if v is not None}


@pytest.mark.parametrize("name", ["q1_fit_T1_nu0", "q1_fit_T1_nu5"])
def test_one_step_matches_reference(name):
    f = load_fixture(name)
    theta, out = _fit_fixture(f)
    print(name, "theta rel", rel(theta, f["theta64"]), "loss rel", rel(out["loss"][0], f["loss0_64"]),
          "prec rel", rel(out["prec"], f["prec64"]), "samples rel",
          rel(out["samples"], f["samples64"]))
    assert rel(theta, f["theta64"]) < 1e-4
    assert rel(out["loss"][0], f["loss0_64"]) < 1e-4
    assert rel(out["prec"], f["prec64"]) < 1e-4
    assert rel(out["samples"], f["samples64"]) < 1e-4


@pytest.mark.parametrize("name", [f"q1_fit_T{T}_nu{Nu}" for T in (10, 200) for Nu in (0, 5)])
def test_longer_fit_within_the_references_own_gap(name):
    f = load_fixture(name)
    c = f["cfg"]
    assert c["gap"] < 0.5 * c["lr"]
    theta, out = _fit_fixture(f)
    err = np.abs(theta - f["theta64"]).max()
    print(name, "max|dtheta|", err, "4 x gap", 4 * c["gap"], "loss0 rel",
          rel(out["loss"][0], f["loss0_64"]))
    assert err <= 4 * c["gap"]
    assert rel(out["loss"][0], f["loss0_64"]) < 1e-4
    assert rel(out["prec"], f["prec64"]) < 1e-4
    assert rel(out["samples"], f["samples64"]) < 1e-4
    assert out["loss"].shape == (c["T"],) and np.isfinite(out["loss"]).all()


def _scores_fixture(f, **want):
    from psvi.runtime import laplace_scores

    c = f["cfg"]
    rows = dev(np.concatenate((f["xc"], f["xb"])))
    labels = dev(np.concatenate((f["yc"], f["yb"])))
    out = laplace_scores(dev(f["samples"]), rows, labels, dev(f["w"]) if c["Nu"] else None,
                         c["Nu"], c["N"] / c["B"], want_ll=True, **want)
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


@pytest.mark.parametrize("name", ["q2_scores_nu0", "q2_scores_nu7"])
def test_scores_match_reference(name):
    f = load_fixture(name)
    c = f["cfg"]
    sc = _scores_fixture(f)
    err = np.abs(sc["ll"] - f["ll64"])
    assert (err <= 1e-4 * np.abs(f["ll64"]) + 1e-6).all()
    tol = 4 * c["tol_corr"]
    assert c["gap"] > 100 * tol and c["top2"] > 100 * tol
    res = sc["result"].tolist()
    ec = np.abs(sc["corr"] - f["corr64"]).max()
    print(name, "ll max err", err.max(), "corr err", ec, "tol", tol)
    assert ec <= tol
    if c["Nu"]:
        ecc = np.abs(sc["corecorr"] - f["corecorr64"]).max()
        print(name, "corecorr err", ecc)
        assert ecc <= tol
        assert abs(res[2] - f["corecorr64"].max()) <= tol
    else:
        assert res[2] == -np.inf
    assert abs(res[0] - f["corr64"].max()) <= tol
    assert int(res[1]) == c["argmax"] and bool(res[3]) == c["attach"]


def test_weight_gradient_matches_reference():
    f = load_fixture("q3_gradw_nu7")
    sc = _scores_fixture(f, want_grad_w=True)
    print("grad_w rel", rel(sc["grad_w"], f["gradw64"]))
    assert rel(sc["grad_w"], f["gradw64"]) < 1e-4


def test_u_gradient_matches_reference():
    f = load_fixture("q3_gradu_nu6")
    sc = _scores_fixture(f, want_grad_w=True, want_grad_u=True)
    print("grad_u rel", rel(sc["grad_u"], f["gradu64"]), "grad_w rel",
          rel(sc["grad_w"], f["gradw64"]))
    assert rel(sc["grad_u"], f["gradu64"]) < 1e-4
    assert rel(sc["grad_w"], f["gradw64"]) < 1e-4
    assert not sc["grad_u"][:, -1].any()


# ---- shape edges: every entry twice, bit for bit, and against the restatement
def _problem(Nu, d, S, B, seed, labels=None, scale=1.0, w=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.cat((scale * torch.randn(Nu + B, d - 1, generator=g), torch.ones(Nu + B, 1)), dim=1)
    y = (torch.rand(Nu + B, generator=g) > 0.5).float() if labels is None \
        else torch.full((Nu + B,), float(labels))
    if w is None:
        w = 0.5 + 2 * torch.rand(Nu, generator=g)
    theta0 = torch.randn(d, generator=g) / d ** 0.5
    eps = torch.randn(S, d, generator=g)
    return x, y, w, theta0, eps


def _run_all(x, y, w, theta0, eps, Nu, T, lr, N):
    from psvi.runtime import laplace_fit, laplace_scores

    X, Y = dev(x), dev(y)
    W = dev(w) if Nu else None
    theta = dev(theta0)
    fit = laplace_fit(X[:Nu].contiguous() if Nu else None, Y[:Nu].contiguous() if Nu else None,
                      W, theta, T, lr, eps=dev(eps), want_loss=True)
    B = x.shape[0] - Nu
    sc = laplace_scores(fit["samples"], X, Y, W, Nu, N / B, want_grad_w=True, want_ll=True,
                        want_grad_u=True)
    out = dict(theta=theta, prec=fit["prec"], samples=fit["samples"], loss=fit["loss"], **sc)
    return {k: v.cpu() for k, v in out.items() if v is not None}


def _check_against_restatement(out, x, y, w, theta0, eps, Nu, T, lr, N):
    X, Y, W = U.t64(x), U.t64(y), U.t64(w)
    theta, losses = U.fit(U.t64(theta0), X[:Nu], Y[:Nu], W, T, lr)
    prec = U.precision(theta, X[:Nu], W)
    assert (out["theta"].double() - theta).abs().max() <= 1e-6 * max(theta.abs().max(), 1.0)
    assert rel(out["loss"], losses) < 1e-9
    assert rel(out["prec"], prec) < 1e-6
    assert rel(out["samples"], U.samples(theta, prec, U.t64(eps))) < 1e-6
    # the scores' own arithmetic: the restatement on the GPU's samples and ll
    smp = out["samples"].double()
    ll64 = U.ll_matrix(smp, X, Y)
    assert ((out["ll"].double() - ll64).abs() <= 1e-6 * ll64.abs() + 1e-7).all()
    B = x.shape[0] - Nu
    corr, corecorr, resid, gw = U.scores(out["ll"].double(), W, Nu, N / B)
    res = out["result"].tolist()
    assert rel(out["corr"], corr) < 1e-6
    assert corr[int(res[1])] >= corr.max() - 1e-6 * corr.max().abs()
    assert res[0] == pytest.approx(float(corr.max()), rel=1e-6)
    if Nu:
        assert rel(out["corecorr"], corecorr) < 1e-6
        assert res[2] == pytest.approx(float(corecorr.max()), rel=1e-6)
        # the flag follows the kernel's own maxima; against the restatement only
        # where the margin is clear of rounding (at S = 2 every |corr| ties)
        assert res[3] == float(res[0] > res[2])
        if abs(float(corr.max() - corecorr.max())) > 1e-6 * float(corr.abs().max()):
            assert res[3] == float(corr.max() > corecorr.max())
        assert rel(out["grad_w"], gw) < 1e-6
        gu = U.grad_u_closed(smp, X[:Nu], Y[:Nu], W, resid)
        assert (out["grad_u"].double() - gu).abs().max() <= 1e-6 * max(gu.abs().max(), 1e-30)
        assert not out["grad_u"][:, -1].any()
    else:
        assert res[3] == 1.0 and res[2] == -np.inf


def _twice(prob, Nu, T=3, lr=1e-2, N=40.0, check=True):
    a = _run_all(*prob, Nu, T, lr, N)
    b = _run_all(*prob, Nu, T, lr, N)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert all(torch.isfinite(v).all() for k, v in a.items() if k != "result")
    if check:
        _check_against_restatement(a, *prob, Nu, T, lr, N)
    return a


@pytest.mark.parametrize("B", [1, 13])
@pytest.mark.parametrize("S", [2, 3, 65])
@pytest.mark.parametrize("d", [2, 3, 65])
@pytest.mark.parametrize("Nu", [0, 1, 7, 65])
def test_edge_shapes_and_bitwise_repeat(Nu, d, S, B):
    _twice(_problem(Nu, d, S, B, 1000 * Nu + 100 * d + 10 * S + B), Nu)


def test_core_rows_read_from_global_memory():
    """Nu * d floats beyond the 160 KiB LDS budget: the fit reads x from global memory."""
    Nu, d = 700, 65
    assert 4 * Nu * (d | 1) + 8 * (2 * 256 + 256 + Nu) > 160 * 1024
    _twice(_problem(Nu, d, 3, 13, 5, scale=0.3), Nu, T=2, N=1400.0)


@pytest.mark.parametrize("label", [0, 1])
def test_constant_labels(label):
    _twice(_problem(7, 3, 3, 5, 7 + label, labels=label), 7)


def test_large_logits_are_overflow_safe():
    """Logits of +-40 in the fit and in the scores: sigmoid and softplus in
    their overflow-safe forms."""
    x = torch.tensor([[1.0, 1.0], [-1.0, 1.0], [1.0, 1.0], [-1.0, 1.0], [0.5, 1.0]])
    y = torch.tensor([1.0, 1.0, 0.0, 0.0, 1.0])
    prob = (x, y, torch.ones(4), torch.tensor([40.0, 0.0]), torch.zeros(3, 2)
            + torch.tensor([[0.0, 0.0], [1e-3, 0.0], [0.0, 1e-3]]))
    a = _twice(prob, 4, T=2, lr=1e-3)
    f = U.t64(x[:4]) @ a["theta"].double()
    assert f.abs().max().item() == pytest.approx(40.0, rel=1e-3)


def test_zero_weights():
    """A core with some zero weights fits as the core without those rows; with
    all weights zero the prior alone drives theta and the precision is exactly 1."""
    Nu, d, S, B = 7, 3, 3, 5
    x, y, w, theta0, eps = _problem(Nu, d, S, B, 21)
    w[1] = w[4] = 0.0
    a = _twice((x, y, w, theta0, eps), Nu)
    keep = [0, 2, 3, 5, 6]
    theta, _ = U.fit(U.t64(theta0), U.t64(x[keep]), U.t64(y[keep]), U.t64(w[keep]), 3, 1e-2)
    assert (a["theta"].double() - theta).abs().max() <= 1e-6
    z = _twice((x, y, torch.zeros(Nu), theta0, eps), Nu)
    e = _twice((x[Nu:], y[Nu:], torch.zeros(0), theta0, eps), 0)
    assert torch.equal(z["prec"], torch.ones(d)) and torch.equal(e["prec"], torch.ones(d))
    assert torch.equal(z["theta"], e["theta"]) and torch.equal(z["samples"], e["samples"])


def test_out_of_range_arguments_return_einval():
    from psvi.runtime import PsviError, laplace_fit, laplace_scores

    def fit(Nu=3, d=3, S=2, T=1, lr=1e-2, w=None, **kw):
        x, y, w0, theta0, eps = _problem(Nu, d, S, 1, 3)
        return laplace_fit(dev(x[:Nu]) if Nu else None, dev(y[:Nu]) if Nu else None,
                           dev(w0 if w is None else w) if Nu else None, dev(theta0), T, lr,
                           eps=dev(eps), **kw)

    def scores(Nu=3, d=3, S=2, B=2):
        x, y, w, _, eps = _problem(Nu, d, S, B, 4)
        return laplace_scores(dev(eps), dev(x), dev(y), dev(w) if Nu else None, Nu, 2.0)

    fit(), scores()
    bad = [lambda: fit(d=1), lambda: fit(d=257), lambda: fit(Nu=4097), lambda: fit(S=2049),
           lambda: fit(T=-1), lambda: fit(T=(1 << 20) + 1), lambda: fit(lr=0.0),
           lambda: fit(lr=float("nan")), lambda: fit(prior_sd=0.0), lambda: fit(betas=(1.0, 0.999)),
           lambda: fit(w=torch.tensor([1.0, -1e-3, 1.0])),
           lambda: fit(w=torch.tensor([1.0, float("nan"), 1.0])),
           lambda: scores(S=1), lambda: scores(S=2049), lambda: scores(d=1), lambda: scores(d=257),
           lambda: scores(B=0), lambda: scores(Nu=2040, B=9)]
    for i, call in enumerate(bad):
        with pytest.raises(PsviError, match="PSVI_EINVAL"):
            call()
            pytest.fail(f"case {i} was accepted")


# ---- whole runs of the reference, replayed through the hooks
class _Stream:
    def __init__(self, flat):
        self.flat, self.o = torch.tensor(flat), 0

    def take(self, n):
        out = self.flat[self.o:self.o + n]
        assert out.numel() == n, "draw stream exhausted"
        self.o += n
        return out


@pytest.mark.parametrize("method", ["random", "sparsevi", "opsvi"])
def test_whole_run_replays_reference(method):
    import psvi.inference as I

    f = load_fixture("q4_run_" + method)
    c = f["cfg"]
    assert c["gap"] > 100 * 4 * c["tol_corr"] and c["top2"] > 100 * 4 * c["tol_corr"]
    st, batches, choices, state = _Stream(f["draws"]), iter(f["batches"]), iter(f["choices"]), {}
    kw = dict(x=torch.tensor(f["x"]), y=torch.tensor(f["y"]), xt=torch.tensor(f["xt"]),
              yt=torch.tensor(f["yt"]), mc_samples=c["S"], data_minibatch=c["B"],
              num_epochs=c["epochs"], log_every=c["log_every"], N=c["N"], D=2, seed=c["seed"],
              lr0net=c["lr0net"], noise_source=st.take, state_out=state)
    if method == "random":
        def choose(candidates):
            pt = int(next(choices))
            assert pt in candidates
            return pt

        res = I.run_random(choice_source=choose, **kw)
    elif method == "sparsevi":
        res = I.run_sparsevi(inner_it=c["inner_it"], outer_it=c["outer_it"], lr0v=c["lr0v"],
                             batch_source=lambda: next(batches), **kw)
    else:
        res = I.run_opsvi(inner_it=c["inner_it"], num_pseudo=c["num_pseudo"], lr0u=c["lr0u"],
                          lr0v=c["lr0v"], register_elbos=True, log_pseudodata=True,
                          batch_source=lambda: next(batches), **kw)
    # every stream consumed to its end
    assert st.o == st.flat.numel()
    assert next(batches, None) is None and next(choices, None) is None
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
    assert len(res["times"]) == len(res["accs"])
    if method == "opsvi":
        assert set(res) == {"accs", "nlls", "csizes", "times", "elbos", "us", "zs", "vs"}
        assert np.abs(state["u"] - f["u"]).max() < 0.5 * c["lr0u"]
        assert np.array_equal(np.array(res["elbos"])[:, 0], f["elbos"][:, 0])
        assert rel(np.array(res["elbos"])[:, 1], f["elbos"][:, 1]) < 1e-4
        assert np.abs(np.stack(res["us"]) - f["us"]).max() < 0.5 * c["lr0u"]
        assert np.abs(np.stack(res["vs"]) - f["vs"]).max() < 0.5 * lr_w
    else:
        assert set(res) == {"accs", "nlls", "csizes", "times", "wt_index"}
        ref = [{int(k): v for k, v in d.items()} for d in json.loads(str(f["wt_index"]))]
        assert [list(d) for d in res["wt_index"]] == [list(d) for d in ref]
        for got, exp in zip(res["wt_index"], ref):
            assert all(abs(got[k] - exp[k]) < 0.5 * lr_w for k in exp)


@pytest.mark.parametrize("method", ["random", "sparsevi", "opsvi"])
def test_experiment_driver_runs_the_laplace_baselines(method, tmp_path):
    from psvi.experiments import experiment_driver

    args = dict(mc_samples=4, num_epochs=3, data_minibatch=20, inner_it=5, outer_it=2,
                trainer="nested", log_every=1, lr0u=1e-3, lr0net=1e-2, lr0v=1e-2, init_sd=1e-3,
                coreset_sizes=[10], num_trials=1, test_ratio=0.2, architecture="logistic_regression",
                logistic_regression=True, n_hidden=10, fnm="lap", results_folder=str(tmp_path),
                register_elbos=True)
    res = experiment_driver(["halfmoon"], [method], args)
    r = res["halfmoon"][method]["10" if method == "opsvi" else "-1"]["0"]
    keys = {"accs", "nlls", "csizes", "times"} | ({"elbos"} if method == "opsvi" else {"wt_index"})
    assert set(r) == keys
    assert len(r["accs"]) == 3 and np.isfinite(r["accs"]).all() and np.isfinite(r["nlls"]).all()
    assert r["csizes"] == ([10, 10, 10] if method == "opsvi" else
                           [0, 1, 2] if method == "random" else r["csizes"])
    assert r["csizes"][-1] >= 1
    assert (tmp_path / "lap.json").exists() and (tmp_path / "lap.pk").exists()
