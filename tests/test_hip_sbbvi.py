"""Sparse black-box VI on the GPU: the Bernoulli plan, the sampled KL term, the
row log-likelihoods, the selection scores and the weight objective against
the reference-generated fixtures s1-s4 and, at the shape edges, against the
fp64 restatement (sbbvi_util, itself pinned to the fixtures on the CPU).

Tolerances: 1e-4 relative (the project's parity bound) for objectives and
gradients; ll within 1e-4 relative + 1e-6 absolute; corr / corecorr within 4x
the reference's own fp32-against-fp64 gap recorded in the fixture.  The
kernels' own arithmetic is fp64 with float outputs, so against the restatement
applied to the GPU's own ll they agree to float rounding (1e-6 relative)."""
import numpy as np
import pytest
import torch

from golden_util import l2rel, load_fixture, rel
import sbbvi_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _plan(layers, S, M):
    from psvi.runtime import InnerLoopPlan

    return InnerLoopPlan("meanfield", [tuple(l) for l in layers], S, M, likelihood="bernoulli")


@pytest.mark.parametrize("name", ["s1_elbo_nu0", "s1_elbo_nu5"])
def test_elbo_and_gradient_match_reference(name):
    f = load_fixture(name)
    c = f["cfg"]
    S, Nu = c["S"], c["Nu"]
    plan = _plan(c["layers"], S, max(Nu, 1))
    params, eps = dev(f["params"]), dev(f["eps"])
    if Nu:
        loss, grad = plan.elbo_grad(dev(f["u"]), dev(f["z"], torch.int32), dev(S * f["w"]), eps,
                                    params, include_kl=False)
    else:
        loss = torch.zeros(1, dtype=torch.float64, device=DEV)
        grad = torch.zeros_like(params)
    nkl = plan.sampled_kl_grad(eps, params, grad=grad)
    loss = (loss - nkl.sum()).item()
    print(name, "loss rel", rel(loss, f["loss64"]), "grad l2rel", l2rel(grad.cpu(), f["grad64"]),
          "nkl rel", rel(nkl.cpu(), f["nkl64"]))
    assert rel(nkl.cpu(), f["nkl64"]) < 1e-4
    assert rel(loss, f["loss64"]) < 1e-4
    assert l2rel(grad.cpu().numpy(), f["grad64"]) < 1e-4
    assert rel(grad.cpu().numpy(), f["grad64"]) < 1e-4


def _fixture_ll(f):
    c = f["cfg"]
    rows = np.concatenate((f["u"], f["xb"]))
    lab = np.concatenate((f["z"], f["yb"]))
    plan = _plan(c["layers"], c["S"], rows.shape[0])
    return plan.row_loglik(dev(rows), dev(lab, torch.int32), dev(f["eps"]), dev(f["params"]))


@pytest.mark.parametrize("name", ["s2_scores_nu0", "s2_scores_nu7"])
def test_selection_scores_match_reference(name):
    from psvi.runtime import select_scores

    f = load_fixture(name)
    c = f["cfg"]
    ll, _, nkl = _fixture_ll(f)
    err = np.abs(ll.cpu().numpy() - f["ll64"])
    print(name, "ll max err", err.max(), "nkl rel", rel(nkl.cpu(), f["nkl64"]))
    assert (err <= 1e-4 * np.abs(f["ll64"]) + 1e-6).all()
    sc = select_scores(ll, nkl, dev(f["w"]), c["Nu"], c["N"] / c["B"])
    tol = 4 * c["tol_corr"]
    assert c["gap"] > 100 * tol
    res = sc["result"].tolist()
    ec = np.abs(sc["corr"].cpu().numpy() - f["corr64"]).max()
    print(name, "corr err", ec, "tol", tol, "W err", np.abs(sc["W"].cpu().numpy() - f["W64"]).max())
    assert ec <= tol
    assert np.abs(sc["W"].cpu().numpy() - f["W64"]).max() <= 1e-4
    if c["Nu"]:
        ecc = np.abs(sc["corecorr"].cpu().numpy() - f["corecorr64"]).max()
        print(name, "corecorr err", ecc)
        assert ecc <= tol
        assert abs(res[2] - f["corecorr64"].max()) <= tol
    assert abs(res[0] - f["corr64"].max()) <= tol
    assert int(res[1]) == c["argmax"] and bool(res[3]) == c["attach"]


@pytest.mark.parametrize("name", ["s3_weights_nu7", "s3_weights_logreg"])
def test_weight_objective_matches_reference(name):
    from psvi.runtime import select_weight_grad

    f = load_fixture(name)
    ll, _, nkl = _fixture_ll(f)
    loss, gw = select_weight_grad(ll, nkl, dev(f["w"]), f["cfg"]["N"])
    print(name, "loss rel", rel(loss.item(), f["loss64"]), "grad rel", rel(gw.cpu(), f["gradw64"]))
    assert rel(loss.item(), f["loss64"]) < 1e-4
    assert rel(gw.cpu().numpy(), f["gradw64"]) < 1e-4


class _Stream:
    def __init__(self, flat):
        self.flat, self.o = torch.tensor(flat), 0

    def take(self, n):
        out = self.flat[self.o:self.o + n]
        assert out.numel() == n, "draw stream exhausted"
        self.o += n
        return out


@pytest.mark.parametrize("name", ["s4_run_logreg", "s4_run_fn"])
def test_whole_run_replays_reference(name):
    from psvi.inference import run_sparsevi_with_bb_elbo

    f = load_fixture(name)
    c = f["cfg"]
    assert c["gap"] > 100 * 4 * c["tol_corr"]
    st, batches, state = _Stream(f["draws"]), iter(f["batches"]), {}
    res = run_sparsevi_with_bb_elbo(
        n_layers=1, logistic_regression=c["arch"] == "logreg", n_hidden=c["H"], log_every=1,
        lr0=c["lr0"], register_elbos=True, seed=c["seed"], num_epochs=c["epochs"],
        inner_it=c["inner_it"], outer_it=c["outer_it"], x=torch.tensor(f["x"]),
        y=torch.tensor(f["y"]), xt=torch.tensor(f["xt"]), yt=torch.tensor(f["yt"]),
        mc_samples=c["S"], data_minibatch=c["B"], scatterplot_coreset=False,
        eps_source=st.take, batch_source=lambda: next(batches), params0=f["params0"],
        state_out=state)
    assert st.o == st.flat.numel() and next(batches, None) is None
    print(name, "core", state["core_idcs"], "max|dw|", np.abs(state["w"] - f["w"]).max(),
          "max|dp|", np.abs(state["params"] - f["params"]).max(), "nlls", res["nlls"], f["nlls"])
    assert state["core_idcs"] == f["core_idcs"].tolist()
    assert res["csizes"] == f["csizes"].tolist()
    assert np.abs(state["w"] - f["w"]).max() < 0.5 * c["lr0"]
    assert np.abs(state["params"] - f["params"]).max() < 0.5 * c["lr0"]
    nt = len(f["yt"])
    assert np.array_equal(np.round(np.array(res["accs"]) * nt), np.round(f["accs"] * nt))
    assert np.allclose(res["nlls"], f["nlls"], rtol=1e-4)
    assert np.array_equal(np.array(res["elbos"])[:, 0], f["elbos"][:, 0])
    assert rel(np.array(res["elbos"])[:, 1], f["elbos"][:, 1]) < 1e-4


def _problem(S, Nu, B, layers, seed, labels=None):
    g = torch.Generator().manual_seed(seed)
    D = layers[0][0]
    n_tot = sum(i * o + o for i, o in layers)
    params = torch.cat([torch.cat((0.7 * torch.randn(i * o + o, generator=g),
                                   -3 + 2 * torch.rand(i * o + o, generator=g)))
                        for i, o in layers])
    eps = torch.randn(S * n_tot, generator=g)
    x = torch.randn(Nu + B, D, generator=g)
    z = (torch.rand(Nu + B, generator=g) > 0.5).float() if labels is None \
        else torch.full((Nu + B,), float(labels))
    w = 0.5 + 2 * torch.rand(Nu, generator=g)
    return params, eps, x, z, w


def _run_all(plan, params, eps, x, z, w, Nu, N):
    """Every new entry point once; the outputs as CPU tensors."""
    from psvi.runtime import select_scores, select_weight_grad

    P, E = dev(params), dev(eps)
    ll, f, nkl = plan.row_loglik(dev(x), dev(z, torch.int32), E, P, logits=True)
    grad = torch.zeros_like(P)
    plan.sampled_kl_grad(E, P, grad=grad)
    B = x.shape[0] - Nu
    sc = select_scores(ll, nkl, dev(w) if Nu else None, Nu, N / B)
    out = dict(ll=ll, f=f, nkl=nkl, klgrad=grad, W=sc["W"], corr=sc["corr"], result=sc["result"])
    if Nu:
        out["corecorr"] = sc["corecorr"]
        out["loss"], out["gw"] = select_weight_grad(ll, nkl, dev(w), N)
    return {k: v.cpu() for k, v in out.items()}


def _check_against_restatement(out, params, eps, x, z, w, S, Nu, N, layers):
    P, E = U.t64(params), U.t64(eps)
    f64 = U.logits(P, layers, E, S, U.t64(x))
    ll64 = U.loglik(f64, U.t64(z))
    nkl64, gk64 = U.sampled_kl(P, layers, E, S)
    assert ((out["ll"].double() - ll64).abs() <= 1e-4 * ll64.abs() + 1e-6).all()
    assert ((out["f"].double() - f64).abs() <= 1e-4 * f64.abs() + 1e-6).all()
    assert rel(out["nkl"], nkl64) < 1e-6
    assert rel(out["klgrad"], gk64) < 1e-5
    # the selection kernels' own arithmetic: the restatement on the GPU's ll
    B = x.shape[0] - Nu
    W, corr, corecorr = U.scores(out["ll"].double(), out["nkl"], U.t64(w), Nu, N / B)
    assert rel(out["W"], W) < 1e-6 and rel(out["corr"], corr) < 1e-6
    res = out["result"].tolist()
    assert corr[int(res[1])] >= corr.max() - 1e-6 * corr.max().abs()
    assert res[0] == pytest.approx(float(corr.max()), rel=1e-6)
    if Nu:
        assert rel(out["corecorr"], corecorr) < 1e-6
        assert res[2] == pytest.approx(float(corecorr.max()), rel=1e-6)
        loss, gw = U.weight_objective(out["ll"].double(), out["nkl"], U.t64(w), N)
        assert rel(out["loss"], loss) < 1e-9 and rel(out["gw"], gw) < 1e-6
    else:
        assert res[3] == 1.0


@pytest.mark.parametrize("S", [2, 3, 65])
@pytest.mark.parametrize("Nu", [0, 1, 7])
@pytest.mark.parametrize("B", [1, 13])
def test_edge_shapes_and_bitwise_repeat(S, Nu, B):
    layers = [(3, 10), (10, 1)]
    prob = _problem(S, Nu, B, layers, 100 * S + 10 * Nu + B)
    plan = _plan(layers, S, Nu + B)
    a = _run_all(plan, *prob, Nu, 40.0)
    b = _run_all(plan, *prob, Nu, 40.0)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    _check_against_restatement(a, *prob, S, Nu, 40.0, layers)


@pytest.mark.parametrize("label", [0, 1])
def test_constant_labels(label):
    layers, S, Nu, B = [(3, 10), (10, 1)], 3, 2, 5
    prob = _problem(S, Nu, B, layers, 7 + label, labels=label)
    plan = _plan(layers, S, Nu + B)
    a = _run_all(plan, *prob, Nu, 40.0)
    b = _run_all(plan, *prob, Nu, 40.0)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    _check_against_restatement(a, *prob, S, Nu, 40.0, layers)


def test_rows_split_across_chunks():
    """A row count the network kernels split over several workgroups
    (PSVI_Q_NET_MCHUNKS > 1): every chunk writes its own rows."""
    layers, S = [(3, 10), (10, 1)], 2
    M = next((m for m in (256, 512, 1024, 2048, 4096, 8192, 16384)
              if _plan(layers, S, m).net_mchunks > 1), None)
    assert M is not None, "no row count splits into chunks"
    M += 3  # not a multiple of the tile
    plan = _plan(layers, S, M)
    assert plan.net_mchunks > 1
    Nu = 7
    prob = _problem(S, Nu, M - Nu, layers, 5)
    a = _run_all(plan, *prob, Nu, float(M))
    b = _run_all(plan, *prob, Nu, float(M))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    _check_against_restatement(a, *prob, S, Nu, float(M), layers)


def test_large_logits_are_overflow_safe():
    """Logits of +-40: softplus in its overflow-safe form, for the row
    log-likelihoods and for the inner objective's fused head.  The new entry
    points run twice, bit for bit; psvi_elbo_grad's objective is summed with
    double atomics over workgroups (as on every plan) and is not in that
    comparison."""
    layers, S = [(1, 1)], 2
    params = torch.tensor([40.0, 0.0, -20.0, -20.0])   # mu_W, mu_b, rho_W, rho_b
    eps = torch.zeros(S * 2)
    x = torch.tensor([[1.0], [-1.0], [1.0], [-1.0]])
    z = torch.tensor([1.0, 1.0, 0.0, 0.0])
    plan = _plan(layers, S, 4)
    ll, f, _ = plan.row_loglik(dev(x), dev(z, torch.int32), dev(eps), dev(params), logits=True)
    f64 = U.logits(U.t64(params), layers, U.t64(eps), S, U.t64(x))
    ll64 = U.loglik(f64, U.t64(z))
    assert torch.isfinite(ll).all() and f.abs().max().item() == pytest.approx(40.0, rel=1e-5)
    assert ((ll.cpu().double() - ll64).abs() <= 1e-4 * ll64.abs() + 1e-6).all()
    a = _run_all(plan, params, eps, x, z, torch.ones(2), 2, 40.0)
    b = _run_all(plan, params, eps, x, z, torch.ones(2), 2, 40.0)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["ll"], ll.cpu()) and torch.equal(a["f"], f.cpu())
    assert all(torch.isfinite(v).all() for k, v in a.items() if k != "result")
    w = torch.ones(4)
    loss, grad = plan.elbo_grad(dev(x), dev(z, torch.int32), dev(w), dev(eps), dev(params),
                                include_kl=False)
    p = U.t64(params).requires_grad_(True)
    nll = -(U.loglik(U.logits(p, layers, U.t64(eps), S, U.t64(x)), U.t64(z)) @ U.t64(w)).sum()
    (g64,) = torch.autograd.grad(nll, p)
    assert torch.isfinite(grad).all()
    assert rel(loss.item(), nll.item()) < 1e-4 and rel(grad.cpu(), g64) < 1e-4


def test_step_loop_and_phases_agree_with_elbo_grad():
    """psvi_inner_step, psvi_inner_loop and the mean-field phases on a Bernoulli
    plan: the same network launch as psvi_elbo_grad, so the objective, the
    gradient and the Adam steps agree with it to fp32 rounding (1e-6)."""
    from psvi.runtime import adam_update_

    layers, S, M, lr = [(3, 10), (10, 1)], 3, 9, 1e-2
    params, eps, x, z, _ = _problem(S, 0, M, layers, 11)
    g = torch.Generator().manual_seed(12)
    eps2 = torch.randn(eps.numel(), generator=g)
    w = 0.5 + torch.rand(M, generator=g)
    plan = _plan(layers, S, M)
    X, Z, Wt, E, E2 = dev(x), dev(z, torch.int32), dev(w), dev(eps), dev(eps2)
    P0 = dev(params)
    loss, grad = plan.elbo_grad(X, Z, Wt, E, P0)
    # the phases: accumulate + update in gradient mode
    acc = torch.empty(plan.acc_count, device=DEV)
    nll = torch.zeros(1, dtype=torch.float64, device=DEV)
    kl = torch.zeros(1, dtype=torch.float64, device=DEV)
    g2 = torch.empty_like(P0)
    plan.mf_accumulate(X, Z, Wt, E, P0, acc, nll)
    plan.mf_update(acc, P0, kl_out=kl, grad_out=g2)
    assert rel(g2.cpu(), grad.cpu()) < 1e-6
    # the phase update sums its KL in fp32 over 256-parameter blocks, the fused
    # path over 16-parameter blocks: the same terms grouped differently, so the
    # objectives agree to fp32 rounding, not to fp64
    assert rel((nll + kl).item(), loss.item()) < 1e-6
    # one fused step = the gradient + the generic Adam update
    P1, m1, v1 = P0.clone(), torch.zeros_like(P0), torch.zeros_like(P0)
    e1 = plan.inner_step(X, Z, Wt, E, P1, m1, v1, step=1, lr=lr)
    Pr, mr, vr = P0.clone(), torch.zeros_like(P0), torch.zeros_like(P0)
    adam_update_(Pr, grad, mr, vr, step=1, lr=lr)
    assert rel(e1.item(), loss.item()) < 1e-9
    assert (P1 - Pr).abs().max().item() < 1e-6 * lr + 1e-7
    # two chained steps = two fused steps
    P2, m2, v2 = P0.clone(), torch.zeros_like(P0), torch.zeros_like(P0)
    el = plan.inner_loop(X, Z, Wt, P2, m2, v2, 2, lr, eps=torch.cat((E, E2)))
    e2 = plan.inner_step(X, Z, Wt, E2, P1, m1, v1, step=2, lr=lr)
    assert rel(el.cpu(), torch.cat((e1, e2)).cpu()) < 1e-9
    assert (P2 - P1).abs().max().item() < 1e-6


def test_unsupported_entry_points_refuse():
    from psvi.runtime import PsviError

    layers, S, M = [(3, 10), (10, 1)], 3, 6
    params, eps, x, z, w = _problem(S, 0, M, layers, 3)
    plan = _plan(layers, S, M)
    args = (dev(x), dev(z, torch.int32), dev(torch.ones(M)), dev(eps), dev(params))
    with pytest.raises(PsviError, match="PSVI_EUNSUP"):
        plan.outer_elbo_grad(2, *args)
    with pytest.raises(PsviError, match="PSVI_EUNSUP"):
        plan.evaluate(2, *args)
    with pytest.raises(PsviError, match="PSVI_EUNSUP"):
        plan.hvp(*args, dev(params))


def test_experiment_driver_runs_sparsebbvi(tmp_path):
    from psvi.experiments import experiment_driver

    args = dict(mc_samples=4, num_epochs=3, data_minibatch=20, inner_it=2, outer_it=2,
                trainer="nested", log_every=1, lr0u=1e-3, lr0net=1e-3, lr0v=1e-2, init_sd=1e-3,
                coreset_sizes=[10], num_trials=1, test_ratio=0.2, architecture="fn",
                logistic_regression=False, n_hidden=10, fnm="sb", results_folder=str(tmp_path))
    res = experiment_driver(["halfmoon"], ["sparsebbvi"], args)
    r = res["halfmoon"]["sparsebbvi"]["-1"]["0"]
    assert set(r) == {"accs", "nlls", "csizes", "times", "elbos"}
    assert len(r["accs"]) == 3 and np.isfinite(r["accs"]).all() and np.isfinite(r["nlls"]).all()
    assert r["csizes"][0] == 0 and r["csizes"][-1] >= 1


# --------------------------------------------------------------------------
# The one-workgroup selection kernels past the first trip of their loops:
# kSelThreads = 512 threads stride over the samples (S > 512, up to kSelMaxS =
# 2048), over the columns (Nu + B > 512) and over grad_w (Nu > 512).
SEL_SHAPES = [(513, 0, 1), (1025, 513, 600), (2048, 3, 515)]


def _sel_inputs(S, Nu, B, seed):
    """ll at log-likelihood scale (negative, 0.5 to 10), nkl and core weights
    whose weighted sums spread the samples' softmax weights over a few units."""
    g = torch.Generator().manual_seed(seed)
    ll = -(0.5 + 9.5 * torch.rand(S, Nu + B, generator=g))
    nkl = 2.0 * torch.randn(S, generator=g, dtype=torch.float64)
    w = (0.5 + 2 * torch.rand(Nu, generator=g)) * (3.0 / max(Nu, 1))
    return ll, nkl, w


def _scores_dev(ll, nkl, w, Nu, scale):
    from psvi.runtime.engine import select_scores

    sc = select_scores(dev(ll), dev(nkl, torch.float64), dev(w) if Nu else None, Nu, scale)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in sc.items() if v is not None}


@pytest.mark.parametrize("S,Nu,B", SEL_SHAPES)
def test_scores_past_one_trip(S, Nu, B):
    ll, nkl, w = _sel_inputs(S, Nu, B, S + Nu + B)
    scale = 1000.0 / B
    a, b = _scores_dev(ll, nkl, w, Nu, scale), _scores_dev(ll, nkl, w, Nu, scale)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    W, corr, corecorr = U.scores(ll.double(), nkl, U.t64(w), Nu, scale)
    res = a["result"].tolist()
    print(f"scores S {S} Nu {Nu} B {B}: W rel {rel(a['W'], W):.2e} corr rel {rel(a['corr'], corr):.2e}")
    assert rel(a["W"], W) < 1e-6 and rel(a["corr"], corr) < 1e-6
    assert corr[int(res[1])] >= corr.max() - 1e-6 * corr.max().abs()
    assert res[0] == pytest.approx(float(corr.max()), rel=1e-6)
    if Nu:
        assert rel(a["corecorr"], corecorr) < 1e-6
        assert res[2] == pytest.approx(float(corecorr.max()), rel=1e-6)
        assert res[3] == (1.0 if res[0] > res[2] else 0.0)
    else:
        assert res[3] == 1.0


@pytest.mark.parametrize("other", [300, 3])
def test_argmax_takes_the_first_of_equal_maxima_across_trips(other):
    """The winning data column, as bits, in columns 4 and 4 + 512 (one thread's
    first and second trip) and in a column of another thread, above (300) or
    below (3) them.  A column's sums run in sample order whichever thread owns
    it, so equal columns score equal bits; the lowest index must win."""
    S, Nu, B = SEL_SHAPES[2]
    ll, nkl, w = _sel_inputs(S, Nu, B, 77)
    scale = 1000.0 / B
    win = int(_scores_dev(ll, nkl, w, Nu, scale)["result"][1])
    col = ll[:, Nu + win].clone()
    for j in (4, 4 + 512, other):           # global columns; data index j - Nu
        ll[:, j] = col
    tied = [c for c in range(B) if torch.equal(ll[:, Nu + c], col)]
    assert {4 - Nu, 4 + 512 - Nu, other - Nu} <= set(tied) and len(tied) <= 4
    _, corr, _ = U.scores(ll.double(), nkl, U.t64(w), Nu, scale)
    rest = torch.ones(B, dtype=torch.bool)
    rest[tied] = False
    assert corr[tied].min() > corr[rest].max() + 1e-4 * corr.abs().max()   # the tied columns lead
    a = _scores_dev(ll, nkl, w, Nu, scale)
    res = a["result"].tolist()
    cb = a["corr"].view(torch.int32)
    assert len({int(cb[c]) for c in tied}) == 1
    assert int(res[1]) == min(tied), (res, tied)
    assert res[0] == pytest.approx(float(corr.max()), rel=1e-6)
    assert res[3] == (1.0 if res[0] > res[2] else 0.0)


def _weight_dev(ll, nkl, w, N):
    from psvi.runtime.engine import select_weight_grad

    loss, gw = select_weight_grad(dev(ll), dev(nkl, torch.float64), dev(w), N)
    torch.cuda.synchronize()
    return loss.cpu(), gw.cpu()


@pytest.mark.parametrize("S,Nu,B,late_max", [(1025, 513, 600, False), (2048, 3, 515, False),
                                             (1025, 513, 600, True)])
def test_weight_objective_past_one_trip(S, Nu, B, late_max):
    """late_max: the samples of the first trip lie 800 below those from s = 512
    on, so lw spans more than 700 and sel_softmax's maximum is one the second
    trip finds (exp of a difference to the first trip's maximum overflows)."""
    ll, nkl, w = _sel_inputs(S, Nu, B, 3 * S + Nu + B)
    if late_max:
        nkl[:512] -= 800.0
    N = 1000.0
    a, b = _weight_dev(ll, nkl, w, N), _weight_dev(ll, nkl, w, N)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    loss, gw = U.weight_objective(ll.double(), nkl, U.t64(w), N)
    if late_max:
        lw = -N / Nu * (-ll[:, :Nu].double() @ U.t64(w)) + nkl
        assert lw.max() - lw[:512].max() > 700 and int(lw.argmax()) >= 512
    print(f"weights S {S} Nu {Nu} B {B} late {late_max}: loss rel {rel(a[0], loss):.2e} "
          f"grad rel {rel(a[1], gw):.2e}")
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
    assert rel(a[0], loss) < 1e-9 and rel(a[1], gw) < 1e-6


def test_more_samples_than_the_lds_holds_are_refused():
    from psvi.runtime import PsviError
    from psvi.runtime.engine import select_scores, select_weight_grad

    S = 2049                                  # kSelMaxS + 1
    ll, nkl, w = _sel_inputs(S, 3, 5, 1)
    with pytest.raises(PsviError):
        select_scores(dev(ll), dev(nkl, torch.float64), dev(w), 3, 2.0)
    with pytest.raises(PsviError):
        select_weight_grad(dev(ll), dev(nkl, torch.float64), dev(w), 10.0)
    torch.cuda.synchronize()
