"""Gaussian-likelihood (regressor) plans of libpsvi_hip against the reference's
own numbers (fixtures tests/golden/r*.npz, tools/gen_golden_regressor.py: the
reference's PSVI_regressor family in float64 on fp32-rounded draws) and
against themselves.

Bars (the project's own, tests/test_hip_variants.py / README "Parity"):
objective values rel < 1e-5, gradients l2rel < 1e-4, evaluate rel < 1e-5; a
whole nested_step: final parameters l2rel < 1e-5, hypergradients
< max(1e-4, 4 x the reference's own fp32-replay error), the stepped
u / v / z / alpha within 1e-3 * lr on the entries above 1 % of the largest.

Shapes: "small" (D 3, hidden 10, one hidden layer, M 5, S 3) sits inside one
16-row tile and one pseudopoint chunk; "large" (D 6, hidden 24, two hidden
layers, M 37, S 8) spans three row tiles with a ragged last one and more than
one pseudopoint chunk: test_pseudopoint_chunks_covered reads the counts from
the plans (PSVI_Q_NET_MCHUNKS) -- the large inner plan (M = 37) runs two chunks,
the large outer plan (M = 37 + 11) three, every small plan one."""
import ctypes

import numpy as np
import pytest
import torch

from golden_util import fixture_names, l2rel, load_fixture, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(x, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def _plan(cfg, M, **kw):
    from psvi.runtime import InnerLoopPlan

    return InnerLoopPlan("meanfield", cfg["layers"], cfg["S"], M,
                         likelihood=("gaussian", cfg["tau"]), **kw)


def _weights(cfg, f, alpha=None):
    """N f(v) and its Jacobian-vector helper (float64 host): PSVI_regressor
    f = identity, the others softmax(v) (times exp(alpha))."""
    v = torch.tensor(f["v0"], dtype=torch.float64, requires_grad=True)
    a = None
    if cfg["cls"] == "PSVI_regressor":
        w = cfg["N"] * v
    elif cfg["cls"] == "PSVILearnV_regressor":
        w = cfg["N"] * torch.softmax(v, 0)
    else:
        a = torch.tensor([cfg["alpha0"]], dtype=torch.float64, requires_grad=True)
        w = cfg["N"] * torch.exp(a) * torch.softmax(v, 0)
    return v, a, w


def _chain(w, grad_w, *leaves):
    gs = torch.autograd.grad(w, [l for l in leaves if l is not None],
                             torch.tensor(grad_w, dtype=torch.float64), retain_graph=True)
    return [g.numpy() for g in gs]


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", fixture_names("r1"))
def test_inner_elbo_and_gradients(name):
    """psvi_elbo_grad (value, parameter gradient) and the row pass
    psvi_outer_elbo_grad_coef_ex with coefficient 1 on every sample's pseudo
    term (u, w -> v, z gradients) against the reference's inner_elbo."""
    from psvi.runtime.sharded import pack_coef

    f = load_fixture(name)
    cfg = f["cfg"]
    S, M = cfg["S"], cfg["M"]
    plan = _plan(cfg, M)
    v, _, w = _weights(cfg, f)
    u, z, wd = _t(f["u0"]), _t(f["z0"]), _t(w.detach().numpy())
    eps, p = _t(f["eps"]), _t(f["params0"])
    elbo, grad = plan.elbo_grad(u, z, wd, eps, p)
    one, zero = torch.ones(S, dtype=torch.float64), torch.zeros(S, dtype=torch.float64)
    g = plan.outer_grad_coef(M, u, z, wd, eps, p, pack_coef(one, zero, zero, 0, S).to(DEV),
                             grad_z=True)
    (gv,) = _chain(w, g["grad_w"].cpu().numpy(), v)
    e = dict(elbo=rel(elbo.item(), f["out"]), params=l2rel(grad.cpu().numpy(), f["grad_params"]),
             u=l2rel(g["grad_u"].cpu().numpy(), f["u_grad"]), v=l2rel(gv, f["v_grad"]),
             z=l2rel(g["grad_z"].cpu().numpy(), f["z_grad"]))
    print(name, {k: f"{x:.2e}" for k, x in e.items()})
    assert e["elbo"] < 1e-5
    for k in ("params", "u", "v", "z"):
        assert e[k] < 1e-4, (k, e[k])


@pytest.mark.parametrize("name", fixture_names("r2"))
def test_psvi_elbo_and_gradients(name):
    """psvi_outer_elbo_grad_ex against the reference's psvi_elbo: value and
    the gradients w.r.t. the parameters, u, v / alpha (through N f(v)) and z."""
    f = load_fixture(name)
    cfg = f["cfg"]
    Mu, Nx = cfg["M"], cfg["Nx"]
    plan = _plan(cfg, Mu + Nx)
    v, a, w = _weights(cfg, f)
    x_all = _t(np.concatenate([f["u0"], f["xb"]]))
    z_all = _t(np.concatenate([f["z0"], f["yb"]]))
    w_all = _t(np.concatenate([w.detach().numpy(), np.full(Nx, cfg["N"] / Nx)]))
    out = plan.outer_elbo_grad(Mu, x_all, z_all, w_all, _t(f["eps"]), _t(f["params0"]),
                               grad_z=True)
    gs = _chain(w, out["grad_w"].cpu().numpy(), v, a)
    e = dict(loss=rel(out["loss"].item(), f["out"]),
             params=l2rel(out["grad"].cpu().numpy(), f["grad_params"]),
             u=l2rel(out["grad_u"].cpu().numpy(), f["u_grad"]), v=l2rel(gs[0], f["v_grad"]),
             z=l2rel(out["grad_z"].cpu().numpy(), f["z_grad"]))
    if a is not None:
        e["alpha"] = l2rel(gs[1], f["alpha_grad"])
    print(name, {k: f"{x:.2e}" for k, x in e.items()})
    assert e.pop("loss") < 1e-5
    for k, x in e.items():
        assert x < 1e-4, (k, x)


@pytest.mark.parametrize("name", fixture_names("r4"))
def test_evaluate_regression(name):
    """psvi_evaluate_regression over the fixture's two test batches: (rmse,
    test_ll) as PSVI_regressor.evaluate accumulates them."""
    f = load_fixture(name)
    cfg = f["cfg"]
    Mu = cfg["M"]
    v, _, w = _weights(cfg, f)
    se = ll = 0.0
    total = 0
    for i, nt in enumerate(cfg["nts"]):
        plan = _plan(cfg, Mu + nt)
        x_all = _t(np.concatenate([f["u0"], f[f"xt{i}"]]))
        y_all = _t(np.concatenate([f["z0"], f[f"yt{i}"]]))
        w_all = _t(np.concatenate([w.detach().numpy(), np.zeros(nt)]))
        st, pred = plan.evaluate_regression(Mu, x_all, y_all, w_all, _t(f[f"eps{i}"]),
                                            _t(f["params0"]), cfg["y_mean"], cfg["y_std"],
                                            pred=True)
        st = st.cpu().numpy()
        # the statistics are the sums over the returned predictions
        d = pred.cpu().numpy().astype(np.float64) - f[f"yt{i}"]
        assert rel(st[2], (d * d).sum()) < 1e-6
        assert 0.0 < st[1] <= 1.0 + 1e-12
        se, ll, total = se + st[2], ll + st[3], total + nt
    rmse, tll = np.sqrt(se / total), ll / total
    print(name, f"rmse {rmse:.6f} (ref {float(f['rmse']):.6f}) ll {tll:.6f} (ref {float(f['test_ll']):.6f})")
    assert rel(rmse, f["rmse"]) < 1e-5
    assert rel(tll, f["test_ll"]) < 1e-5


def test_evaluate_uniform_weights():
    """correction = 0: W = 1 / S -- the prediction is the plain mean over the
    samples of the network output (float64 host forward)."""
    f = load_fixture("r4_eval_small_t01")
    cfg = f["cfg"]
    Mu, nt = cfg["M"], cfg["nts"][0]
    plan = _plan(cfg, Mu + nt)
    args = (Mu, _t(np.concatenate([f["u0"], f["xt0"]])), _t(np.concatenate([f["z0"], f["yt0"]])),
            torch.zeros(Mu + nt, device=DEV), _t(f["eps0"]), _t(f["params0"]), 0.0, 1.0)
    _, p0 = plan.evaluate_regression(*args, correction=False, pred=True)
    _, p1 = plan.evaluate_regression(*args, correction=True, pred=True)
    assert not torch.equal(p0, p1)
    fs = _forward64(cfg, f["params0"], f["eps0"], np.concatenate([f["u0"], f["xt0"]]))[:, Mu:]
    assert l2rel(p0.cpu().numpy(), fs.mean(0)) < 1e-5


# ------------------------------------------------- fp64 host model (test-local)
def _sample64(cfg, params, eps):
    """Per-sample weights of the mean-field stack from the flat parameter and
    eps vectors (the library's layouts), float64 torch tensors."""
    S = cfg["S"]
    po = eo = 0
    out = []
    for din, dout in cfg["layers"]:
        nw, n = din * dout, din * dout + dout
        mu, rho = params[po:po + n], params[po + n:po + 2 * n]
        sd = torch.nn.functional.softplus(rho)
        eW = eps[eo:eo + S * nw].reshape(S, dout, din)
        eB = eps[eo + S * nw:eo + S * n].reshape(S, dout)
        W = mu[:nw].reshape(dout, din) + eW * sd[:nw].reshape(dout, din)
        b = mu[nw:] + eB * sd[nw:]
        out.append((W, b))
        po += 2 * n
        eo += S * n
    return out


def _net64(cfg, params, eps, x):
    h = x.unsqueeze(0).expand(cfg["S"], -1, -1)
    Ws = _sample64(cfg, params, eps)
    for i, (W, b) in enumerate(Ws):
        h = torch.einsum("smi,soi->smo", h, W) + b[:, None, :]
        if i + 1 < len(Ws):
            h = torch.relu(h)
    return h.squeeze(-1)


def _forward64(cfg, params, eps, x):
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    return _net64(cfg, t(params), t(eps), t(x)).numpy()


def _inner64(cfg, params, eps, u, z, w):
    """The negative inner ELBO of the Gaussian head in float64 (closed-form KL)."""
    tau = cfg["tau"]
    f = _net64(cfg, params, eps, u)
    nll = 0.5 * tau * (f - z) ** 2 + 0.5 * np.log(2 * np.pi / tau)
    kl, po = 0.0, 0
    for din, dout in cfg["layers"]:
        n = din * dout + dout
        mu, sd = params[po:po + n], torch.nn.functional.softplus(params[po + n:po + 2 * n])
        kl = kl + (-torch.log(sd) + 0.5 * (sd ** 2 + mu ** 2) - 0.5).sum()   # prior_sd = 1
        po += 2 * n
    return (nll * w).sum() + kl


def _hvp_case():
    f = load_fixture("r1_inner_small_t4")
    cfg = f["cfg"]
    _, _, w = _weights(cfg, f)
    rng = np.random.default_rng(11)
    vec = (rng.normal(size=f["params0"].size) * 0.1).astype(np.float32)
    return f, cfg, w.detach().numpy().astype(np.float32), vec


def test_hvp_matches_float64_autograd():
    """psvi_hvp_ex (hv, du, dw, dz) against double backward of the same
    objective in float64 on the host; the bar of tests/test_hip_hvp.py."""
    f, cfg, w, vec = _hvp_case()
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=True)
    p, u, z, wt = t(f["params0"]), t(f["u0"]), t(f["z0"]), t(w)
    loss = _inner64(cfg, p, torch.tensor(f["eps"], dtype=torch.float64), u, z, wt)
    (g,) = torch.autograd.grad(loss, p, create_graph=True)
    ref = torch.autograd.grad((g * torch.tensor(vec, dtype=torch.float64)).sum(), [p, u, wt, z])
    plan = _plan(cfg, cfg["M"])
    got = plan.hvp(_t(f["u0"]), _t(f["z0"]), _t(w), _t(f["eps"]), _t(f["params0"]), _t(vec))
    for name, a, b in zip(("hv", "du", "dw", "dz"), got, ref):
        e = l2rel(a.cpu().numpy(), b.numpy())
        print(f"hvp {name}: l2rel {e:.2e}")
        assert e < 1e-4, (name, e)


def test_hvp_matches_finite_differences():
    """hv, du, dw, dz against central finite differences of psvi_elbo_grad in
    the directions vec / u / w / z (fp32 kernels, differences formed in
    float64 on the host).  Bar: 1e-4 l2-relative, the bar tests/test_hip_hvp.py
    holds the categorical head's products to.  vec . grad is linear in w and
    in z, so those differences are exact up to rounding at any step; along vec
    and u the step is 2^-8 of the direction's scale (fp32 gradient noise ~1e-7
    over it, second-order truncation of the same size)."""
    f, cfg, w, vec = _hvp_case()
    plan = _plan(cfg, cfg["M"])
    eps, ws = _t(f["eps"]), plan.workspace()
    # the direction the two fp32 parameter points really differ by (exact in fp32)
    h = 2.0 ** -8
    php, plo = f["params0"] + np.float32(h) * vec, f["params0"] - np.float32(h) * vec
    v64 = (php.astype(np.float64) - plo) / (2 * h)
    vec = v64.astype(np.float32)
    assert np.array_equal(vec.astype(np.float64), v64)

    def grad(p=f["params0"], u=f["u0"], z=f["z0"], ww=w):
        return plan.elbo_grad(_t(u), _t(z), _t(ww), eps, _t(p), ws=ws)[1].cpu().numpy().astype(
            np.float64)

    def fd(base, h, key):
        out = np.zeros(base.size)
        for i in range(base.size):
            d = np.zeros(base.size, np.float32)
            d[i] = h
            hi, lo = (base.ravel() + d).reshape(base.shape), (base.ravel() - d).reshape(base.shape)
            step = float((hi.ravel()[i].astype(np.float64) - lo.ravel()[i]))
            out[i] = (grad(**{key: hi}) @ v64 - grad(**{key: lo}) @ v64) / step
        return out.reshape(base.shape)

    hv, du, dw, dz = (x.cpu().numpy() for x in plan.hvp(
        _t(f["u0"]), _t(f["z0"]), _t(w), eps, _t(f["params0"]), _t(vec)))
    hv_fd = (grad(p=php) - grad(p=plo)) / (2 * h)
    e = dict(hv=l2rel(hv, hv_fd), du=l2rel(du, fd(f["u0"], h, "u")),
             dw=l2rel(dw, fd(w, 0.25 * float(np.abs(w).mean()), "ww")),
             dz=l2rel(dz, fd(f["z0"], 0.5, "z")))
    print("hvp vs finite differences:", {k: f"{x:.2e}" for k, x in e.items()})
    for k, x in e.items():
        assert x < 1e-4, (k, x)


# ------------------------------------------------------------- consistency
@pytest.mark.parametrize("name", ["r1_inner_small_t01", "r1_inner_large_t4"])
def test_inner_loop_equals_steps_and_is_reproducible(name):
    """psvi_inner_loop of T = 4 == four psvi_inner_step calls on the same
    Philox draws -- the mean-field criterion of
    test_inner_loop_philox_equals_stepwise: parameters and Adam state bitwise,
    ELBOs to 1e-6 -- and a second run of the loop gives the same bits."""
    from psvi.runtime import randn_

    f = load_fixture(name)
    cfg = f["cfg"]
    plan = _plan(cfg, cfg["M"])
    _, _, w = _weights(cfg, f)
    u, z, wd, p0 = _t(f["u0"]), _t(f["z0"]), _t(w.detach().numpy()), _t(f["params0"])
    T, lr = 4, 1e-3
    runs = []
    for _ in range(2):
        pa, ma, va = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        ea = plan.inner_loop(u, z, wd, pa, ma, va, T, lr, seed=5, offset=0).clone()
        runs.append((pa, ma, va, ea))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    pa, ma, va, ea = runs[0]
    pb, mb, vb = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    eps, ws, eb = torch.empty(plan.eps_count, device=DEV), plan.workspace(), []
    for t in range(T):
        randn_(eps, 5, t * plan.eps_stride)
        eb.append(plan.inner_step(u, z, wd, eps, pb, mb, vb, step=t + 1, lr=lr, ws=ws).item())
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert np.allclose(ea.cpu().numpy(), eb, rtol=1e-6, atol=0)
    assert not torch.equal(pa, p0)


def test_gradient_calls_bitwise_reproducible():
    f = load_fixture("r2_outer_large_t4")
    cfg = f["cfg"]
    Mu, Nx = cfg["M"], cfg["Nx"]
    plan = _plan(cfg, Mu + Nx)
    _, _, w = _weights(cfg, f)
    args = (Mu, _t(np.concatenate([f["u0"], f["xb"]])), _t(np.concatenate([f["z0"], f["yb"]])),
            _t(np.concatenate([w.detach().numpy(), np.full(Nx, cfg["N"] / Nx)])), _t(f["eps"]),
            _t(f["params0"]))
    a, b = plan.outer_elbo_grad(*args, grad_z=True), plan.outer_elbo_grad(*args, grad_z=True)
    for k in ("loss", "grad", "grad_u", "grad_w", "grad_z"):
        assert torch.equal(a[k], b[k]), k
    g = load_fixture("r1_inner_large_t4")
    gc = g["cfg"]
    ip = _plan(gc, gc["M"])
    vec = _t(np.random.default_rng(3).normal(size=g["params0"].size))
    hargs = (_t(g["u0"]), _t(g["z0"]), torch.full((gc["M"],), 7.0, device=DEV), _t(g["eps"]),
             _t(g["params0"]), vec)
    for x, y in zip(ip.hvp(*hargs), ip.hvp(*hargs)):
        assert torch.equal(x, y)


def test_categorical_lik_plan_is_the_default_plan():
    """psvi_plan_create and psvi_plan_create_lik(categorical) give bitwise
    equal psvi_elbo_grad outputs on a mean-field g* fixture."""
    from psvi.runtime import InnerLoopPlan, _lib

    name = next(n for n in fixture_names() if load_fixture(n)["cfg"]["family"] == "mf")
    f = load_fixture(name)
    cfg = f["cfg"]
    a = InnerLoopPlan("meanfield", cfg["layers"], cfg["S"], cfg["M"])
    b = InnerLoopPlan("meanfield", cfg["layers"], cfg["S"], cfg["M"])
    lib = _lib.load()
    h = ctypes.c_void_p()
    lik = _lib.Likelihood(_lib.LIK_CATEGORICAL, 0.0)
    _lib.check(lib.psvi_plan_create_lik(_lib.FAMILY_MEANFIELD, ctypes.byref(b.desc), 1, 0,
                                        ctypes.byref(lik), ctypes.byref(h)), "psvi_plan_create_lik")
    lib.psvi_plan_destroy(b.handle)
    b.handle = h
    args = (_t(f["u"]), _t(f["z"].astype(np.int32), torch.int32), _t(f["w"]), _t(f["eps"][0]),
            _t(f["params0"]))
    (ea, ga), (eb, gb) = a.elbo_grad(*args), b.elbo_grad(*args)
    assert torch.equal(ea, eb) and torch.equal(ga, gb)
    assert float(ga.abs().max()) > 0


# ---------------------------------------------------------------- refusals
def test_refusals():
    from psvi.runtime import InnerLoopPlan
    from psvi.runtime._lib import PsviError

    f = load_fixture("r2_outer_small_t01")
    cfg = f["cfg"]
    Mu, Nx = cfg["M"], cfg["Nx"]
    M = Mu + Nx
    gp = _plan(cfg, M)
    x, w = torch.zeros(M, 3, device=DEV), torch.ones(M, device=DEV)
    zf = torch.zeros(M, device=DEV)
    eps, p = _t(f["eps"]), _t(f["params0"])
    with pytest.raises(PsviError, match="PSVI_ESTATE"):   # psvi_evaluate on a Gaussian plan
        gp.evaluate(Mu, x, zf, w, eps, p)
    with pytest.raises(PsviError, match="PSVI_EUNSUP"):   # the ablated objective
        gp.outer_ablated_elbo_grad(x, zf, w, eps, p)
    with pytest.raises(ValueError):                       # int labels on a Gaussian plan
        gp.elbo_grad(x, torch.zeros(M, dtype=torch.int32, device=DEV), w, eps, p)
    cp = InnerLoopPlan("meanfield", cfg["layers"], cfg["S"], M)
    zi = torch.zeros(M, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        cp.outer_elbo_grad(Mu, x, zi, w, eps, p, grad_z=True)
    # grad_z / dz_out on a categorical plan at the C ABI: PSVI_ESTATE
    buf = torch.zeros(M, device=DEV)
    ws = torch.empty(max(cp.outer_ws_bytes, cp.hvp_ws_bytes), dtype=torch.uint8, device=DEV)
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    grad = torch.zeros(cp.param_count, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = cp.lib.psvi_outer_elbo_grad_ex(cp.handle, Mu, P(x), P(zi), P(w), P(eps), P(p), P(loss),
                                        P(grad), None, None, P(buf), None, P(ws), ws.numel(), None)
    assert rc == -4 and b"Gaussian" in cp.lib.psvi_last_error()
    hv = torch.zeros_like(grad)
    rc = cp.lib.psvi_hvp_ex(cp.handle, P(x), P(zi), P(w), P(eps), P(p), P(grad), 1, P(hv),
                            None, None, P(buf), P(ws), ws.numel(), None)
    assert rc == -4 and b"Gaussian" in cp.lib.psvi_last_error()
    with pytest.raises(PsviError, match="PSVI_ESTATE"):   # evaluate_regression on a categorical plan
        _lib_check_eval_regression(cp, Mu, x, zf, w, eps, p)


def _lib_check_eval_regression(plan, Mu, x, y, w, eps, p):
    from psvi.runtime._lib import check

    st = torch.zeros(4, dtype=torch.float64, device=DEV)
    ws = torch.empty(plan.eval_ws_bytes, dtype=torch.uint8, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    check(plan.lib.psvi_evaluate_regression(plan.handle, Mu, P(x), P(y), P(w), P(eps), P(p), 1,
                                            0.0, 1.0, None, P(st), P(ws), ws.numel(), None),
          "psvi_evaluate_regression")


# ------------------------------------------------------------ chunk coverage
def test_pseudopoint_chunks_covered():
    """The plans' own chunk counts: the small shape stays in one pseudopoint
    chunk, the large one really splits its rows -- inner / HVP plans (M = 37)
    and outer / evaluate plans (M = 37 + 11, 37 + 7) -- so the fixed-order
    sums over chunks (dW slots, grad_z, dz) are exercised by the tests above."""
    small, large = load_fixture("r1_inner_small_t01")["cfg"], load_fixture("r1_inner_large_t4")["cfg"]
    got = {(tag, M): _plan(cfg, M).net_mchunks
           for tag, cfg, Ms in (("small", small, (5, 16, 12)), ("large", large, (37, 48, 44)))
           for M in Ms}
    print("pseudopoint chunks:", got)
    assert all(n == 1 for (tag, _), n in got.items() if tag == "small"), got
    assert all(n >= 2 for (tag, _), n in got.items() if tag == "large"), got


# --------------------------------------------------------- the psvi classes
def _obj(f):
    """The fixture's regressor object on the device: model, u, z, v (alpha)
    set explicitly, optimisers as the generator's."""
    import psvi.inference as PI
    from psvi.models import make_regressor_net

    cfg = f["cfg"]
    layers = cfg["layers"]
    model = make_regressor_net(layers[0][0], layers[0][1], 1, n_layers=len(layers) - 1,
                               mc_samples=cfg["S"]).to(DEV)
    torch.nn.utils.vector_to_parameters(_t(f["params0"]), model.parameters())
    ps = getattr(PI, cfg["cls"])(N=cfg["N"], D=layers[0][0], num_pseudo=cfg["M"],
                                 mc_samples=cfg["S"], tau=cfg["tau"], learn_z=True,
                                 lr0alpha=cfg["lr0alpha"], y_mean=cfg.get("y_mean"),
                                 y_std=cfg.get("y_std"))
    ps.model = model
    ps.u, ps.z, ps.v = (_t(f[k]).requires_grad_(True) for k in ("u0", "z0", "v0"))
    ps.learn_v = True
    ps.inner_it, ps.log_every, ps.scheduler_optim_net = cfg["T"], 10, None
    ps.optim_net = torch.optim.Adam(list(model.parameters()), cfg["lr0net"])
    ps.optim_u = torch.optim.Adam([ps.u], cfg["lr0u"])
    ps.optim_v = torch.optim.Adam([ps.v], cfg["lr0v"])
    ps.optim_z = torch.optim.Adam([ps.z], cfg["lr0z"])
    if cfg.get("alpha0") is not None:
        ps.alpha = _t([cfg["alpha0"]]).requires_grad_(True)
        ps.optim_alpha = torch.optim.Adam([ps.alpha], cfg["lr0alpha"])
    return ps, model


def _autograd_errors(f, ps, model, loss):
    g = torch.cat([q.grad.reshape(-1) for q in model.parameters()]).cpu().numpy()
    e = dict(value=rel(loss.item(), f["out"]), params=l2rel(g, f["grad_params"]))
    for key, t in (("u_grad", ps.u), ("v_grad", ps.v), ("z_grad", ps.z),
                   ("alpha_grad", getattr(ps, "alpha", None))):
        if key in f:
            e[key] = l2rel(t.grad.cpu().numpy(), f[key])
    return e


@pytest.mark.parametrize("name", fixture_names("r1") + fixture_names("r2"))
def test_class_objectives_backward(name):
    """PSVI*_regressor.inner_elbo / psvi_elbo as autograd nodes: one backward()
    delivers the reference's gradients to the parameters, u, v (alpha) and z."""
    f = load_fixture(name)
    ps, model = _obj(f)
    if f["cfg"]["kind"] == "inner":
        loss = ps.inner_elbo(eps=_t(f["eps"]))
    else:
        loss = ps.psvi_elbo(_t(f["xb"]), _t(f["yb"]), eps=_t(f["eps"]))
    loss.backward()
    e = _autograd_errors(f, ps, model, loss)
    print(name, {k: f"{x:.2e}" for k, x in e.items()})
    assert {"u_grad", "v_grad", "z_grad"} <= set(e)
    assert e.pop("value") < 1e-5
    for k, x in e.items():
        assert x < 1e-4, (k, x)


@pytest.mark.parametrize("name", fixture_names("r3"))
def test_nested_step_matches_reference(name):
    """One whole nested_step (T = 3, learn_z) of each of the three classes on
    the reference's draws: outer loss, final parameters, the hypergradients of
    u, v, z (alpha) and their Adam steps.  The hypergradient bar is
    max(1e-4, 4 x the error of the reference's own fp32 run on the same draws,
    recorded in the fixture)."""
    f = load_fixture(name)
    cfg = f["cfg"]
    ps, model = _obj(f)
    out = ps.nested_step(_t(f["xb"]), _t(f["yb"]), eps_inner=[_t(e) for e in f["eps_inner"]],
                         eps_outer=[_t(f["eps_outer"])]).item()
    print(f"{name}: out {out:.6f} (reference {float(f['out']):.6f})")
    assert rel(out, f["out"]) < 1e-5
    p = torch.nn.utils.parameters_to_vector(model.parameters()).detach().cpu().numpy()
    e = l2rel(p, f["params"])
    print(f"  params: l2rel {e:.2e} (reference fp32 {l2rel(f['params_fp32'], f['params']):.2e})")
    assert e < 1e-5
    hp = [("u_grad", ps.u, "u", cfg["lr0u"]), ("v_grad", ps.v, "v", cfg["lr0v"]),
          ("z_grad", ps.z, "z", cfg["lr0z"])]
    if cfg.get("alpha0") is not None:
        hp.append(("alpha_grad", ps.alpha, "alpha", cfg["lr0alpha"]))
    for key, t, vkey, lr in hp:
        got = t.grad.detach().cpu().numpy()
        own = l2rel(f[key + "_fp32"], f[key])
        e = l2rel(got, f[key])
        print(f"  {key}: l2rel {e:.2e} (reference fp32 {own:.2e})")
        assert e < max(1e-4, 4 * own), key
        big = np.abs(f[key]) > 1e-2 * np.abs(f[key]).max()
        assert np.abs(t.detach().cpu().numpy() - f[vkey])[big].max() < 1e-3 * lr, vkey
        assert not np.array_equal(t.detach().cpu().numpy(), f[vkey + "0"] if vkey != "alpha"
                                  else np.array([cfg["alpha0"]], np.float32))


@pytest.mark.parametrize("name", fixture_names("r4"))
def test_class_evaluate(name):
    """PSVILearnV_regressor.evaluate over the fixture's two test batches."""
    f = load_fixture(name)
    ps, _ = _obj(f)
    n = len(f["cfg"]["nts"])
    ps.test_loader = [(_t(f[f"xt{i}"]), _t(f[f"yt{i}"])) for i in range(n)]
    rmse, ll = ps.evaluate(eps=[_t(f[f"eps{i}"]) for i in range(n)])
    print(name, f"rmse {rmse.item():.6f} ll {ll.item():.6f}")
    assert rel(rmse.item(), f["rmse"]) < 1e-5
    assert rel(ll.item(), f["test_ll"]) < 1e-5


def test_run_psvi_results():
    """run_psvi end to end on a tiny synthetic regression set: the reference's
    results keys, one evaluation per log_every steps, u / z / v moved."""
    from torch.utils.data import TensorDataset

    from psvi.inference import PSVIAV_regressor

    g = torch.Generator().manual_seed(3)
    x = torch.randn(40, 3, generator=g)
    y = x @ torch.tensor([0.5, -1.0, 0.25]) + 0.1 * torch.randn(40, generator=g)
    ps = PSVIAV_regressor(train_dataset=TensorDataset(x[:32], y[:32]),
                          test_dataset=TensorDataset(x[32:], y[32:]), N=32, D=3, num_pseudo=4,
                          mc_samples=3, tau=4.0, y_mean=0.3, y_std=1.5, seed=1)
    res = ps.run_psvi(architecture="regressor_net", n_hidden=5, n_layers=2, inner_it=2,
                      data_minibatch=8, num_epochs=3, log_every=2)
    assert {"rmses", "lls", "csizes", "times", "went", "ness", "vent", "vs"} <= set(res)
    assert len(res["rmses"]) == len(res["lls"]) == len(res["vs"]) == len(res["alpha"]) == 2
    assert res["csizes"] == [4, 4] and np.isfinite(res["rmses"] + res["lls"]).all()
    assert all(float(t.grad.abs().max()) > 0 for t in (ps.u, ps.z, ps.v, ps.alpha))
    assert float(ps.alpha.detach().abs().max()) > 0
