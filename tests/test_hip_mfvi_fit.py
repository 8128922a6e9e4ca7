"""psvi_mfvi_fit on the device: the fused MFVI regressor fit against the
float64 restatement (tests/mfvi_regr_util.py) and the reference's own fit
(fixtures m*), within the project's parity bound of 1e-4 relative (golden_util.rel:
largest deviation over the largest reference magnitude); both state placements;
the bitwise properties of the header (run to run, member independence, Philox
against replay, a fit split over two calls)."""
import numpy as np
import pytest
import torch

import mfvi_regr_util as R
from golden_util import fixture_names, load_fixture, rel

pytestmark = pytest.mark.gpu

TOL = 1e-4
DEV = "cuda"


def _t(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _case(D, H, nh, B, S, T, G, seed, init_sd=0.05):
    rng = np.random.default_rng(seed)
    layers = R.layer_table(D, H, nh)
    P, E = R.counts(layers, S)
    x = rng.standard_normal((B, D)).astype(np.float32)
    y = rng.standard_normal(B).astype(np.float32)
    p0 = np.stack([R.init_params(layers, init_sd, rng) for _ in range(G)])
    eps = rng.standard_normal((G, T, E)).astype(np.float32)
    return dict(layers=layers, S=S, B=B, T=T, G=G, P=P, E=E, x=x, y=y, p0=p0, eps=eps,
                scale=37.0 / B, lr=1e-2)


def _run(c, taus, eps="replay", T=None, **kw):
    from psvi.runtime import mfvi_fit

    T = c["T"] if T is None else T
    params = _t(c["p0"][:len(taus)])
    e = _t(c["eps"][:len(taus), :T]) if eps == "replay" else None
    out = mfvi_fit(c["layers"], c["S"], _t(c["x"]), _t(c["y"]), c["scale"], taus, params, T,
                   c["lr"], eps=e, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(out, c, taus, what):
    worst = 0.0
    for g, tau in enumerate(taus):
        L, p, m, v = R.fit(c["layers"], c["S"], c["x"], c["y"], c["scale"], tau, c["p0"][g],
                           c["eps"][g], c["lr"])
        errs = dict(loss=rel(out["loss"][g], L), params=rel(out["params"][g], p),
                    adam_m=rel(out["adam_m"][g], m), adam_v=rel(out["adam_v"][g], v))
        print(f"{what} member {g} tau {tau}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        worst = max(worst, *errs.values())
    return worst


def _stepwise(c, g, tau):
    """The existing path: psvi_elbo_grad + psvi_adam_update(kind="torch") per step."""
    from psvi.runtime import InnerLoopPlan, adam_update_

    plan = InnerLoopPlan("meanfield", c["layers"], c["S"], c["B"], likelihood=("gaussian", tau))
    p = _t(c["p0"][g])
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    x, y, w = _t(c["x"]), _t(c["y"]), torch.full((c["B"],), c["scale"], device=DEV)
    losses = []
    for t in range(c["T"]):
        loss, grad = plan.elbo_grad(x, y, w, _t(c["eps"][g, t]), p)
        adam_update_(p, grad, m, v, step=t + 1, lr=c["lr"], kind="torch")
        losses.append(loss.item())
    return dict(loss=np.array([losses]), params=p.cpu().numpy()[None],
                adam_m=m.cpu().numpy()[None], adam_v=v.cpu().numpy()[None])


SHAPES = {
    "d3_h4": (dict(D=3, H=4, nh=1, B=5, S=3, T=4, G=2, seed=1), [0.5, 4.0]),
    "d7_h9x2_b67": (dict(D=7, H=9, nh=2, B=67, S=5, T=6, G=2, seed=2), [0.5, 4.0]),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_parity_with_restatement(name):
    from psvi.runtime import mfvi_fit_query

    kw, taus = SHAPES[name]
    c = _case(**kw)
    assert mfvi_fit_query(c["layers"], c["S"], c["B"])["placement"] == "lds"
    fused = _check(_run(c, taus), c, taus, f"fused {name}")
    step = 0.0
    for g, tau in enumerate(taus):
        cg = dict(c, p0=c["p0"][g:g + 1], eps=c["eps"][g:g + 1])
        step = max(step, _check(_stepwise(c, g, tau), cg, [tau], f"stepwise {name} g{g}"))
    print(f"{name}: fused {fused:.2e}, step by step {step:.2e}")
    assert fused < TOL
    assert step < TOL


@pytest.mark.parametrize("name", fixture_names("m"))
def test_reference_fixtures(name):
    f = load_fixture(name)
    cfg = f["cfg"]
    c = dict(layers=cfg["layers"], S=cfg["S"], B=cfg["B"], T=cfg["T"], G=1, x=f["x"], y=f["y"],
             p0=f["params0"][None], eps=f["eps"][None], scale=cfg["scale"], lr=cfg["lr"])
    out = _run(c, [cfg["tau"]])
    errs = dict(loss=rel(out["loss"][0], f["losses"]), params=rel(out["params"][0], f["params"]))
    print(f"fixture {name}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert max(errs.values()) < TOL


def test_global_placement():
    from psvi.runtime import mfvi_fit_query

    c = _case(D=128, H=64, nh=3, B=8, S=2, T=2, G=2, seed=3)
    q = mfvi_fit_query(c["layers"], c["S"], c["B"])
    assert q["placement"] == "global" and q["ws_bytes"] == 4 * c["P"]
    taus = [0.5, 4.0]
    assert _check(_run(c, taus), c, taus, "global") < TOL
    # D = 90, H = 50 x 2 spills too; the default regressor (D = 13) does not
    c = _case(D=90, H=50, nh=2, B=9, S=2, T=2, G=1, seed=4)
    assert mfvi_fit_query(c["layers"], c["S"], c["B"])["placement"] == "global"
    assert _check(_run(c, [2.0]), c, [2.0], "global d90") < TOL
    assert mfvi_fit_query(R.layer_table(13, 50, 2), 4, 128)["placement"] == "lds"


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("params", "adam_m", "adam_v", "loss"))


@pytest.mark.parametrize("placement", ["lds", "global"])
def test_bitwise_properties(placement):
    from psvi.runtime import mfvi_fit_query, randn_

    if placement == "lds":
        c = _case(D=7, H=9, nh=2, B=67, S=5, T=6, G=3, seed=5)
    else:
        c = _case(D=128, H=64, nh=3, B=8, S=2, T=6, G=3, seed=6)
    assert mfvi_fit_query(c["layers"], c["S"], c["B"])["placement"] == placement
    taus = [0.5, 4.0, 30.0]
    a = _run(c, taus)
    assert _same(a, _run(c, taus)), "two runs differ"
    # member g of the G = 3 call against the G = 1 call with its inputs
    for g in range(3):
        one = _run(dict(c, p0=c["p0"][g:g + 1], eps=c["eps"][g:g + 1]), taus[g:g + 1])
        assert all(np.array_equal(one[k][0], a[k][g]) for k in one), f"member {g} depends on G"
    # Philox mode against replay of psvi_randn's output at the stated offsets
    stride = (c["E"] + 3) // 4 * 4
    seed, offs = 1234567, [8, 4 * 1000 * stride, 4]
    eps = torch.empty(3, c["T"], c["E"], device=DEV)
    for g in range(3):
        for t in range(c["T"]):
            randn_(eps[g, t], seed, offs[g] + t * stride)
    cr = dict(c, eps=eps.cpu().numpy())
    ph = _run(c, taus, eps="philox", seed=seed, offsets=offs)
    assert _same(ph, _run(cr, taus)), "Philox and replay differ"
    # T = 6 as 4 + 2: params, moments, step count and offset carried over
    for mode, cc, kw1, kw2 in (
            ("replay", c, {}, {}),
            ("philox", c, dict(seed=seed, offsets=offs),
             dict(seed=seed, offsets=[o + 4 * stride for o in offs]))):
        full = a if mode == "replay" else ph
        first = _run(cc, taus, eps=mode, T=4, **kw1)
        c2 = dict(cc, p0=first["params"], eps=cc["eps"][:, 4:])
        second = _run(c2, taus, eps=mode, T=2, adam_m=_t(first["adam_m"]),
                      adam_v=_t(first["adam_v"]), step0=4, **kw2)
        for k in ("params", "adam_m", "adam_v"):
            assert np.array_equal(second[k], full[k]), f"{mode}: split {k} differs"
        assert np.array_equal(np.concatenate([first["loss"], second["loss"]], 1), full["loss"])
