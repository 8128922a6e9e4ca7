"""Host side of the Gaussian-likelihood (regressor) family, no GPU: the model
builder and gaussian_fn against the reference's inner_elbo fixtures in
float64, the parameter order, the C ABI's refusals for psvi_plan_create_lik
(no kernel launch) and the geometry of a Gaussian plan."""
import ctypes

import numpy as np
import pytest
import torch

from golden_util import fixture_names, load_fixture, rel

R1 = fixture_names("r1")


def _model(f):
    from psvi.models import make_regressor_net

    cfg = f["cfg"]
    layers = cfg["layers"]
    net = make_regressor_net(layers[0][0], layers[0][1], 1, n_layers=len(layers) - 1,
                             mc_samples=cfg["S"]).double()
    torch.nn.utils.vector_to_parameters(torch.tensor(f["params0"], dtype=torch.float64),
                                        net.parameters())
    return net


def test_fixtures_present():
    assert len(R1) == 4 and len(fixture_names("r2")) == 8 and len(fixture_names("r4")) == 4
    assert sorted(load_fixture(n)["cfg"]["cls"] for n in fixture_names("r3")) == [
        "PSVIAV_regressor", "PSVILearnV_regressor", "PSVI_regressor"]


def test_regressor_classes_and_refusals():
    """The public classes with the reference's keywords, and what they refuse
    before any GPU work: other trainers / inits, world > 1, full-covariance
    and LeNet models; PSVI itself keeps refusing a Gaussian distr_fn."""
    from psvi.inference import PSVI, PSVI_regressor, PSVIAV_regressor, PSVILearnV_regressor
    from psvi.models import gaussian_fn, make_fc2net, make_lenet, make_regressor_net

    assert issubclass(PSVIAV_regressor, PSVILearnV_regressor)
    assert issubclass(PSVILearnV_regressor, PSVI_regressor)
    kw = dict(N=20, D=3, num_pseudo=4, mc_samples=3, tau=4.0, y_mean=0.5, y_std=2.0)
    ps = PSVIAV_regressor(**kw)
    assert ps.learn_z and ps.learn_v and ps.parameterised and ps.tau == 4.0
    assert ps.alpha.shape == (1,) and ps.results["alpha"] == []
    assert ps.distr_fn(torch.zeros(2)).scale[0].item() == pytest.approx(0.5)
    base = PSVI_regressor(**kw)
    assert not base.learn_v and not base.parameterised
    assert torch.allclose(base.v, torch.full((4,), 0.25, device=base.v.device))
    with pytest.raises(NotImplementedError):
        PSVI_regressor(world=2, **kw)
    with pytest.raises(NotImplementedError):
        PSVI(N=20, D=3, num_pseudo=4, distr_fn=gaussian_fn)
    for bad in (dict(trainer="hyper"), dict(trainer="joint"), dict(init_args="random")):
        with pytest.raises(NotImplementedError):
            base.run_psvi(architecture="regressor_net", **bad)
    base.u, base.z = torch.zeros(4, 3), torch.zeros(4)
    for model in (make_fc2net(3, 5, 1, mc_samples=3), make_lenet(mc_samples=3)):
        with pytest.raises(NotImplementedError):
            base.inner_elbo(model=model)
    with pytest.raises(NotImplementedError):   # two outputs: not the Gaussian head's shape
        base.inner_elbo(model=make_regressor_net(3, 5, 2, mc_samples=3))
    for step in (base.hyper_step, base.joint_step, base.alternating_step):
        with pytest.raises(NotImplementedError):
            step(torch.zeros(2, 3), torch.zeros(2))


def test_regressor_net_modules_and_parameter_order():
    from psvi.models import VILinear, make_regressor_net, model_spec

    net = make_regressor_net(6, 24, n_layers=2, mc_samples=8)
    assert [n for n, _ in net.named_children()] == ["lin0", "nonl0", "lin1", "nonl1", "regressor"]
    assert isinstance(net.regressor, VILinear) and net.regressor.out_features == 1
    assert model_spec(net) == ("meanfield", [(6, 24), (24, 24), (24, 1)], 1.0, 8)
    names = [n for n, _ in net.named_parameters()]
    assert names[:4] == ["lin0.weight", "lin0.bias", "lin0._weight_sd", "lin0._bias_sd"]
    f = load_fixture("r1_inner_large_t4")
    assert sum(p.numel() for p in net.parameters()) == f["params0"].size


@pytest.mark.parametrize("name", R1)
def test_torch_forward_and_gaussian_fn_reproduce_inner_elbo(name):
    """The host modules' torch forward on the fixture's draws and gaussian_fn
    give the reference's inner_elbo value in float64 (which also pins the
    parameter order of make_regressor_net to the fixture's params0)."""
    import torch.distributions.normal as normal_mod

    from psvi.models import VILinear, gaussian_fn

    f = load_fixture(name)
    cfg = f["cfg"]
    net = _model(f)
    S, eps, pos = cfg["S"], torch.tensor(f["eps"], dtype=torch.float64), [0]
    orig = normal_mod._standard_normal

    def replay(shape, dtype, device):
        n = int(np.prod(shape))
        out = eps[pos[0]:pos[0] + n].reshape(shape).to(dtype)
        pos[0] += n
        return out

    normal_mod._standard_normal = replay
    try:
        out = net(torch.tensor(f["u0"], dtype=torch.float64)).squeeze(-1)
    finally:
        normal_mod._standard_normal = orig
    assert pos[0] == eps.numel() and out.shape == (S, cfg["M"])
    w = cfg["N"] * torch.softmax(torch.tensor(f["v0"], dtype=torch.float64), 0)
    dist = gaussian_fn(out, 1.0 / np.sqrt(cfg["tau"]))
    nll = -dist.log_prob(torch.tensor(f["z0"], dtype=torch.float64))
    kl = sum(m.kl() for m in net.modules() if isinstance(m, VILinear))
    val = float(nll.matmul(w).sum() + kl)
    assert rel(val, f["out"]) < 1e-9, (val, float(f["out"]))


def _create(fam, dims, S, M, world, lik):
    from psvi.runtime import _lib

    lib = _lib.load()
    d = _lib.NetDesc()
    d.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        d.dims[i] = v
    d.S, d.M, d.prior_sd = S, M, 1.0
    h = ctypes.c_void_p()
    rc = lib.psvi_plan_create_lik(fam, ctypes.byref(d), world, 0,
                                  ctypes.byref(lik) if lik is not None else None, ctypes.byref(h))
    msg = lib.psvi_last_error()
    return rc, msg, h, lib


def test_plan_create_lik_refusals():
    from psvi.runtime import _lib

    G = lambda tau: _lib.Likelihood(_lib.LIK_GAUSSIAN, tau)
    for args, code in (((_lib.FAMILY_FULLCOV, [3, 10, 1], 3, 5, 1, G(0.1)), -3),
                       ((_lib.FAMILY_LENET, [3, 10, 1], 3, 5, 1, G(0.1)), -3),
                       ((_lib.FAMILY_MEANFIELD, [3, 10, 1], 4, 5, 2, G(0.1)), -3),
                       ((_lib.FAMILY_MEANFIELD, [3, 10, 2], 3, 5, 1, G(0.1)), -1),
                       ((_lib.FAMILY_MEANFIELD, [3, 10, 1], 3, 5, 1, G(0.0)), -1),
                       ((_lib.FAMILY_MEANFIELD, [3, 10, 1], 3, 5, 1, G(-1.0)), -1),
                       ((_lib.FAMILY_MEANFIELD, [3, 10, 1], 3, 5, 1, G(float("nan"))), -1),
                       ((_lib.FAMILY_MEANFIELD, [3, 10, 1], 3, 5, 1, _lib.Likelihood(9, 1.0)), -1)):
        rc, msg, h, _ = _create(*args)
        assert rc == code and msg and not h.value, (args[:5], rc, msg)


def test_plan_create_lik_geometry_and_default():
    from psvi.runtime import _lib

    counts = []
    for lik in (_lib.Likelihood(_lib.LIK_GAUSSIAN, 4.0), None,
                _lib.Likelihood(_lib.LIK_CATEGORICAL, 0.0)):
        rc, _, h, lib = _create(_lib.FAMILY_MEANFIELD, [6, 24, 24, 1], 8, 37, 1, lik)
        assert rc == 0 and h.value
        v = ctypes.c_int64()
        row = []
        for key in (_lib.Q_PARAM_COUNT, _lib.Q_EPS_COUNT, _lib.Q_ACC_COUNT):
            assert lib.psvi_plan_query(h, key, ctypes.byref(v)) == 0
            row.append(v.value)
        counts.append(row)
        lib.psvi_plan_destroy(h)
    n_tot = 6 * 24 + 24 + 24 * 24 + 24 + 24 + 1
    assert counts[0] == [2 * n_tot, 8 * n_tot, 2 * n_tot]
    assert counts[0] == counts[1] == counts[2]


def test_targets_kind_refusals_at_the_abi():
    """psvi_outer_elbo_grad_ex (with grad_z), psvi_evaluate and
    psvi_evaluate_regression take their targets through the same `z` slot; a
    plan of the wrong likelihood is refused with PSVI_ESTATE before anything
    is launched.  A plan created without a HIP device is refused one check
    earlier, with PSVI_ESTATE too, whatever its kind."""
    from psvi.runtime import _lib

    dims, S, M = [3, 10, 1], 3, 5
    have_dev = torch.cuda.is_available()
    no_dev = b"plan was created without a HIP device"
    buf = (ctypes.c_float * (S * 64))()   # never read: every call is refused first
    b = ctypes.addressof(buf)
    for lik in (None, _lib.Likelihood(_lib.LIK_GAUSSIAN, 4.0)):
        rc, _, h, lib = _create(_lib.FAMILY_MEANFIELD, dims, S, M, 1, lik)
        assert rc == 0 and h.value
        gauss = lik is not None
        outer = lambda: lib.psvi_outer_elbo_grad_ex(h, 2, b, b, b, b, b, b, b, None, None, b, None,
                                                    None, 0, None)
        evalr = lambda: lib.psvi_evaluate_regression(h, 2, b, b, b, b, b, 0, 0.0, 1.0, None, b,
                                                     None, 0, None)
        evalc = lambda: lib.psvi_evaluate(h, 2, b, b, b, b, b, 0, None, b, None, 0, None)
        if not have_dev:
            calls = [(outer, no_dev), (evalr, no_dev), (evalc, no_dev)]
        elif gauss:   # the right kind for outer / evalr: not called (they would go on)
            calls = [(evalc, b"psvi_evaluate_regression")]
        else:
            calls = [(outer, b"grad_z needs a Gaussian-likelihood plan"),
                     (evalr, b"needs a Gaussian-likelihood plan")]
        for call, text in calls:
            assert call() == -4 and text in lib.psvi_last_error(), (gauss, text)
        lib.psvi_plan_destroy(h)


def test_engine_likelihood_keyword():
    from psvi.runtime import InnerLoopPlan

    p = InnerLoopPlan("meanfield", [(3, 10), (10, 1)], 3, 5, likelihood=("gaussian", 0.1))
    assert p.likelihood == "gaussian" and p.tau == pytest.approx(0.1)
    assert p.param_count == 2 * (3 * 10 + 10 + 10 + 1) and p.eps_count == 3 * (3 * 10 + 10 + 10 + 1)
    assert InnerLoopPlan("meanfield", [(3, 10), (10, 2)], 3, 5).likelihood == "categorical"
    with pytest.raises(ValueError):
        InnerLoopPlan("meanfield", [(3, 10), (10, 1)], 3, 5, likelihood=("poisson", 1.0))
