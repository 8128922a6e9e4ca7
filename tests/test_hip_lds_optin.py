"""Every kernel family that launches with more than 64 KiB of dynamic LDS,
run on device 0 and then on device 1 of one process: each launch needs the
kernel's opt-in (allow_dynamic_lds, csrc/capi_plan.cpp) on the device it runs on,
so the second device only works if the opt-in is made per device (or is a
property of the kernel on all devices at once).  Every call must succeed on
both devices and device 1's outputs must equal device 0's bit for bit: the
kernels add in fixed orders (csrc/block_reduce.hpp) and use no float atomics.

Dynamic LDS of each launch, from the launcher's own size function (all above
65,536):
  laplace_fit    Nu 300, d 64 (row stride 65): lap_fit_lds = 8 (512 + 256 +
                 300) + 4 * 300 * 65 = 86,544 bytes
  giga_step      n_data 2048, S 1100: 8 (3 * 2048 + 2 * 1100) = 66,752 bytes
  mfvi_fit       8 -> 50 -> 50 -> 1 (n_tot 3051, hs 51, xs 9), B 16, S 2, LDS
                 placement, RB 16: mffit_lds = 8 * 512 + 4 (10 * 3051 + 16 * 9
                 + 4 * 16 * 51) = 139,768 bytes
  predict_scores 20 -> 100 -> 90 -> 3 (hs 101, xs 21), rows_per_draw 64: RG
                 64, W tile 90 * 101 floats: pred_lds = 8 * 512 + 4 (9090 +
                 64 * 226) = 98,312 bytes.  (A 100 -> 100 layer cannot be a
                 plan: psvi_plan_create refuses it, PSVI_EUNSUP, because the
                 network kernel's own carve for it passes 160 KiB at any M.)
  inner_step     full-cov 64 -> 40 -> 40 -> 2, S 2, M 100: two role workgroups
                 per sample, 6 pseudopoint chunks of 17 rows (padded to 32):
                 the plan's net_lds = 80,176 bytes

The one figure of inner_step that is not compared bit for bit is the ELBO it
returns: its fp64 partials are added with atomics in arrival order (see
test_hip_net_lds.py), so it is held to 1e-12 relative; the parameters and the
Adam moments the step writes are compared exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NET = [(64, 40), (40, 40), (40, 2)]
PRED = [(20, 100), (100, 90), (90, 3)]
FIT = [(8, 50), (50, 50), (50, 1)]


def _inputs():
    """Host inputs of every call, made once."""
    rng = np.random.default_rng(11)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    h = {}
    # laplace_fit: Nu 300, d 64 (ones column last), T 2, S 2
    x = rng.normal(size=(300, 64))
    x[:, -1] = 1.0
    h["lap"] = dict(x=f32(x), y=f32(rng.integers(0, 2, size=300)),
                    w=f32(rng.uniform(0.5, 2.0, size=300)), theta=f32(0.1 * rng.normal(size=64)),
                    eps=f32(rng.normal(size=(2, 64))))
    # giga_step: n_data 2048, S 1100, d 4
    r = rng.normal(size=(2048, 4))
    r[:, -1] = 1.0
    h["giga"] = dict(samples=f32(rng.normal(size=(1100, 4))), rows=f32(r),
                     labels=f32(rng.integers(0, 2, size=2048)), lw=f32(np.zeros(1100)))
    # mfvi_fit: B 16, S 2, T 2, G 2
    P = 2 * sum(i * o + o for i, o in FIT)
    mu_rho = lambda n: np.concatenate([0.3 * rng.normal(size=n), rng.uniform(-4.0, -2.0, size=n)])
    h["fit"] = dict(x=f32(rng.normal(size=(16, 8))), y=f32(rng.normal(size=16)),
                    params=f32(np.stack([np.concatenate([mu_rho(i * o + o) for i, o in FIT])
                                         for _ in range(2)])))
    assert h["fit"]["params"].shape == (2, P)
    # predict_scores: S 2, 64 rows on one eps block
    h["pred"] = dict(x=f32(rng.normal(size=(64, 20))), z=rng.integers(0, 3, size=64).astype(np.int32),
                     params=f32(np.concatenate([mu_rho(i * o + o) for i, o in PRED])))
    # inner_step: full-cov, S 2, M 100
    parts = []
    for i, o in NET:
        n = i * o + o
        parts += [0.1 * rng.normal(size=n), rng.uniform(-5.0, -3.0, size=n),
                  (0.15 / n ** 0.5) * rng.normal(size=(n - 1) * (n - 2) // 2)]
    h["net"] = dict(u=f32(rng.normal(size=(100, 64))), z=rng.integers(0, 2, size=100).astype(np.int32),
                    w=f32(np.full(100, 3.0)), params=f32(np.concatenate(parts)))
    h["rng"] = rng
    return h


def _run_all(h, dev):
    """Every call on device `dev` (current for the plans and the launches);
    returns the outputs as host arrays."""
    from psvi.runtime import (InnerLoopPlan, giga_step, laplace_fit, mfvi_fit, mfvi_fit_query,
                              predict_scores)

    def t(a):
        return torch.tensor(a, device=f"cuda:{dev}")

    out = {}
    with torch.cuda.device(dev):
        c = h["lap"]
        theta = t(c["theta"])
        o = laplace_fit(t(c["x"]), t(c["y"]), t(c["w"]), theta, T=2, lr=0.05, eps=t(c["eps"]),
                        want_loss=True)
        out.update(lap_theta=theta, lap_prec=o["prec"], lap_samples=o["samples"], lap_loss=o["loss"])

        c = h["giga"]
        o = giga_step(t(c["samples"]), t(c["rows"]), t(c["labels"]), t(c["lw"]))
        out.update(giga_score=o["score"], giga_lw=o["lw"], giga_result=o["result"])

        c = h["fit"]
        assert mfvi_fit_query(FIT, 2, 16)["placement"] == "lds"
        E = mfvi_fit_query(FIT, 2, 16)["eps_count"]
        o = mfvi_fit(FIT, 2, t(c["x"]), t(c["y"]), 1.5, [1.0, 4.0], t(c["params"]), T=2, lr=0.01,
                     eps=t(h["fit_eps"](E)))
        out.update(fit_params=o["params"], fit_m=o["adam_m"], fit_v=o["adam_v"], fit_loss=o["loss"])

        c = h["pred"]
        plan = InnerLoopPlan("meanfield", PRED, 2, 3)  # M is not read
        o = predict_scores(plan, t(c["x"]), t(c["z"]), t(h["pred_eps"](plan.eps_count)),
                           t(c["params"]), 64, stats=True)
        out.update({"pred_" + k: v for k, v in o.items()})

        c = h["net"]
        plan = InnerLoopPlan("fullcov", NET, 2, 100)
        params = t(c["params"])
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        elbo = plan.inner_step(t(c["u"]), t(c["z"]), t(c["w"]), t(h["net_eps"](plan.eps_count)),
                               params, m, v, step=1, lr=1e-3)
        out.update(net_params=params, net_m=m, net_v=v, net_elbo=elbo)
        torch.cuda.synchronize()
    return {k: a.cpu().numpy() for k, a in out.items()}


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_large_lds_launches_on_two_devices():
    h = _inputs()
    # the draws, sized by the library's counts, made once and shared
    cache = {}

    def draws(key, per):
        def make(n):
            if key not in cache:
                cache[key] = h["rng"].normal(size=per(n)).astype(np.float32)
            return cache[key]
        return make

    h["fit_eps"] = draws("fit", lambda E: (2, 2, E))
    h["pred_eps"] = draws("pred", lambda E: E)
    h["net_eps"] = draws("net", lambda E: E)
    a = _run_all(h, 0)   # any failed launch raises PsviError here ...
    b = _run_all(h, 1)   # ... or here
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert np.isfinite(a[k]).all(), k
        if k == "net_elbo":  # fp64 atomics: order only
            assert abs(a[k][0] - b[k][0]) <= 1e-12 * abs(a[k][0]), (k, a[k], b[k])
        else:
            assert np.array_equal(a[k], b[k]), k
