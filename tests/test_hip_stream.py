"""The streaming fused full-cov update (mvn_stream_kernel: persistent workgroup
per CU, G / eps blocks in LDS, Adam on the accumulators, the next step's
sample from the registers) against the chunked packed-state update on the
same inputs, and the whole inner loop at C3's shape against the oracle.

Same inputs, same arithmetic per corr entry (dL sums the samples in the same
pairs and order; mean / sd sums too), so corr / m / v agree to a few ulp (fma
contraction of the Adam epilogue); x' sums in another order (fp32, 1e-6)."""
import numpy as np
import pytest
import torch

import psvi_oracle as O
from golden_util import l2rel, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
DBG_STREAM_OFF = 10


def _lib():
    from psvi.runtime import _lib as L

    return L.load()


def _case(layers, S, seed):
    rng = np.random.default_rng(seed)
    parts = []
    for din, dout in layers:
        n = din * dout + dout
        parts += [0.1 * rng.standard_normal(n), rng.uniform(-5, -3, n),
                  (0.15 / np.sqrt(n)) * rng.standard_normal((n - 1) * (n - 2) // 2)]
    p = np.concatenate(parts).astype(np.float32)
    m = (1e-3 * rng.standard_normal(p.size)).astype(np.float32)
    v = (1e-6 * rng.random(p.size)).astype(np.float32)
    return rng, p, m, v


# the stream kernel runs at S = 128 (stream_ok in kernels_mvn_stream.hip)
SHAPES = [([(64, 40), (40, 40), (40, 2)], 128),   # C3
          ([(7, 5), (5, 3)], 128),                 # n = 40, 18: one partial band each
          ([(30, 33), (33, 2)], 128),              # n = 1023, 68
          ([(12, 20), (20, 4)], 128)]


@pytest.mark.parametrize("layers,S", SHAPES)
@pytest.mark.parametrize("kind", ["higher", "hypergrad"])
def test_stream_update_equals_chunked(layers, S, kind):
    from psvi.runtime import InnerLoopPlan

    plan = InnerLoopPlan("fullcov", layers, S, 10)
    assert plan.tiled_floats > 0
    rng, p0, m0, v0 = _case(layers, S, 11)
    t = lambda a: torch.tensor(a, device=DEV)
    eps0 = t(rng.standard_normal(plan.eps_count).astype(np.float32))
    eps1 = t(rng.standard_normal(plan.eps_count).astype(np.float32))
    gs = t((0.05 * rng.standard_normal(plan.xshard_count)).astype(np.float32))
    out = {}
    for mode in ("packed", "stream", "chunked", "stream"):
        p, m, v = t(p0), t(m0), t(v0)
        kl = torch.zeros(1, dtype=torch.float64, device=DEV)
        x = torch.full((plan.xshard_count,), float("nan"), device=DEV)
        if mode == "packed":
            plan.mvn_update(eps0, gs, p, m, v, step=3, lr=1e-3, kind=kind, kl_out=kl,
                            eps_next=eps1, x_next=x)
        else:
            _lib().psvi_debug_set(DBG_STREAM_OFF, 1 if mode == "chunked" else 0)
            try:
                ts = plan.tiled_state()
                plan.tiled_convert(p, m, v, ts, True)
                plan.mvn_update_tiled(eps0, gs, p, m, v, ts, step=3, lr=1e-3, kind=kind,
                                      kl_out=kl, eps_next=eps1, x_next=x)
                plan.tiled_convert(p, m, v, ts, False)
            finally:
                _lib().psvi_debug_set(DBG_STREAM_OFF, 0)
        torch.cuda.synchronize()
        res = [a.cpu().numpy() for a in (p, m, v, x)] + [kl.item()]
        if mode in out:  # the stream kernel twice: x' (the in-launch band combine adds
            # a band's slots in slot order, whichever segment arrives last) and the
            # state are bitwise run to run
            for a, b in zip(res[:4], out[mode][:4]):
                assert np.array_equal(a, b), mode
        out[mode] = res
    ref = out["packed"]
    for mode in ("stream", "chunked"):
        p, m, v, x, kl = out[mode]
        assert np.isfinite(x).all(), mode
        assert l2rel(x, ref[3]) < 1e-6, (mode, l2rel(x, ref[3]))
        assert rel(kl, ref[4]) < 1e-6, mode
        for a, b, what in ((p, ref[0], "p"), (m, ref[1], "m"), (v, ref[2], "v")):
            d = np.abs(a.astype(np.float64) - b)
            assert d.max() <= 1e-6 * max(np.abs(b).max(), 1e-30), (mode, what, d.max())
    # corr / m / v: the same arithmetic in both kernels (the sample sums in the
    # same pairs and order), up to the compiler's fma contraction of Adam
    for k in range(3):
        a, b = out["stream"][k].astype(np.float64), out["chunked"][k]
        assert np.abs(a - b).max() <= 1e-7 * np.abs(b).max(), k


def test_mean_sd_bitwise_across_routes():
    """The mean / sd entries of params, m and v bit for bit the same from the
    chunked packed kernel, the chunked tiled kernel (converted back) and the
    fp32 streaming kernel: all three sum the samples in the same order and go
    through one diagonal head (diag_head / adam_diag in mvn_common.hpp).
    n = 91 (two bands, a 27-row tail) and n = 28 (one band)."""
    from psvi.runtime import InnerLoopPlan

    DBG_STREAM_BF_OFF = 24
    layers, S = [(6, 13), (13, 2)], 128
    plan = InnerLoopPlan("fullcov", layers, S, 10)
    rng, p0, m0, v0 = _case(layers, S, 17)
    t = lambda a: torch.tensor(a, device=DEV)
    eps0 = t(rng.standard_normal(plan.eps_count).astype(np.float32))
    eps1 = t(rng.standard_normal(plan.eps_count).astype(np.float32))
    gs = t((0.05 * rng.standard_normal(plan.xshard_count)).astype(np.float32))
    head = []  # the mean and sd entries: the first 2 n of each layer's block
    off = 0
    for din, dout in layers:
        n = din * dout + dout
        head.append(np.arange(off, off + 2 * n))
        off += 2 * n + (n - 1) * (n - 2) // 2
    head = np.concatenate(head)
    out = {}
    for route in ("packed", "tiled", "stream"):
        p, m, v = t(p0), t(m0), t(v0)
        kl = torch.zeros(1, dtype=torch.float64, device=DEV)
        kw = dict(step=3, lr=1e-3, kind="higher", kl_out=kl, include_kl=True)
        if route == "packed":
            plan.mvn_update(eps0, gs, p, m, v, **kw)
        else:
            ts = plan.tiled_state()
            plan.tiled_convert(p, m, v, ts, True)
            if route == "tiled":  # no next step: the chunked tiled form
                plan.mvn_update_tiled(eps0, gs, p, m, v, ts, **kw)
            else:
                x = torch.empty(plan.xshard_count, device=DEV)
                _lib().psvi_debug_set(DBG_STREAM_BF_OFF, 1)
                try:
                    plan.mvn_update_tiled(eps0, gs, p, m, v, ts, eps_next=eps1, x_next=x, **kw)
                finally:
                    _lib().psvi_debug_set(DBG_STREAM_BF_OFF, 0)
            plan.tiled_convert(p, m, v, ts, False)
        torch.cuda.synchronize()
        out[route] = [a.cpu().numpy()[head] for a in (p, m, v)]
    assert not np.array_equal(out["packed"][0], p0[head])  # the step moved them
    for route in ("tiled", "stream"):
        for a, b, what in zip(out[route], out["packed"], "pmv"):
            nd = int((a != b).sum())
            print(f"{route} vs packed, {what}: {nd} of {a.size} mean / sd entries differ")
            assert np.array_equal(a, b), (route, what, nd)


def test_c3_inner_loop_stream_matches_oracle():
    """Three chained C3 steps through psvi_inner_loop (fused, tiled, streaming)
    against the chunked kernel's loop (tight) and the float64 oracle's
    trajectory (Adam turns sub-rounding gradient entries into +-lr steps, so
    both fp32 paths sit the same distance from it)."""
    from psvi.runtime import InnerLoopPlan

    layers, S, M, T = [(64, 40), (40, 40), (40, 2)], 128, 100, 3
    rng = np.random.default_rng(5)
    _, p0, _, _ = _case(layers, S, 5)
    u = rng.standard_normal((M, 64)).astype(np.float32)
    z = rng.integers(0, 2, M).astype(np.int32)
    w = O.coreset_weights(0.3 * rng.standard_normal(M), 800).astype(np.float32)
    plan = InnerLoopPlan("fullcov", layers, S, M)
    eps = rng.standard_normal((T, plan.eps_count)).astype(np.float32)
    t = lambda a, d=torch.float32: torch.tensor(a, dtype=d, device=DEV)
    res = {}
    for off in (0, 1):
        _lib().psvi_debug_set(DBG_STREAM_OFF, off)
        try:
            p = t(p0)
            m, v = torch.zeros_like(p), torch.zeros_like(p)
            e = plan.inner_loop(t(u), t(z, torch.int32), t(w), p, m, v, T, 1e-3, eps=t(eps))
            res[off] = (e.cpu().numpy(), p.cpu().numpy())
        finally:
            _lib().psvi_debug_set(DBG_STREAM_OFF, 0)
    o_elbo, _, o_traj, _, _ = O.run_inner_loop("mvn", layers, p0, u, z, w, eps, S, 1e-3, "higher")
    (es, ps), (ec, pc) = res[0], res[1]
    assert np.all(np.abs(es - o_elbo) <= 1e-5 * np.abs(o_elbo)), (es, o_elbo)
    assert np.all(np.abs(es - ec) <= 1e-6 * np.abs(ec))
    # the two kernels add x' partials in different orders (the streaming
    # kernel per run segment, its run partition tuned for speed; the chunked
    # one per chunk), and Adam's normalisation turns rounding-level gradient
    # differences of near-zero entries into +-lr steps: the parameters are held
    # to each other loosely and to the oracle below
    assert l2rel(ps, pc) < 1e-4, l2rel(ps, pc)
    assert np.abs(ps - pc).max() <= 2 * T * 1e-3
    e_s, e_c = l2rel(ps, o_traj[-1]), l2rel(pc, o_traj[-1])
    print(f"C3 T={T}: params l2rel vs oracle stream {e_s:.2e} chunked {e_c:.2e}")
    assert e_s < 2 * e_c + 1e-6 and e_s < 1e-3
    assert np.abs(ps - o_traj[-1]).max() <= 2 * T * 1e-3


@pytest.mark.parametrize("kind", ["higher", "hypergrad"])
def test_stream_step_gradient_matches_oracle(kind):
    """The gradient the streaming kernel applies, pinned to the float64
    oracle at C3: one tiled stream step from zero Adam moments leaves m = (1 -
    beta1) g exactly (one fp32 multiply), so g = m / (1 - beta1) is the
    kernel's own gradient of the negative ELBO (mean / sd from the diagonal
    tiles, corr from the dL GEMM, KL included).  Checked in its two factors:
      * the update arithmetic: g against the oracle's update phase
        (mvn_grad_from_G) on the network's G, at 1e-5;
      * the network's per-sample G against the oracle's, at 1e-4, except
        samples on a ReLU kink (fp32 and fp64 may take the other mask there:
        margin < 1e-4 in their own rounding units, and rare) --
    and, when no sample sits on a kink, g against the whole oracle gradient at
    1e-4 (at this seed the first layer has kink samples: its end-to-end error
    is the mask flip's, 1e-3, for the chunked update as for the stream)."""
    from golden_util import assert_grad_close
    from psvi.runtime import InnerLoopPlan

    layers, S, M = [(64, 40), (40, 40), (40, 2)], 128, 100
    rng = np.random.default_rng(21)
    _, p0, _, _ = _case(layers, S, 21)
    u = rng.standard_normal((M, 64)).astype(np.float32)
    z = rng.integers(0, 2, M).astype(np.int32)
    w = O.coreset_weights(0.3 * rng.standard_normal(M), 800).astype(np.float32)
    plan = InnerLoopPlan("fullcov", layers, S, M)
    e0 = rng.standard_normal(plan.eps_count).astype(np.float32)
    e1 = rng.standard_normal(plan.eps_count).astype(np.float32)
    t = lambda a, d=torch.float32: torch.tensor(a, dtype=d, device=DEV)
    p = t(p0)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    x = torch.empty(plan.xshard_count, device=DEV)
    g = torch.zeros(plan.xrecv_count, device=DEV)
    nll = torch.zeros(1, dtype=torch.float64, device=DEV)
    kl = torch.zeros(1, dtype=torch.float64, device=DEV)
    plan.mvn_sample(t(e0), p, x)
    plan.mvn_net(t(u), t(z, torch.int32), t(w), x, g, nll)
    G = g.view(S, -1).cpu().numpy().astype(np.float64)
    ts = plan.tiled_state()
    plan.tiled_convert(p, m, v, ts, True)
    xn = torch.empty(plan.xshard_count, device=DEV)
    plan.mvn_update_tiled(t(e0), g, p, m, v, ts, step=1, lr=1e-3, kind=kind, kl_out=kl,
                          eps_next=t(e1), x_next=xn)
    plan.tiled_convert(p, m, v, ts, False)
    torch.cuda.synchronize()
    omb1 = np.float32(1.0) - np.float32(0.9)
    grad = m.cpu().numpy().astype(np.float64) / np.float64(omb1)
    # the update arithmetic on the same G
    assert_grad_close(grad, O.mvn_grad_from_G(layers, p0, G, e0, S), l2tol=1e-5,
                      what=f"stream-step gradient from G ({kind})")
    # the network's G per sample
    Ws, bs = O._split(layers, O._sample("mvn", layers, p0.astype(np.float64),
                                        e0.astype(np.float64), S))
    val, dWs, dbs = O.net_forward_backward(u.astype(np.float64), z, w.astype(np.float64), Ws, bs)
    Go = np.concatenate([np.concatenate([dW.reshape(S, -1), db], 1) for dW, db in zip(dWs, dbs)], 1)
    per = np.linalg.norm(G - Go, axis=1) / np.maximum(np.linalg.norm(Go, axis=1), 1e-30)
    bad = np.where(per > 1e-4)[0]
    marg = O.relu_margin(u.astype(np.float64), Ws, bs)
    good = np.setdiff1d(np.arange(S), bad)
    print(f"C3 stream step ({kind}): {len(bad)} kink samples {bad[:8]} margins {marg[bad][:8]}; "
          f"good samples' G l2rel {l2rel(G[good], Go[good]):.2e}")
    assert len(bad) <= 0.02 * S and np.all(marg[bad] < 1e-4), (bad, marg[bad])
    assert l2rel(G[good], Go[good]) < 1e-5
    lv, og = O.mvn_elbo_grad(layers, p0, u, z, w, e0, S)
    assert rel(nll.item() + kl.item(), lv) < 1e-5
    if len(bad) == 0:
        assert_grad_close(grad, og, what=f"stream-step gradient ({kind})")
