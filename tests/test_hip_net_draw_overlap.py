"""The network launch's fused next-step draw, drawn partly by the waves that
carry no row tile while the others run the row chain and for the rest by every
wave behind the weight gradients, in whole-wave chunks handed out at run time.
Who draws which quad must not matter: every case runs one launch with the
draw through the entry the loop uses and asserts, bitwise,

  * the fp32 buffer == psvi_randn(seed, offset) (Philox4x32-10 + Box-Muller;
    the reference's torch.randn_like draw, models/neural_net.py:485-491, is
    replaced by this stream throughout the library);
  * full-cov: the three bf16 planes == the separate planes draw's (the
    stand-alone kernel, reached through a launch without samples), which in
    turn == the round-to-nearest-even split of the fp32 values computed here;
    pad columns keep the sentinel they were filled with;
  * the gradients and the NLL == those of the same launch without a draw.

The planes of a phase launch come out through PSVI_DBG_NET_DRAW_PLANES (the
loop passes its own buffer; the kernel path is the same).  Plans are created
with PSVI_DBG_NET_WG_TARGET = 1, so that a plan of a few samples keeps the
whole pseudopoint chunk of the large configurations (two role workgroups per
sample, no pseudopoint chunks beyond what the LDS forces)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FN2 = [(64, 40), (40, 40), (40, 2)]
WG_TARGET, DRAW_PLANES = 15, 35  # PSVI_DBG_NET_WG_TARGET, PSVI_DBG_NET_DRAW_PLANES
SENT = 0x5A5A


def _plan(fam, layers, S, M):
    from psvi.runtime import InnerLoopPlan
    from psvi.runtime import _lib

    lib = _lib.load()
    assert lib.psvi_debug_set(WG_TARGET, 1) == 0
    try:
        return InnerLoopPlan(fam, layers, S, M)
    finally:
        lib.psvi_debug_set(WG_TARGET, 256)


def _data(plan, layers, M, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(M, layers[0][0], generator=g).to(DEV)
    z = torch.randint(0, layers[-1][1], (M,), generator=g).to(torch.int32).to(DEV)
    w = (torch.rand(M, generator=g) * 10 + 1).to(DEV)
    return u, z, w, g


def _layout(layers, S):
    """EpsPlanes of a full-cov draw: per layer (eoff, n, npad, poff), plane length."""
    lay, eo, po = [], 0, 0
    for din, dout in layers:
        n = din * dout + dout
        npad = (n + 63) // 64 * 64
        lay.append((eo, n, npad, po))
        eo += S * n
        po += S * npad
    return lay, (po + 63) // 64 * 64


def _expected_planes(e, layers, S):
    """The three bf16 pieces (round to nearest even, exact residuals) of the fp32
    draw e in the plane layout, pads = SENT."""
    lay, pl = _layout(layers, S)
    out = torch.full((3, pl), SENT, dtype=torch.int16, device=e.device)
    for eo, n, npad, po in lay:
        x = e[eo:eo + S * n].view(S, n)
        r = x
        for p in range(3):
            b = r.to(torch.bfloat16)
            out[p, po:po + S * npad].view(S, npad)[:, :n] = b.view(torch.int16)
            r = r - b.float()
    return out


def _net(plan, u, z, w, xs, draw=None, samples=None, part=(0, 1), planes=None, e=None):
    """One network launch; draw = (seed, offset).  Returns g_send, nll, eps, planes."""
    gs = torch.full((plan.xrecv_count,), float("nan"), device=DEV)
    nll = torch.zeros(1, dtype=torch.float64, device=DEV)
    if draw is None:
        plan.mvn_net(u, z, w, xs, gs, nll, samples=samples)
        torch.cuda.synchronize()
        return gs, nll, None, None
    if e is None:
        e = torch.full((plan.eps_count,), float("nan"), device=DEV)
    assert plan.lib.psvi_debug_set_ptr(DRAW_PLANES, ctypes.c_void_p(planes.data_ptr())) == 0
    try:
        if samples is None:
            plan.mvn_net(u, z, w, xs, gs, nll, draw=(e,) + tuple(draw))
        else:
            plan.mvn_net(u, z, w, xs, gs, nll, draw=(e,) + tuple(draw), samples=samples, draw_part=part)
        torch.cuda.synchronize()
    finally:
        plan.lib.psvi_debug_set_ptr(DRAW_PLANES, None)
    return gs, nll, e, planes


def _sentinel_planes(layers, S):
    return torch.full((3 * _layout(layers, S)[1],), SENT, dtype=torch.int16, device=DEV)


def _check_fullcov(layers, S, M, seed, offset):
    from psvi.runtime import randn_

    plan = _plan("fullcov", layers, S, M)
    u, z, w, g = _data(plan, layers, M, S + M)
    xs = (0.2 * torch.randn(plan.xrecv_count, generator=g)).to(DEV)
    n = plan.eps_count
    ref = randn_(torch.empty(n, device=DEV), seed, offset)
    # the separate planes draw: a launch without samples draws on the stand-alone kernel
    _, _, e_sep, p_sep = _net(plan, u, z, w, xs, (seed, offset), samples=(0, 0),
                              planes=_sentinel_planes(layers, S))
    assert torch.equal(e_sep, ref)
    pl = _layout(layers, S)[1]
    assert torch.equal(p_sep.view(3, pl), _expected_planes(ref, layers, S))
    g0, nll0, _, _ = _net(plan, u, z, w, xs)
    g1, nll1, e1, p1 = _net(plan, u, z, w, xs, (seed, offset), planes=_sentinel_planes(layers, S))
    assert torch.isfinite(g0).all()
    assert torch.equal(e1, ref)
    assert torch.equal(p1, p_sep)
    assert torch.equal(g1, g0) and torch.equal(nll1, nll0)
    return plan


@pytest.mark.parametrize("layers,S,M", [
    (FN2, 2, 100),               # a: fixed geometry, one spare wave, both roles
    (FN2, 2, 200),               # b: looped pseudopoint chunks, the draw once
    (FN2, 2, 128),               # c: 8 tiles on 8 waves, no spare wave, run-time geometry
    ([(5, 3), (3, 2)], 3, 20),   # d: 256 threads, two spare waves, fewer chunks than workgroups, n % 4 != 0
], ids=["fn2_m100", "fn2_m200_mloop", "fn2_m128_nospare", "small_ragged"])
def test_fullcov_draw_any_wave(layers, S, M):
    plan = _check_fullcov(layers, S, M, seed=31, offset=0)
    if layers is FN2 and M == 200:
        assert plan.eps_count % 4 == 0
    if len(layers) == 2:
        assert plan.eps_count % 4 != 0


def test_fullcov_draw_offset_and_wide_seed():
    """An offset that is a non-zero multiple of the eps stride and a seed with a
    non-zero high word (the Philox key's second half)."""
    S, M = 2, 100
    n = S * sum(a * b + b for a, b in FN2)
    stride = (n + 3) // 4 * 4
    _check_fullcov(FN2, S, M, seed=(0x9E3779B9 << 32) | 12345, offset=3 * stride)


def test_meanfield_loop_draw():
    """e: mean-field 2-100-4, M = 50, S = 4 (no planes, four spare waves).  The
    mean-field network launch draws only inside the inner loop: two Philox
    steps leave the second step's draw in the loop workspace, == psvi_randn;
    parameters, Adam state and ELBOs == the loop on those draws passed in
    (network launches without a draw)."""
    from psvi.runtime import randn_

    layers, S, M = [(2, 100), (100, 4)], 4, 50
    plan = _plan("meanfield", layers, S, M)
    u, z, w, g = _data(plan, layers, M, 11)
    p0 = (0.1 * torch.randn(plan.param_count, generator=g)).to(DEV)
    n, es, seed, off = plan.eps_count, plan.eps_stride, 77, 8 * plan.eps_stride
    eps = torch.stack([randn_(torch.empty(n, device=DEV), seed, off + t * es) for t in range(2)])
    outs = []
    for fused in (False, True):
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        ws = torch.zeros(plan.loop_ws_bytes, dtype=torch.uint8, device=DEV)
        elbo = plan.inner_loop(u, z, w, p, m, v, 2, 1e-2, ws=ws, seed=seed, offset=off,
                               eps=None if fused else eps.view(-1))
        torch.cuda.synchronize()
        outs.append((p, m, v, elbo.clone(), ws))
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert torch.equal(a, b)
    a256 = lambda x: (x + 255) // 256 * 256
    at = a256(plan.ws_bytes) + a256(4 * (es + 64))  # the loop's second eps buffer
    drawn = outs[1][4][at:at + 4 * n].view(torch.float32)
    assert torch.equal(drawn, eps[1])


def test_part_draw_of_an_empty_half():
    """f: a rank with one local sample in the two-half schedule: half 0 has no
    sample and part 0 of the draw, half 1 the sample and part 1 -- and the
    other way round.  The launch without samples must draw exactly its part
    (before the fix it drew nothing unless it held part 0, and then the whole
    draw).  The union of the two launches is the whole draw, planes included."""
    from psvi.runtime import randn_

    S, M, seed, off = 1, 100, 5, 0
    plan = _plan("fullcov", FN2, S, M)
    u, z, w, g = _data(plan, FN2, M, 3)
    xs = (0.2 * torch.randn(plan.xrecv_count, generator=g)).to(DEV)
    n = plan.eps_count
    ref = randn_(torch.empty(n, device=DEV), seed, off)
    pref = _expected_planes(ref, FN2, S).view(-1)
    nq = (n + 3) // 4
    g0, nll0, _, _ = _net(plan, u, z, w, xs)
    for empty_part in (0, 1):
        e = torch.full((n,), float("nan"), device=DEV)
        pb = _sentinel_planes(FN2, S)
        _net(plan, u, z, w, xs, (seed, off), samples=(0, 0), part=(empty_part, 2), planes=pb, e=e)
        # exactly this part's quads so far
        lo, hi = 4 * (nq * empty_part // 2), min(n, 4 * (nq * (empty_part + 1) // 2))
        assert torch.equal(e[lo:hi], ref[lo:hi])
        assert torch.isnan(e[:lo]).all() and torch.isnan(e[hi:]).all()
        g1, nll1, _, _ = _net(plan, u, z, w, xs, (seed, off), samples=(0, 1),
                              part=(1 - empty_part, 2), planes=pb, e=e)
        assert torch.equal(e, ref)
        assert torch.equal(pb, pref)
        assert torch.equal(g1, g0) and torch.equal(nll1, nll0)
