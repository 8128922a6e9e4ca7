"""The fused conjugate-gradient iteration of hyper_step (psvi_cg_*,
psvi.runtime.cg.DeviceCG) against the reference's cg loop
(psvi/hypergrad/CG_torch.py:21-43) on CG_normaleq's operator
(hypergradients.py:217-230: A(p) = vmj - J vmj, vmj = lr H_A p, J y = y - lr
H_B y), with explicit fp32 matrices standing in for the two Hessian-vector
products: the same products, the same number of operator calls, x within
float64 summation order; the iterate before the residual test fired when it
fires; nothing non-finite reaches x after convergence."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops(n, seed, indefinite=False):
    g = torch.Generator().manual_seed(seed)
    Q = torch.randn(n, n, generator=g, dtype=torch.float64)
    HA = (Q @ Q.T / n + torch.eye(n, dtype=torch.float64))
    HB = HA + 0.01 * torch.randn(n, n, generator=g, dtype=torch.float64)
    if indefinite:
        HA = HA - 1.5 * torch.eye(n, dtype=torch.float64)
    return HA.float().to(DEV), HB.float().to(DEV)


def _reference(HA, HB, b, lr, K, tol):
    """CG_torch.cg on A(p) = vmj - (vmj - lr H_B float(vmj)), vmj = lr H_A float(p)
    (the fp32 products promoted as psvi_classes' torch formulation did)."""
    calls = [0]

    def mv(H, v):  # a matrix, or a diagonal operator given as its vector
        return H @ v if H.dim() == 2 else H * v

    def A(p):
        calls[0] += 1
        vmj = mv(HA, p.float()).double() * lr
        return vmj - torch.sub(vmj, mv(HB, vmj.float()).double(), alpha=lr)

    x, r, p = torch.zeros_like(b), b.clone(), b.clone()
    for _ in range(K):
        Ap = A(p)
        rTr = r @ r
        alpha = rTr / (p @ Ap)
        xn, rn = x + alpha * p, r - alpha * Ap
        if float(torch.norm(rn)) < tol:
            break
        p = rn + (rn @ rn) / rTr * p
        x, r = xn, rn
    return x, calls[0]


@pytest.mark.parametrize("n,K,tol,indef", [(3001, 12, 1e-10, False), (3001, 60, 1e-6, False),
                                           (777, 40, 1e-10, True)])
def test_device_cg_equals_reference_loop(n, K, tol, indef):
    from psvi.runtime.cg import DeviceCG

    HA, HB = _ops(n, n + K, indef)
    g = torch.Generator().manual_seed(1)
    b = torch.randn(n, generator=g, dtype=torch.float64).to(DEV)
    lr = 0.3
    xr, calls = _reference(HA, HB, b, lr, K, tol)
    ncall = [0]

    def hv_a(x32):
        ncall[0] += 1
        return HA @ x32

    def hv_b(x32):
        return HB @ x32

    cg = DeviceCG(n, DEV)
    x = cg.solve(hv_a, hv_b, b, lr, K, tol=tol, sync_every=1)
    torch.cuda.synchronize()
    assert ncall[0] == calls, (ncall[0], calls)   # the reference's exit: same operator calls
    assert torch.isfinite(x).all() == torch.isfinite(xr).all()
    if torch.isfinite(xr).all():
        err = float((x - xr).norm() / xr.norm())
        print(f"n {n} K {K} tol {tol}: {calls} operator calls, rel l2 {err:.2e}")
        # (an indefinite operator amplifies the dots' summation order over 40
        # iterations: the iterates agree to that conditioning only)
        assert err < (1e-4 if indef else 1e-9)
    # a host read every 4 iterations: the same x (frozen), up to 3 more calls
    ncall[0] = 0
    x4 = cg.solve(hv_a, hv_b, b, lr, K, tol=tol, sync_every=4)
    torch.cuda.synchronize()
    assert torch.allclose(x4, x, rtol=0, atol=0, equal_nan=True)
    assert calls <= ncall[0] < calls + 4 or ncall[0] == K


def test_device_cg_is_deterministic():
    from psvi.runtime.cg import DeviceCG

    n = 20001
    HA, HB = _ops(1000, 3)
    HA = torch.block_diag(*([HA] * 20 + [torch.ones(1, 1, device=DEV)]))
    HB = HA
    b = torch.randn(n, dtype=torch.float64, device=DEV)
    cg = DeviceCG(n, DEV)
    a = cg.solve(lambda v: HA @ v, lambda v: HB @ v, b, 0.5, 8)
    c = cg.solve(lambda v: HA @ v, lambda v: HB @ v, b, 0.5, 8)
    torch.cuda.synchronize()
    assert torch.equal(a, c)


# --------------------------------------------------------------------------
# The four passes one at a time, past the first trip of every loop in them:
# grid_sum's last workgroup reads slot columns i = 0..3 (column 1 from 257
# workgroups on: n > 65,536), the launch is capped at kCgBlocks = 1024
# workgroups of kCgThreads = 256 (the stride loop's second pass: n > 262,144).
U53 = 2.0 ** -53
CG_BLOCKS, CG_THREADS = 1024, 256
CG_NS = [65_537,        # 257 workgroups: the first use of slot column 1
         262_157,       # the cap, and a second pass of 13
         786_437]       # three passes, and 5
LR = 0.3
# Roundings from one element to the total of a grid sum, behind the
# elementwise ones: the per-thread run (at most 4 trips at these n, one add
# each), the wave butterfly (6), the waves of a workgroup (4), the four slot
# columns (2), the last workgroup's butterfly and waves (6 + 4).
K_SUM = 4 + 6 + 4 + 2 + 10
# cg_pap, elementwise: lr hv1, lr hv2, the two subtractions of cg_ap, p Ap.
K_PAP = 5 + K_SUM          # 31
# cg_residual, elementwise: rTr / pAp, then cg_ap's four, alpha Ap, r - that.
K_R = 7
# ... and for rnrn: the square, then the sum.
K_RNRN = 1 + K_SUM         # 27


def _ld(a):
    """x87 extended precision (64-bit significand): a product of an fp32 and
    an fp64, or of two fp64, rounds at 2^-64 -- 2^-11 of one fp64 rounding."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    return np.asarray(a, dtype=np.longdouble)


def _fsum(v):
    """The exactly rounded sum of a float64 or extended vector (math.fsum; an
    extended value is passed as its float64 head and tail)."""
    if v.dtype == np.longdouble:
        hi = v.astype(np.float64)
        return math.fsum(hi.tolist() + (v - hi).astype(np.float64).tolist())
    return math.fsum(v.tolist())


@functools.lru_cache(maxsize=None)
def _vectors(n):
    """Host inputs of one size and everything the references share (computed
    once per size, never written)."""
    rng = np.random.default_rng(n)
    p = rng.standard_normal(n)
    d = dict(hv1=rng.standard_normal(n).astype(np.float32),
             hv2=(p * (1 + 0.25 * rng.standard_normal(n))).astype(np.float32),   # pAp > 0
             p=p, r=rng.standard_normal(n), x=rng.standard_normal(n))
    d["t"] = _ld(LR) * _ld(d["hv2"])                      # Ap = vmj - (vmj - lr hv2) = lr hv2
    vmj = LR * d["hv1"].astype(np.float64)
    d["W"] = 2 * np.abs(vmj) + np.abs(d["t"].astype(np.float64))   # cg_ap's operand scale
    d["pap"] = _fsum(_ld(d["p"]) * d["t"])
    d["rtr"] = _fsum(_ld(d["r"]) * _ld(d["r"]))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _cg_lib():
    from psvi.runtime import _lib

    return _lib.load()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.tensor(a, device=DEV)


def _ws(lib):
    return torch.zeros(int(lib.psvi_cg_ws_bytes()), dtype=torch.uint8, device=DEV)


def _counter(ws):
    """The arrival counter behind the kCgBlocks partial slots."""
    return int(ws[8 * CG_BLOCKS:8 * CG_BLOCKS + 4].view(torch.int32).item())


@pytest.mark.parametrize("n", CG_NS)
def test_cg_scale_is_exact(n):
    v, lib = _vectors(n), _cg_lib()
    out = torch.full((n + 1,), -7.0, device=DEV)
    assert lib.psvi_cg_scale(n, _ptr(_dev(v["hv1"])), LR, _ptr(out), _stream()) == 0
    torch.cuda.synchronize()
    want = (LR * v["hv1"].astype(np.float64)).astype(np.float32)
    got = out.cpu().numpy()
    assert np.array_equal(got[:n].view(np.int32), want.view(np.int32)) and got[n] == -7.0


@pytest.mark.parametrize("n", CG_NS)
def test_cg_pap_against_fsum(n):
    """state[kPap] against fsum(p_i Ap_i) within K_PAP 2^-53 sum |p_i| (2 |vmj_i|
    + |lr hv2_i|): K_PAP = 31 roundings lie between an element and the total
    (counted above from kernels_cg.hip); cg_ap cancels at vmj's scale, and the
    compiler contracts lr hv1 into its subtractions, hence the |vmj| terms."""
    v, lib = _vectors(n), _cg_lib()
    state = torch.zeros(7, dtype=torch.float64, device=DEV)
    ws = _ws(lib)
    hv1, hv2, p = _dev(v["hv1"]), _dev(v["hv2"]), _dev(v["p"])
    got = []
    for _ in range(2):
        state.fill_(-1.0)
        assert lib.psvi_cg_pap(n, _ptr(hv1), _ptr(hv2), LR, _ptr(p), _ptr(state), _ptr(ws),
                               ws.numel(), _stream()) == 0
        torch.cuda.synchronize()
        assert _counter(ws) == 0
        got.append(state.cpu().numpy().copy())
    assert np.array_equal(got[0], got[1])                 # whichever workgroup arrives last
    assert (np.delete(got[0], 1) == -1.0).all()           # kPap alone is written
    bound = K_PAP * U53 * _fsum(np.abs(v["p"]) * v["W"])
    err = abs(got[0][1] - v["pap"])
    print(f"cg_pap n {n}: pAp {got[0][1]:.17g} ref {v['pap']:.17g} err {err:.3e} bound {bound:.3e}")
    assert err <= bound


def _residual_ref(v):
    alpha = _ld(v["rtr"]) / _ld(v["pap"])
    rn = _ld(v["r"]) - alpha * v["t"]
    a = abs(float(alpha))
    e = K_R * U53 * (np.abs(v["r"]) + a * v["W"])          # the elementwise bound
    rn64 = np.abs(rn.astype(np.float64))
    rnrn = _fsum(rn * rn)
    rnrn_bound = _fsum(2 * rn64 * e + e * e) + K_RNRN * U53 * _fsum((rn64 + e) ** 2)
    return rn, e, rnrn, rnrn_bound


@pytest.mark.parametrize("n", CG_NS)
def test_cg_residual_against_fsum_and_both_branches(n):
    """r elementwise within K_R = 7 roundings of |r_i| + |alpha| (2 |vmj_i| +
    |lr hv2_i|), rnrn within that carried through the squares plus K_RNRN = 27
    roundings of the sum; then every scalar of the last workgroup's branch,
    the tolerance a millionth to either side of sqrt(rnrn)."""
    v, lib = _vectors(n), _cg_lib()
    rn, e, rnrn, rnrn_bound = _residual_ref(v)
    hv1, hv2 = _dev(v["hv1"]), _dev(v["hv2"])
    ws = _ws(lib)
    rtr, pap = v["rtr"], v["pap"]
    alpha = rtr / pap

    def run(tol, done0):
        r = _dev(v["r"])
        state = torch.tensor([rtr, pap, -1.0, done0, -1.0, -1.0, -1.0], dtype=torch.float64,
                             device=DEV)
        assert lib.psvi_cg_residual(n, _ptr(hv1), _ptr(hv2), LR, _ptr(r), _ptr(state), float(tol),
                                    _ptr(ws), ws.numel(), _stream()) == 0
        torch.cuda.synchronize()
        assert _counter(ws) == 0
        return r.cpu().numpy(), state.cpu().numpy()

    lo, hi = math.sqrt(rnrn) * (1 - 1e-6), math.sqrt(rnrn) * (1 + 1e-6)
    r_a, s_a = run(lo, 0.0)                               # not done
    err = np.abs(_ld(r_a) - rn).astype(np.float64)
    print(f"cg_residual n {n}: max r err / bound {float((err / e).max()):.3f}, rnrn err "
          f"{abs(s_a[2] - rnrn):.3e} bound {rnrn_bound:.3e}")
    assert (err <= e).all()
    assert abs(s_a[2] - rnrn) <= rnrn_bound
    assert abs(s_a[6] - alpha) <= 2 * U53 * abs(alpha)    # alpha: one division
    assert s_a[4] == s_a[6]                               # aeff = alpha
    assert abs(s_a[5] - s_a[2] / rtr) <= 2 * U53 * abs(s_a[5])   # beta = rnrn / rTr
    assert s_a[0] == s_a[2] and s_a[3] == 0.0 and s_a[1] == pap  # rTr <- rnrn, not done
    r_b, s_b = run(hi, 0.0)                               # done
    assert np.array_equal(r_b, r_a) and s_b[2] == s_a[2]
    assert s_b[4] == 0.0 and s_b[0] == rtr and s_b[3] == 1.0 and s_b[6] == s_a[6]
    r_c, s_c = run(lo, 1.0)                               # done before: stays done
    assert np.array_equal(r_c, r_a)
    assert s_c[4] == 0.0 and s_c[0] == rtr and s_c[3] == 1.0


@pytest.mark.parametrize("n", CG_NS)
def test_cg_update_both_branches(n):
    """Not done: x + aeff p and r + beta p each within one fused multiply-add's
    rounding, 2^-53 of the result (plus the extended reference's own 2^-62 of
    the operands); p32 within one fp32 ulp of the reference's p rounded.
    Done: x, p and p32 keep their bits."""
    v, lib = _vectors(n), _cg_lib()
    aeff, beta = 0.37, 0.81
    r = _dev(v["r"])

    def run(done):
        x, p = _dev(v["x"]), _dev(v["p"])
        p32 = torch.full((n,), -7.0, device=DEV)
        state = torch.tensor([0, 0, 0, done, 0.0 if done else aeff, beta, aeff],
                             dtype=torch.float64, device=DEV)
        assert lib.psvi_cg_update(n, _ptr(x), _ptr(p), _ptr(p32), _ptr(r), _ptr(state),
                                  _stream()) == 0
        torch.cuda.synchronize()
        return x.cpu().numpy(), p.cpu().numpy(), p32.cpu().numpy()

    x1, p1, q1 = run(0.0)
    xr = _ld(v["x"]) + _ld(aeff) * _ld(v["p"])
    pr = _ld(v["r"]) + _ld(beta) * _ld(v["p"])
    ex = np.abs(x1 - xr).astype(np.float64)
    ep = np.abs(p1 - pr).astype(np.float64)
    bx = U53 * np.abs(xr.astype(np.float64)) + 2.0 ** -62 * (np.abs(v["x"]) + aeff * np.abs(v["p"]))
    bp = U53 * np.abs(pr.astype(np.float64)) + 2.0 ** -62 * (np.abs(v["r"]) + beta * np.abs(v["p"]))
    print(f"cg_update n {n}: max x err / bound {float((ex / bx).max()):.3f}, p "
          f"{float((ep / bp).max()):.3f}")
    assert (ex <= bx).all() and (ep <= bp).all()
    want32 = pr.astype(np.float64).astype(np.float32)
    assert (np.abs(q1 - want32) <= np.spacing(np.abs(want32))).all()
    x2, p2, q2 = run(1.0)
    assert np.array_equal(x2.view(np.int64), v["x"].view(np.int64))
    assert np.array_equal(p2.view(np.int64), v["p"].view(np.int64))
    assert (q2 == -7.0).all()


def test_device_cg_past_the_grid_cap():
    """A whole solve at 1024 workgroups and a second pass of 13 elements, with
    diagonal operators: the file's reference loop, its bound, its operator
    count; and two solves with the same bits, the last arriver varying."""
    from psvi.runtime.cg import DeviceCG

    n, lr, K, tol = 262_157, 0.3, 20, 1e-3
    g = torch.Generator().manual_seed(5)
    dA = (1 + torch.rand(n, generator=g)).to(DEV)
    dB = (1 + torch.rand(n, generator=g)).to(DEV)
    b = torch.randn(n, generator=g, dtype=torch.float64).to(DEV)
    xr, calls = _reference(dA, dB, b, lr, K, tol)
    assert 2 < calls < K, calls                            # the residual test fires
    ncall = [0]

    def hv_a(v32):
        ncall[0] += 1
        return dA * v32

    cg = DeviceCG(n, DEV)
    x = cg.solve(hv_a, lambda v32: dB * v32, b, lr, K, tol=tol)
    torch.cuda.synchronize()
    assert ncall[0] == calls, (ncall[0], calls)
    err = float((x - xr).norm() / xr.norm())
    print(f"n {n}: {calls} operator calls, rel l2 {err:.2e}")
    assert err < 1e-9
    x2 = cg.solve(hv_a, lambda v32: dB * v32, b, lr, K, tol=tol)
    torch.cuda.synchronize()
    assert torch.equal(x, x2)
