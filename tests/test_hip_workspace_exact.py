"""Every workspace-taking entry point stays inside the size its query reports.

Each case hands the entry point a buffer of queried_bytes + 4096 bytes filled
with 0xA5 and passes ws_bytes = queried_bytes: after one run the trailing 4096
bytes must be untouched, and the same call with ws_bytes = queried_bytes - 1
must return PSVI_ENOSPC.  (The buffer is larger than anything the code may
touch, so an overrun shows in the guard band instead of faulting.)

Shapes: full-cov 12-20-4, S = 128, M = 8 (tiled state, bf16-plane stream,
stream table); full-cov 3-5-2, S = 4, M = 3 (packed path); mean-field 2-5-2,
S = 4, M = 3; Gaussian 5-8-1, S = 4, M = 3 (the dz / dzd regions and
psvi_evaluate_regression)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, FILL = 4096, 0xA5
ENOSPC = -2

SHAPES = {
    "fullcov-tiled": ("fullcov", [12, 20, 4], 128, 8, None),
    "fullcov-packed": ("fullcov", [3, 5, 2], 4, 3, None),
    "meanfield": ("meanfield", [2, 5, 2], 4, 3, None),
    "gaussian": ("meanfield", [5, 8, 1], 4, 3, ("gaussian", 2.0)),
}


class _Spy:
    """Forwards to the library and keeps the last call's function and arguments."""

    def __init__(self, lib):
        self._lib, self.last = lib, None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.last = (fn, args)
            return fn(*args)

        return call


@functools.lru_cache(maxsize=None)
def _case(shape):
    from psvi.runtime import InnerLoopPlan

    family, dims, S, M, lik = SHAPES[shape]
    plan = InnerLoopPlan(family, list(zip(dims[:-1], dims[1:])), S, M, likelihood=lik)
    plan.lib = _Spy(plan.lib)
    g = torch.Generator(device="cpu").manual_seed(20261021)
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV)
    if lik:
        z = rn(M)
    else:
        z = torch.randint(0, dims[-1], (M,), generator=g, dtype=torch.int32).to(DEV)
    return dict(plan=plan, u=rn(M, dims[0]), z=z, w=rn(M).abs() + 0.5, eps=rn(plan.eps_count),
                params=0.1 * rn(plan.param_count), vec=rn(plan.param_count))


def _inner_step(c, ws):
    p = c["params"].clone()
    c["plan"].inner_step(c["u"], c["z"], c["w"], c["eps"], p, torch.zeros_like(p),
                         torch.zeros_like(p), step=1, lr=1e-3, ws=ws)


def _inner_loop(c, ws):
    p = c["params"].clone()
    c["plan"].inner_loop(c["u"], c["z"], c["w"], p, torch.zeros_like(p), torch.zeros_like(p), 3,
                         1e-3, seed=7, offset=8, ws=ws)


def _outer(c, ws):
    plan = c["plan"]
    plan.outer_elbo_grad(plan.M - 1, c["u"], c["z"], c["w"], c["eps"], c["params"],
                         sample_stats=True, ws=ws, grad_z=plan.likelihood == "gaussian")


def _evaluate(c, ws):
    plan = c["plan"]
    if plan.likelihood == "gaussian":
        plan.evaluate_regression(1, c["u"], c["z"], c["w"], c["eps"], c["params"], pred=True, ws=ws)
    else:
        plan.evaluate(1, c["u"], c["z"], c["w"], c["eps"], c["params"], probs=True, ws=ws)


def _hvp(c, ws):
    c["plan"].hvp(c["u"], c["z"], c["w"], c["eps"], c["params"], c["vec"], ws=ws)


ENTRY = {
    "inner_step": (_inner_step, "ws_bytes"),
    "inner_loop": (_inner_loop, "loop_ws_bytes"),
    "outer_elbo_grad": (_outer, "outer_ws_bytes"),
    "evaluate": (_evaluate, "eval_ws_bytes"),
    "hvp": (_hvp, "hvp_ws_bytes"),
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("entry", list(ENTRY))
def test_exact_workspace(entry, shape):
    c = _case(shape)
    plan = c["plan"]
    run, query = ENTRY[entry]
    q = getattr(plan, query)
    buf = torch.full((q + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    run(c, buf[:q])
    torch.cuda.synchronize()
    touched = int((buf[q:] != FILL).sum().item())
    assert touched == 0, f"{touched} bytes written past the {q} bytes {query} reports"
    # the library saw exactly this workspace: the pointer, then ws_bytes = q
    fn, args = plan.lib.last
    at = [i for i, a in enumerate(args)
          if isinstance(a, ctypes.c_void_p) and a.value == buf.data_ptr()]
    assert len(at) == 1 and args[at[0] + 1] == q, (fn.__name__, at)
    short = list(args)
    short[at[0] + 1] = q - 1
    assert fn(*short) == ENOSPC
    torch.cuda.synchronize()
