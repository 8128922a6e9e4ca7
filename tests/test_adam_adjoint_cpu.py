"""The oracle's Adam adjoints (adam_higher_adjoint, adam_hypergrad_adjoint and
the adam_adjoint dispatcher in oracle/psvi_oracle.py) against torch.autograd
through a direct float64 restatement of the forward step (adam_util.step64).
The oracle's adjoints are hand derivations, the same ones as the HIP kernel's;
autograd shares no sign or factor with them.  The oracle's forward steps are
held to the same restatement, so that both sides differentiate one function."""
import numpy as np
import pytest
import torch

import psvi_oracle as O
from adam_util import F64, adjoint64_leaves, l2rel, step64

N = 509
STEPS = (1, 2, 10, 1000)
BETAS = ((0.9, 0.999), (0.5, 0.99))
KINDS = ("higher", "hypergrad")


def _case(kind, t, betas, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(N, generator=gen, dtype=F64)
    p, g = r(), r()
    fresh = t == 1
    m = torch.zeros(N, dtype=F64) if fresh else 0.3 * r()
    v = torch.zeros(N, dtype=F64) if fresh else 0.1 * r() ** 2
    return p, m, v, g, r(), r(), r()


@pytest.mark.parametrize("betas", BETAS)
@pytest.mark.parametrize("t", STEPS)
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_adjoint_matches_autograd(kind, t, betas):
    b1, b2 = betas
    lr, eps = 1e-3, 1e-8
    p, m, v, g, lt, lm, lv = _case(kind, t, betas, 100 * t + len(kind))
    (dp, dm, dv, dg), (m2, v2) = adjoint64_leaves(kind, p, m, v, g, lt, lm, lv, t, lr, b1, b2,
                                                  eps)
    po, mo, vo = O.adam(kind, p.numpy(), g.numpy(), m.numpy(), v.numpy(), t, lr, b1, b2, eps)
    p2 = step64(kind, p, m, v, g, t, lr, b1, b2, eps)[0]
    assert l2rel(torch.from_numpy(po - p.numpy()), p2 - p) < 1e-10
    assert l2rel(torch.from_numpy(mo), m2) < 1e-10 and l2rel(torch.from_numpy(vo), v2) < 1e-10
    lg_o, lm_o, lv_o = O.adam_adjoint(kind, lt.numpy(), lm.numpy(), lv.numpy(), m2.numpy(),
                                      v2.numpy(), g.numpy(), t, lr, b1, b2, eps)
    errs = {"lg": l2rel(torch.from_numpy(lg_o), dg), "lm": l2rel(torch.from_numpy(lm_o), dm),
            "lv": l2rel(torch.from_numpy(lv_o), dv)}
    print(f"{kind} t={t} betas={betas}: {errs}")
    assert max(errs.values()) < 1e-10, errs
    assert torch.equal(dp, lt)


@pytest.mark.parametrize("kind", KINDS)
def test_adjoint_dispatcher_selects_the_variant(kind):
    a = [np.full(3, x) for x in (0.7, 0.2, -0.4, 0.05, 0.01, 0.3)]
    fn = O.adam_higher_adjoint if kind == "higher" else O.adam_hypergrad_adjoint
    other = O.adam_hypergrad_adjoint if kind == "higher" else O.adam_higher_adjoint
    got = O.adam_adjoint(kind, *a, 3, 1e-3, beta1=0.5)
    for x, y, z in zip(got, fn(*a, 3, 1e-3, beta1=0.5), other(*a, 3, 1e-3, beta1=0.5)):
        assert np.array_equal(x, y) and not np.array_equal(x, z)
