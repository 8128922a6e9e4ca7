"""Float64 references for one generic Adam step and its adjoint, shared by
tests/test_adam_adjoint_cpu.py and tests/test_hip_adam_elementwise.py.

step64 restates the three forward variants of adam_apply
(csrc/psvi_internal.hpp) in torch.float64, from Python doubles, so that
torch.autograd differentiates them; adjoint64 contracts (p', m', v') with the
incoming adjoints and returns what psvi_adam_adjoint computes.  Nothing here
is a hand derivation."""
import torch

F64 = torch.float64


def step64(kind, p, m, v, g, t, lr, b1, b2, eps):
    """One Adam step (t 1-based) on float64 tensors: (p', m', v')."""
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    m2 = b1 * m + (1.0 - b1) * g
    if kind == "higher":
        v2 = b2 * v + (1.0 - b2) * g * g
        p2 = p - (lr / bc1) * m2 / (torch.sqrt(v2 + 1e-8) / bc2 ** 0.5 + eps)
    elif kind == "torch":
        v2 = b2 * v + (1.0 - b2) * g * g
        p2 = p - (lr / bc1) * m2 / (torch.sqrt(v2) / bc2 ** 0.5 + eps)
    elif kind == "hypergrad":
        v2 = b2 * v + (1.0 - b2) * g * g + 1e-12
        p2 = p - lr * (m2 / bc1) / (torch.sqrt(v2 / bc2) + eps)
    else:
        raise ValueError(kind)
    return p2, m2, v2


def adjoint64_leaves(kind, p, m, v, g, lt, lm, lv, t, lr, b1, b2, eps):
    """Autograd through step64 from the leaves (p, m, v, g), contracted with
    (lt, lm, lv): returns (dp, dm, dv, dg) and the step's detached (m', v')."""
    p, m, v, g = (x.detach().to(F64).clone().requires_grad_(True) for x in (p, m, v, g))
    p2, m2, v2 = step64(kind, p, m, v, g, t, lr, b1, b2, eps)
    s = (p2 * lt).sum() + (m2 * lm).sum() + (v2 * lv).sum()
    dp, dm, dv, dg = torch.autograd.grad(s, (p, m, v, g))
    return (dp, dm, dv, dg), (m2.detach(), v2.detach())


def adjoint64(kind, lt, lm, lv, m2, v2, g, t, lr, b1, b2, eps):
    """psvi_adam_adjoint's contract by autograd at the given stored (m', v')
    and g: the incoming state is solved from them (the adjoint does not depend
    on it otherwise), so step64 reproduces m', v' to float64 rounding.
    Returns (lg, adjoint of m, adjoint of v)."""
    lt, lm, lv, m2, v2, g = (x.to(F64) for x in (lt, lm, lv, m2, v2, g))
    m = (m2 - (1.0 - b1) * g) / b1
    v = (v2 - (1.0 - b2) * g * g - (1e-12 if kind == "hypergrad" else 0.0)) / b2
    (_, dm, dv, dg), _ = adjoint64_leaves(kind, torch.zeros_like(g), m, v, g, lt, lm, lv, t, lr,
                                          b1, b2, eps)
    return dg, dm, dv


def l2rel(a, b):
    """|a - b| / |b| on float64 tensors; 0 for two zero arrays."""
    a, b = a.to(F64), b.to(F64)
    d, n = float(torch.linalg.norm(a - b)), float(torch.linalg.norm(b))
    return d / n if n > 0 else d
