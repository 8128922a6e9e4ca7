#!/usr/bin/env python3
"""Golden vectors for PSVI.weight_reset and PSVI.increment_coreset (t1_*).

Runs ONLY on the development machine: like tools/gen_golden_giga.py the parent
re-launches this script in a child interpreter whose sys.path holds the
reference tree (PSVI_REFERENCE, or the first argument) and not this
repository.  On the CPU, in the reference's own float32, the child records

  * t1_reset_<arch>: the parameter vector after torch.manual_seed(k), the
    reference's set_up_model() and weight_reset() (psvi_classes.py:689-758,
    1110-1128) for logistic regression, 'fn' (D = 2, H = 8) and 'fn2' (D = 2,
    H = 4).  A model whose layers refuse the reset (the full-covariance ones:
    reset_parameters_variational raises) is recorded as the exception's name.
  * t1_increment: v, num_pseudo and the labels after increment_coreset
    (psvi_classes.py:1194-1217) from a given (u, z, v) with init_args =
    "random" under a fixed CPU seed, for the base class and for PSVIAV (whose
    override also rebuilds optim_alpha, 1501-1503).

Data only: nothing of the reference's code is written out.

Usage:  PSVI_REFERENCE=<reference tree> python tools/gen_golden_continual.py
"""
import json
import os
import subprocess
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def _child():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from gen_golden import _install_stubs

    _install_stubs()
    import numpy as np
    import torch
    from torch.nn.utils import parameters_to_vector
    from torch.utils.data import DataLoader, TensorDataset

    from psvi.inference import psvi_classes as PC

    def save(name, cfg, **arrs):
        np.savez_compressed(os.path.join(OUT, name + ".npz"), config=np.array(json.dumps(cfg)),
                            **arrs)
        print("wrote", name, {k: getattr(v, "shape", None) for k, v in arrs.items()})

    g = torch.Generator().manual_seed(77)
    x = torch.randn(40, 2, generator=g)
    y = torch.randint(0, 3, (40,), generator=g).float()
    ds = TensorDataset(x, y)

    def obj(cls, M, **kw):
        o = cls(train_dataset=ds, test_dataset=ds, N=40, D=2, num_pseudo=M, nc=3, mc_samples=4,
                seed=0, **kw)
        o.device = torch.device("cpu")
        return o

    # ---- weight_reset
    for arch, cfg in (("logreg", dict(logistic_regression=True, architecture=None, n_hidden=None)),
                      ("fn", dict(logistic_regression=False, architecture="fn", n_hidden=8)),
                      ("fn2", dict(logistic_regression=False, architecture="fn2", n_hidden=4))):
        cfg.update(D=2, nc=3, n_layers=1, init_sd=1e-3, mc_samples=4, seed=5)
        o = obj(PC.PSVI, 6)
        for k in ("logistic_regression", "architecture", "n_hidden", "n_layers", "init_sd"):
            setattr(o, k, cfg[k])
        torch.manual_seed(cfg["seed"])
        o.set_up_model()
        built = parameters_to_vector(o.model.parameters()).detach().numpy().copy()
        try:
            o.weight_reset()
            after = parameters_to_vector(o.model.parameters()).detach().numpy().copy()
            cfg["raises"] = None
        except Exception as e:     # noqa: BLE001 - the exception's type is the recorded result
            after = np.zeros(0, np.float32)
            cfg["raises"] = type(e).__name__
        save("t1_reset_" + arch, cfg, built=built, after=after)

    # ---- increment_coreset
    for name, cls in (("t1_increment", PC.PSVI), ("t1_increment_av", PC.PSVIAV)):
        M, to_size, new_class = 5, 9, 2
        o = obj(cls, M, increment=True, increment_sizes=[M, to_size])
        u0 = torch.randn(M, 2, generator=g)
        z0 = torch.tensor([0., 0., 1., 1., 1.])
        v0 = torch.rand(M, generator=g) + 0.1
        o.u, o.z, o.v = u0.clone().requires_grad_(True), z0.clone(), v0.clone().requires_grad_(True)
        o.init_args = "random"
        o.train_loader = DataLoader(ds, batch_size=16, shuffle=False)
        o.model = torch.nn.Linear(2, 3)
        torch.manual_seed(9)
        o.increment_coreset(to_size=to_size, lr0v=1e-2, lr0u=1e-3, lr0net=1e-3,
                            new_class=new_class, increment_idx=1)
        cfg = dict(M=M, to_size=to_size, new_class=new_class, seed=9, cls=cls.__name__,
                   num_pseudo=int(o.num_pseudo), u_requires_grad=bool(o.u.requires_grad),
                   v_requires_grad=bool(o.v.requires_grad))
        save(name, cfg, x=x.numpy(), y=y.numpy(), u0=u0.numpy(), z0=z0.numpy(), v0=v0.numpy(),
             v=o.v.detach().numpy(), z=o.z.detach().numpy(), u_shape=np.array(o.u.shape))


def main():
    if "--child" in sys.argv:
        _child()
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ref = args[0] if args else os.environ.get("PSVI_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set PSVI_REFERENCE (or pass the path) to the reference tree")
    os.makedirs(OUT, exist_ok=True)
    env = dict(os.environ)
    env["PYTHONPATH"] = ref
    env["PYTHONDONTWRITEBYTECODE"] = "1"
    subprocess.run([sys.executable, "-B", os.path.abspath(__file__), "--child"],
                   env=env, check=True, cwd="/tmp")


if __name__ == "__main__":
    main()
