#!/usr/bin/env python3
"""Golden vectors for the MFVI regression baselines (psvi_mfvi_fit).

Runs ONLY in the development container (the reference is mounted read-only at
/root/reference); like tools/gen_golden_regressor.py the parent re-launches
this script in a child interpreter whose sys.path holds the reference and not
this repo.  In float64 on the CPU, with every Monte-Carlo draw rounded to fp32
and recorded in call order, the child runs the reference's own

  fit   psvi/inference/baselines.py:1283-1346 on make_regressor_net
        (neural_net.py:300-331) with torch.optim.Adam, log_every = -1

for tiny shapes and writes numeric-only fixtures tests/golden/m*.npz: the
inputs (normalised training rows, test rows with targets in original units,
y_mean / y_std, the starting parameters), eps of the T training steps in draw
order ([T][EPS_COUNT]: the library's layout) and of the closing evaluation
(one draw per test batch), the per-step losses (-elbos), the final parameters
and the logged rmse / ll.

Usage:  python tools/gen_golden_mfvi_regr.py
"""
import json
import os
import subprocess
import sys

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def _child():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from gen_golden import _install_stubs

    _install_stubs()
    import numpy as np
    import torch
    import torch.distributions.normal as normal_mod
    from torch.nn.utils import parameters_to_vector
    from torch.utils.data import DataLoader, TensorDataset

    from psvi.inference.baselines import fit
    from psvi.models.neural_net import make_regressor_net

    torch.set_default_dtype(torch.float64)
    draws = []
    orig = normal_mod._standard_normal

    def standard_normal(shape, dtype, device):
        out = orig(shape, dtype=dtype, device=device).float().to(dtype)
        draws.append(out.detach().clone().reshape(-1))
        return out

    normal_mod._standard_normal = standard_normal

    def case(name, D, H, L, n_train, B, n_test, test_batch, S, T, tau, lr, seed):
        gen = torch.Generator().manual_seed(seed)

        def rnd(*shape):
            return torch.randn(*shape, generator=gen).float().double()

        x, y = rnd(n_train, D), rnd(n_train, 1)
        y_mean, y_std = 1.7, 2.3
        xt = rnd(n_test, D)
        yt = (rnd(n_test, 1) * y_std + y_mean).float().double()
        net = make_regressor_net(D, H, 1, n_layers=L, mc_samples=S, init_sd=0.05)
        with torch.no_grad():
            for pname, p in net.named_parameters():
                if pname.split(".")[-1] in ("weight", "bias"):
                    p.copy_(0.4 * torch.randn(p.shape, generator=gen))
                else:
                    p.copy_(-3.0 + 2.0 * torch.rand(p.shape, generator=gen))
                p.copy_(p.float().double())
        params0 = parameters_to_vector(net.parameters()).detach().numpy().copy()
        del draws[:]
        res = fit(net=net, optim_vi=torch.optim.Adam(net.parameters(), lr),
                  train_loader=DataLoader(TensorDataset(x, y), batch_size=B, shuffle=False),
                  pred_loader=DataLoader(TensorDataset(xt, yt), batch_size=test_batch,
                                         shuffle=False),
                  revert_norm=lambda yp: yp * y_std + y_mean, log_every=-1, tau=tau, epochs=T,
                  device=torch.device("cpu"))
        layers = [(D if i == 0 else H, H) for i in range(L)] + [(H, 1)]
        E = S * sum(i * o + o for i, o in layers)
        flat = torch.cat(draws).numpy().astype(np.float32)
        nb = -(-n_test // test_batch)
        assert flat.size == (T + nb) * E, (flat.size, T, nb, E)
        cfg = dict(layers=layers, S=S, B=B, T=T, tau=tau, lr=lr, n_train=n_train,
                   scale=n_train / B, test_batch=test_batch, y_mean=y_mean, y_std=y_std)
        arrays = dict(
            x=x[:B].numpy().astype(np.float32), y=y[:B, 0].numpy().astype(np.float32),
            xt=xt.numpy().astype(np.float32), yt=yt[:, 0].numpy().astype(np.float32),
            params0=params0.astype(np.float32), eps=flat[:T * E].reshape(T, E),
            eps_eval=flat[T * E:].reshape(nb, E), losses=-np.array(res["elbos"]),
            params=parameters_to_vector(net.parameters()).detach().numpy(),
            rmse=np.array(res["rmses"][-1]), ll=np.array(res["lls"][-1]))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), config=np.array(json.dumps(cfg)),
                            **arrays)
        print(f"wrote {name}: E={E} losses={arrays['losses']} rmse={res['rmses']} ll={res['lls']}")

    case("m1_regr_d3_h4", D=3, H=4, L=1, n_train=12, B=5, n_test=7, test_batch=7, S=3, T=4,
         tau=0.5, lr=1e-2, seed=301)
    case("m2_regr_d7_h9x2", D=7, H=9, L=2, n_train=150, B=67, n_test=21, test_batch=16, S=5, T=6,
         tau=4.0, lr=1e-2, seed=302)


def main():
    if os.environ.get("PSVI_GOLDEN_CHILD") == "1":
        _child()
        return
    env = dict(os.environ, PSVI_GOLDEN_CHILD="1", PYTHONPATH=REF)
    subprocess.run([sys.executable, os.path.abspath(__file__)], check=True, env=env, cwd=REF)


if __name__ == "__main__":
    main()
