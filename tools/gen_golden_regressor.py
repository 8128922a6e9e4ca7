#!/usr/bin/env python3
"""Golden vectors for the Gaussian-likelihood (regressor) family.

Runs ONLY in the development container (the reference is mounted read-only at
/root/reference); like tools/gen_golden_variants.py the parent re-launches
this script in a child interpreter whose sys.path holds the reference and not
this repo.  In float64 with every Monte-Carlo draw rounded to fp32 and
recorded in call order, the child runs the reference's own

  * PSVI_regressor / PSVILearnV_regressor / PSVIAV_regressor
    (psvi_classes.py:1940-2335) on make_regressor_net (neural_net.py:300-331)

and writes numeric-only fixtures tests/golden/r*.npz:

  r1*  inner_elbo: value, gradients w.r.t. the parameters, u, v and z
  r2*  psvi_elbo: value, gradients w.r.t. the parameters, u, v / alpha and z
       (PSVI_regressor and PSVIAV_regressor)
  r3*  one whole nested_step of each of the three classes (T = 3, learn_z):
       final parameters, u / v / z / alpha and their gradients, plus the
       reference's own fp32 replay of the same draws
  r4*  evaluate -> (rmse, test_ll) over two test batches with non-trivial
       y_mean / y_std

u, z, v, alpha and the model are set explicitly.  PSVI_regressor.__init__
reads a module global ``device_id`` the reference never defines
(psvi_classes.py:1975); the child sets it to None before constructing.

Usage:  python tools/gen_golden_regressor.py
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
    import copy

    import numpy as np
    import torch
    import torch.distributions.normal as normal_mod
    from torch.nn.utils import parameters_to_vector

    from psvi.inference import psvi_classes as PC
    from psvi.models.neural_net import VILinear, make_regressor_net

    PC.device_id = None
    torch.set_default_dtype(torch.float64)
    draws, replay = [], []
    orig = normal_mod._standard_normal

    def standard_normal(shape, dtype, device):
        if replay:
            out = replay.pop(0).reshape(shape).to(dtype)
        else:
            out = orig(shape, dtype=dtype, device=device).float().to(dtype)
        draws.append(out.detach().clone().reshape(-1))
        return out

    normal_mod._standard_normal = standard_normal
    gen = torch.Generator().manual_seed(777)
    LR = dict(lr0net=1e-3, lr0u=1e-3, lr0v=1e-2, lr0z=1e-2, lr0alpha=1e-2)
    SHAPES = dict(small=dict(D=3, H=10, L=1, M=5, S=3), large=dict(D=6, H=24, L=2, M=37, S=8))
    NX, N = 11, 300

    def rnd(*shape, scale=1.0):
        return (scale * torch.randn(*shape, generator=gen)).float().double()

    def make_model(sh):
        m = make_regressor_net(sh["D"], sh["H"], 1, n_layers=sh["L"], mc_samples=sh["S"],
                               init_sd=0.05)
        with torch.no_grad():
            for name, p in m.named_parameters():
                if name.split(".")[-1] in ("weight", "bias"):
                    p.copy_(0.4 * torch.randn(p.shape, generator=gen))
                else:
                    p.copy_(-3.0 + 2.0 * torch.rand(p.shape, generator=gen))
                p.copy_(p.float().double())
        return m

    def make_obj(cls_name, model, sh, tau, u0, z0, v0, alpha0, T, y_mean=0.0, y_std=1.0):
        obj = getattr(PC, cls_name)(u=None, z=None, N=N, D=sh["D"], num_pseudo=sh["M"],
                                    mc_samples=sh["S"], tau=tau, y_mean=y_mean, y_std=y_std,
                                    learn_z=True, lr0alpha=LR["lr0alpha"])
        obj.model = model
        obj.u = u0.detach().clone().requires_grad_(True)
        obj.z = z0.detach().clone().requires_grad_(True)
        obj.v = v0.detach().clone().requires_grad_(True)
        obj.learn_v = True
        obj.inner_it, obj.log_every, obj.scheduler_optim_net = T, 10, None
        obj.optim_net = torch.optim.Adam(list(model.parameters()), LR["lr0net"])
        obj.optim_u = torch.optim.Adam([obj.u], LR["lr0u"])
        obj.optim_v = torch.optim.Adam([obj.v], LR["lr0v"])
        obj.optim_z = torch.optim.Adam([obj.z], LR["lr0z"])
        if alpha0 is not None:
            with torch.no_grad():
                obj.alpha.fill_(alpha0)
            obj.optim_alpha = torch.optim.Adam([obj.alpha], LR["lr0alpha"])
        return obj

    def start_v(cls_name, M):
        # PSVI_regressor: f = identity on positive v; the others softmax(v)
        if cls_name == "PSVI_regressor":
            return ((1.0 + 0.3 * torch.rand(M, generator=gen)) / M).float().double()
        return rnd(M, scale=0.2)

    def grads(obj, model, with_params):
        res = {}
        for key, t in (("u_grad", obj.u), ("v_grad", obj.v), ("z_grad", obj.z)) + (
                (("alpha_grad", obj.alpha),) if hasattr(obj, "alpha") else ()):
            if t.grad is not None:
                res[key] = t.grad.detach().numpy().copy()
        if with_params:
            res["grad_params"] = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).numpy()
        return res

    def save(name, cfg, arrays):
        np.savez_compressed(os.path.join(OUT, name + ".npz"), config=np.array(json.dumps(cfg)),
                            **arrays)
        print(f"wrote {name}: keys={sorted(arrays)}")

    def case(name, kind, cls_name, shape, tau, alpha0=None, T=3, seed=0):
        sh = SHAPES[shape]
        torch.manual_seed(seed)
        model = make_model(sh)
        model32 = copy.deepcopy(model).float()
        M, D, S = sh["M"], sh["D"], sh["S"]
        u0, z0, v0 = rnd(M, D), rnd(M), start_v(cls_name, M)
        xb, yb = rnd(NX, D), rnd(NX)
        layers = [[m.in_features, m.out_features] for m in model.modules()
                  if isinstance(m, VILinear)]
        cfg = dict(family="mf", layers=layers, S=S, M=M, N=N, Nx=NX, T=T, tau=tau, prior_sd=1.0,
                   cls=cls_name, kind=kind, alpha0=alpha0, seed=seed, **LR)
        arr = dict(params0=parameters_to_vector(model.parameters()).detach().numpy().astype(np.float32),
                   u0=u0.numpy().astype(np.float32), z0=z0.numpy().astype(np.float32),
                   v0=v0.numpy().astype(np.float32), xb=xb.numpy().astype(np.float32),
                   yb=yb.numpy().astype(np.float32))
        obj = make_obj(cls_name, model, sh, tau, u0, z0, v0, alpha0, T)
        draws.clear()
        if kind == "inner":
            loss = obj.inner_elbo(model=model)
            loss.backward()
            arr.update(out=np.array(float(loss.detach())), eps=torch.cat(draws).numpy().astype(np.float32),
                       **grads(obj, model, True))
        elif kind == "outer":
            loss = obj.psvi_elbo(xb, yb, model=model)
            loss.backward()
            arr.update(out=np.array(float(loss.detach())), eps=torch.cat(draws).numpy().astype(np.float32),
                       **grads(obj, model, True))
        elif kind == "nested":
            per = 2 * len(layers)  # draws per objective evaluation (W, b per layer)
            loss = obj.nested_step(xb, yb)
            rec = [d.clone() for d in draws]
            assert len(rec) == per * (T + 1)
            ev = [torch.cat(rec[i * per:(i + 1) * per]).numpy().astype(np.float32)
                  for i in range(T + 1)]
            arr.update(out=np.array(float(loss.detach())), eps_inner=np.stack(ev[:T]),
                       eps_outer=ev[T], u=obj.u.detach().numpy(), v=obj.v.detach().numpy(),
                       z=obj.z.detach().numpy(),
                       params=parameters_to_vector(model.parameters()).detach().numpy(),
                       **grads(obj, model, False))
            if alpha0 is not None:
                arr["alpha"] = obj.alpha.detach().numpy()
            # the reference's own fp32 run on the identical draws
            torch.set_default_dtype(torch.float32)
            replay[:] = [d.float() for d in rec]
            o32 = make_obj(cls_name, model32, sh, tau, u0.float(), z0.float(), v0.float(), alpha0, T)
            o32.nested_step(xb.float(), yb.float())
            assert not replay
            for k, g in grads(o32, model32, False).items():
                arr[k + "_fp32"] = g.astype(np.float64)
            arr["params_fp32"] = parameters_to_vector(model32.parameters()).detach().numpy().astype(np.float64)
            torch.set_default_dtype(torch.float64)
        elif kind == "evaluate":
            y_mean, y_std = 1.7, 2.3
            obj = make_obj(cls_name, model, sh, tau, u0, z0, v0, alpha0, T, y_mean, y_std)
            nts = [11, 7]
            batches = [(rnd(n, D), y_mean + y_std * rnd(n)) for n in nts]
            obj.test_loader = batches
            draws.clear()
            rmse, ll = obj.evaluate()
            per = 2 * len(layers)
            assert len(draws) == per * len(nts)
            cfg.update(y_mean=y_mean, y_std=y_std, nts=nts)
            for i, (xt, yt) in enumerate(batches):
                arr[f"xt{i}"] = xt.numpy().astype(np.float32)
                arr[f"yt{i}"] = yt.numpy().astype(np.float32)
                arr[f"eps{i}"] = torch.cat(draws[i * per:(i + 1) * per]).numpy().astype(np.float32)
            arr.update(rmse=np.array(float(rmse)), test_ll=np.array(float(ll)))
        save(name, cfg, arr)

    seed = 100
    for shape in ("small", "large"):
        for tau, tn in ((0.1, "t01"), (4.0, "t4")):
            seed += 1
            case(f"r1_inner_{shape}_{tn}", "inner", "PSVILearnV_regressor", shape, tau, seed=seed)
            case(f"r2_outer_{shape}_{tn}", "outer", "PSVI_regressor", shape, tau, seed=seed + 20)
            case(f"r2_outer_av_{shape}_{tn}", "outer", "PSVIAV_regressor", shape, tau,
                 alpha0=0.3, seed=seed + 40)
            case(f"r4_eval_{shape}_{tn}", "evaluate", "PSVILearnV_regressor", shape, tau,
                 seed=seed + 60)
    case("r3_nested_small_t01", "nested", "PSVI_regressor", "small", 0.1, seed=201)
    case("r3_nested_lv_large_t4", "nested", "PSVILearnV_regressor", "large", 4.0, seed=202)
    case("r3_nested_av_small_t4", "nested", "PSVIAV_regressor", "small", 4.0, alpha0=0.3, seed=203)


def main():
    if os.environ.get("PSVI_GOLDEN_CHILD") == "1":
        _child()
        return
    env = dict(os.environ, PSVI_GOLDEN_CHILD="1", PYTHONPATH=REF)
    subprocess.run([sys.executable, os.path.abspath(__file__)], check=True, env=env, cwd=REF)


if __name__ == "__main__":
    main()
