#!/usr/bin/env python3
"""Golden vectors for the full-precision Laplace posterior (``diagonal=False``
in the reference's psvi/inference/baselines.py: ``run_laplace``,
``run_sparsevi``, ``run_opsvi``; ``laplace_precision`` of its
psvi/models/logreg.py).

CPU only, and the same child-process pattern as tools/gen_golden_laplace.py:
the child's sys.path holds the reference tree (PSVI_REFERENCE, or the path
given as the first argument) and calls the reference's own functions.  The
noise is supplied (s1, s2) or recorded (s3) through ``_standard_normal`` of
BOTH torch.distributions.normal and torch.distributions.multivariate_normal
(each module imports the name itself).

  s1_*  ``laplace_precision(diagonal=False)`` and ``MultivariateNormal(theta,
        precision_matrix=P)``: P, scale_tril, the samples from supplied noise,
        log det P, and the factor A = scale_tril^-1 as torch forms it
        (flip(cholesky(flip(P)))^T).  The inputs are rounded to float32 first;
        the reference then runs on them in fp64 (stored) and in fp32:
        ``gap32_<output>`` = max |fp32 - fp64|.  A quarter of the weights are
        exactly 0; one case has weights around 1e4.
  s2_*  ``run_laplace(diagonal=False)`` end to end, T = 10, Nu = 5, d = 3
  s3_*  whole ``run_sparsevi`` / ``run_opsvi`` runs with ``diagonal=False`` on
        q4's 60 halfmoon points and configuration: recorded noise, minibatches,
        the margins ``gap`` / ``top2`` / ``tol_corr`` as q4 stores them, and the
        weights (and core sizes / pseudo-inputs) after every epoch, and opsvi's
        initial pseudo-points

Usage:  PSVI_REFERENCE=<reference tree> python tools/gen_golden_laplace_full.py
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
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import random

    import numpy as np
    import torch
    import torch.distributions as dist
    import torch.distributions.multivariate_normal as mvn_mod
    import torch.distributions.normal as normal_mod

    import psvi.inference.baselines as RB
    from psvi.models.logreg import laplace_precision
    import laplace_util as U   # the project's restatement (torch only)

    orig_normal = normal_mod._standard_normal

    class Noise:
        """_standard_normal: a supplied flat stream (replay) or torch's draws, recorded."""

        def __init__(self):
            self.queue, self.o, self.rec = None, 0, None

        def __call__(self, shape, dtype, device):
            n = int(np.prod(shape)) if len(shape) else 1
            if self.queue is not None:
                out = self.queue[self.o:self.o + n].reshape(shape).to(dtype=dtype, device=device)
                assert out.numel() == n
                self.o += n
                return out
            out = orig_normal(shape, dtype=dtype, device=device)
            if self.rec is not None:
                self.rec.append(out.detach().clone().reshape(-1))
            return out

        def replay(self, flat):
            self.queue, self.o = flat, 0

    noise = Noise()
    normal_mod._standard_normal = noise
    mvn_mod._standard_normal = noise
    gen = torch.Generator().manual_seed(2026)

    def data(n, d):
        """n rows with the ones column, labels from a noisy linear rule."""
        x = torch.cat((torch.randn(n, d - 1, generator=gen), torch.ones(n, 1)), dim=1)
        wt = torch.randn(d, generator=gen)
        y = (x @ wt + 0.3 * torch.randn(n, generator=gen) > 0).float()
        return x, y

    def npy(t, dt=np.float64):
        return t.detach().numpy().astype(dt)

    def save(name, cfg, **arrs):
        np.savez_compressed(os.path.join(OUT, name + ".npz"), config=np.array(json.dumps(cfg)),
                            **arrs)
        print("wrote", name, {k: getattr(v, "shape", None) for k, v in arrs.items()})

    # ---- s1: the precision, its factor, the samples and log det P
    def full(name, Nu, d, S, wscale=1.0):
        x, _ = data(Nu, d)
        w = wscale * (0.5 + 2.0 * torch.rand(Nu, generator=gen))
        w[torch.randperm(Nu, generator=gen)[:Nu // 4]] = 0.0
        theta = torch.randn(d, generator=gen) / d ** 0.5
        eps = torch.randn(S * d, generator=gen)
        cfg = dict(kind="s1", Nu=Nu, d=d, S=S, wscale=wscale, n_zero=int((w == 0).sum()))
        out = dict(x=npy(x, np.float32), w=npy(w, np.float32), theta=npy(theta, np.float32),
                   eps=npy(eps, np.float32))
        res = {}
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            c = lambda t: t.to(dtype)
            prec = laplace_precision(c(x), c(theta), c(w), diagonal=False)
            mvn = dist.MultivariateNormal(c(theta), precision_matrix=prec)
            noise.replay(eps)
            smp = mvn.rsample((S,))
            assert noise.o == eps.numel()
            noise.replay(None)
            factor = torch.flip(torch.linalg.cholesky(torch.flip(prec, (-2, -1))), (-2, -1)).mT
            res[tag] = dict(prec=npy(prec), scale_tril=npy(mvn.scale_tril), samples=npy(smp),
                            factor=npy(factor), logdet=npy(torch.logdet(prec)).reshape(1))
        for k, v in res["64"].items():
            out[k + "64"] = v
            cfg["gap32_" + k] = float(np.abs(res["32"][k] - v).max())
        cfg["cond"] = float(np.linalg.cond(res["64"]["prec"]))
        print(name, {k: v for k, v in cfg.items() if k.startswith("gap") or k == "cond"})
        save(name, cfg, **out)

    for Nu, d, S in ((0, 5, 4), (1, 2, 1), (5, 3, 8), (40, 17, 8), (100, 65, 8), (300, 128, 8)):
        full(f"s1_full_nu{Nu}_d{d}", Nu, d, S)
    full("s1_full_nu40_d17_w1e4", 40, 17, 8, wscale=1e4)

    # ---- s2: run_laplace(diagonal=False), fp32 and fp64 on the same draws
    def fit(name, T=10, Nu=5, d=3, S=4, lr=1e-2):
        x, y = data(Nu, d)
        w = 0.5 + 2.0 * torch.rand(Nu, generator=gen)
        theta0 = torch.randn(d, generator=gen)
        eps = torch.randn(S * d, generator=gen)
        cfg = dict(kind="s2", T=T, Nu=Nu, d=d, S=S, lr=lr)
        out = dict(x=npy(x, np.float32), y=npy(y, np.float32), w=npy(w, np.float32),
                   theta0=npy(theta0, np.float32), eps=npy(eps, np.float32))
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            c = lambda t: t.to(dtype)
            mu0, sigma0 = torch.zeros(d, dtype=dtype), torch.ones(d, dtype=dtype)
            theta = torch.nn.Parameter(c(theta0).clone(), requires_grad=True)
            noise.replay(eps)
            smp = RB.run_laplace(theta, mu0, sigma0, c(x), c(y), c(w),
                                 torch.optim.Adam([theta], lr), inner_it=T, diagonal=False,
                                 mc_samples=S, seed=0)
            assert noise.o == eps.numel()
            noise.replay(None)
            out["theta" + tag] = npy(theta)
            out["prec" + tag] = npy(laplace_precision(c(x), theta.detach(), c(w), diagonal=False))
            out["samples" + tag] = npy(smp)
        cfg["gap"] = float(np.abs(out["theta32"] - out["theta64"]).max())
        cfg["gap32_samples"] = float(np.abs(out["samples32"] - out["samples64"]).max())
        assert cfg["gap"] < 0.5 * lr, cfg
        save(name, cfg, **out)

    fit("s2_run_laplace_full")

    # ---- s3: whole runs of the reference with diagonal=False
    class InPlaceAdam(torch.optim.Adam):
        def zero_grad(self, set_to_none=False):
            super().zero_grad(set_to_none=False)

    def run(method, seed, N=60, Nt=20, S=8, B=20, epochs=4, inner_it=10, outer_it=2,
            num_pseudo=6, log_every=2, lr0net=1e-2, lr0v=1e-1, lr0u=1e-2, lr0v_opsvi=1e-3):
        from sklearn.datasets import make_moons

        X, Y = make_moons(n_samples=N + Nt, noise=0.1, random_state=seed)
        X, Y = torch.from_numpy(X.astype(np.float32)), torch.from_numpy(Y.astype(np.float32))
        x, y, xt, yt = X[:N], Y[:N], X[N:], Y[N:]
        x_aug = torch.cat((x, torch.ones(N, 1)), dim=1)
        noise.rec = []
        batches, adam_params, cores, gaps, tols, top2s = [], [], [], [], [], []
        w_steps, core_steps, u_steps, full_calls, init = [], [], [], [0], {}
        calls = [0]
        per_epoch = 1 + outer_it if method == "sparsevi" else 1
        orig = (np.random.randint, torch.optim.Adam, RB.model, RB.laplace_precision)

        def last(shape):
            return [p[0] for p in adam_params if p[0].shape == shape][-1].detach()

        def w_now():
            ws = [p[0] for p in adam_params if p[0].shape == (N,)]
            return ws[-1].detach() if ws else torch.zeros(N)

        def snapshot():
            if method == "sparsevi":
                w_steps.append(npy(w_now()).copy())
                core_steps.append(list(cores[-1]))
            else:
                w_steps.append(npy(last((num_pseudo,))).copy())
                u_steps.append(npy(last((num_pseudo, 3))).copy())

        def randint(*a, **k):
            if batches and len(batches) % per_epoch == 0:
                snapshot()   # the first minibatch of an epoch: the state the last one left
            r = orig[0](*a, **k)
            batches.append(np.asarray(r).copy())
            return r

        def adam(params, *a, **k):
            params = list(params)
            adam_params.append(params)
            if params[0].shape == (num_pseudo, 3):
                init.setdefault("u0", npy(params[0]).copy())
            return InPlaceAdam(params, *a, **k)

        def mdl(thetas, mu0, sigma0, xs, ys, single=False):
            r = orig[2](thetas, mu0, sigma0, xs, ys, single=single)
            if method == "opsvi" and not single:
                init.setdefault("z", npy(ys[B:]).copy())
            if single or method != "sparsevi":
                return r
            k, calls[0] = calls[0], calls[0] + 1
            if k % (1 + outer_it):
                return r
            # the attach decision of this epoch, in fp32 and in fp64
            Nu = xs.shape[0] - B
            core = [int((x_aug == row).all(1).nonzero()[0, 0]) for row in xs[B:]]
            w = w_now()[core]
            sc = {}
            for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
                ll = orig[2](thetas.to(dtype), mu0.to(dtype), sigma0.to(dtype), xs.to(dtype),
                             ys.to(dtype))[0]
                ll = torch.cat((ll[B:], ll[:B])).T
                sc[tag] = U.scores(ll, w.to(dtype), Nu, N / B)
            tols.append(float((sc["32"][0] - sc["64"][0]).abs().max()))
            s = np.sort(npy(sc["64"][0]))
            top2s.append(float(s[-1] - s[-2]))
            if Nu:
                tols.append(float((sc["32"][1] - sc["64"][1]).abs().max()))
                gaps.append(float(abs(sc["32"][0].max() - sc["32"][1].max())))
            return r

        def prec(z_core, theta, w, diagonal=False):
            cores.append([int((x_aug == row).all(1).nonzero()[0, 0]) for row in z_core]
                         if method != "opsvi" else [])
            full_calls[0] += not diagonal
            return orig[3](z_core, theta, w, diagonal=diagonal)

        np.random.randint, torch.optim.Adam = randint, adam
        RB.model, RB.laplace_precision = mdl, prec
        kw = dict(x=x, y=y, xt=xt, yt=yt, mc_samples=S, data_minibatch=B, num_epochs=epochs,
                  log_every=log_every, N=N, D=2, seed=seed, lr0net=lr0net, diagonal=False)
        try:
            if method == "sparsevi":
                res = RB.run_sparsevi(inner_it=inner_it, outer_it=outer_it, lr0v=lr0v, **kw)
            else:
                res = RB.run_opsvi(inner_it=inner_it, num_pseudo=num_pseudo, lr0u=lr0u,
                                   lr0v=lr0v_opsvi, register_elbos=True, log_pseudodata=True,
                                   **kw)
        finally:
            np.random.randint, torch.optim.Adam = orig[:2]
            RB.model, RB.laplace_precision = orig[2:]
        snapshot()
        draws = torch.cat(noise.rec)
        noise.rec = None
        assert len(w_steps) == epochs and len(batches) == epochs * per_epoch
        assert full_calls[0] == epochs * per_epoch   # every selection-loop fit, no logging fit
        theta = last((3,))
        if method == "sparsevi":
            core, w = cores[-1], last((N,))
        else:
            core, w = list(range(num_pseudo)), last((num_pseudo,))
        cfg = dict(kind="s3", method=method, diagonal=False, N=N, S=S, B=B, epochs=epochs,
                   inner_it=inner_it, outer_it=outer_it, num_pseudo=num_pseudo,
                   log_every=log_every, lr0net=lr0net,
                   lr0v=lr0v_opsvi if method == "opsvi" else lr0v, lr0u=lr0u, seed=seed,
                   gap=min(gaps) if gaps else 1e30, top2=min(top2s) if top2s else 1e30,
                   tol_corr=max(tols) if tols else 0.0)
        print(method, "seed", seed, "core", core, "csizes", res["csizes"], "accs", res["accs"],
              "gap", cfg["gap"], "top2", cfg["top2"], "tol", cfg["tol_corr"])
        # every decision well clear of rounding (100 x the tolerance of 4 x the
        # reference's own fp32-against-fp64 gap); otherwise the next seed is tried
        if not (cfg["gap"] > 400 * cfg["tol_corr"] and cfg["top2"] > 400 * cfg["tol_corr"]):
            return False
        arrs = dict(x=npy(x, np.float32), y=npy(y, np.float32), xt=npy(xt, np.float32),
                    yt=npy(yt, np.float32), draws=npy(draws, np.float32),
                    batches=np.stack(batches).astype(np.int64), w=npy(w), theta=npy(theta),
                    core_idcs=np.array(core, np.int64), accs=np.array(res["accs"], np.float64),
                    nlls=np.array(res["nlls"], np.float64),
                    csizes=np.array(res["csizes"], np.int64), w_steps=np.stack(w_steps))
        if method == "opsvi":
            arrs.update(u=npy(last((num_pseudo, 3))), elbos=np.array(res["elbos"], np.float64),
                        u_steps=np.stack(u_steps), u0=init["u0"], z=init["z"])
        else:
            arrs["core_sizes"] = np.array([len(c) for c in core_steps], np.int64)
            assert all(c == core[:len(c)] for c in core_steps)
            arrs["wt_index"] = np.array(json.dumps(
                [{str(k): v for k, v in d.items()} for d in res["wt_index"]]))
        save("s3_run_" + method + "_full", cfg, **arrs)
        return True

    for method in ("sparsevi", "opsvi"):
        for seed in range(200):
            if run(method, seed):
                break
        else:
            raise SystemExit(f"no seed with clear margins ({method})")


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
