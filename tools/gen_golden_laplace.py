#!/usr/bin/env python3
"""Golden vectors for the Laplace coreset baselines (``run_laplace``,
``run_random``, ``run_sparsevi``, ``run_opsvi`` of the reference's
psvi/inference/baselines.py; ``model`` and ``laplace_precision`` of its
psvi/models/logreg.py).

CPU only.  Like tools/gen_golden_sbbvi.py, the parent re-launches this script
in a child whose sys.path holds the reference tree (PSVI_REFERENCE, or the
path given as the first argument) and not this repo.  The child calls the
reference's own functions; the noise is supplied (q1-q3, so that the same
draws run in fp32 and in fp64) or recorded (q4) through torch.distributions'
``_standard_normal``; q4 also records every ``np.random.randint`` minibatch
and every ``random.choice``.

  q1_*  ``run_laplace`` at T in {1, 10, 200}, Nu in {0, 5}, d = 3: the fitted
        theta, the loss before each step, the precision and the samples, by the
        reference in fp32 and in fp64; ``gap`` = max |theta32 - theta64|
  q2_*  the (rows x S) log-likelihoods of ``model`` and the derived corr,
        corecorr and attach decision, at Nu = 0 and Nu = 7, B = 13
  q3_*  the weight gradient (Nu = 7) and opsvi's pseudo-input gradient by
        autograd through ``model`` (Nu = 6)
  q4_*  whole runs of the three methods on 60 halfmoon points, 4 epochs,
        inner_it = 10, outer_it = 2, S = 8, B = 20, log_every = 2

``run_opsvi`` as written does ``optim_w.zero_grad()`` followed by
``w.grad.data = ...``, which trips on this torch's ``set_to_none=True``
default; the generator hands it optimisers that zero in place, the behaviour
the reference was written against.

Usage:  PSVI_REFERENCE=<reference tree> python tools/gen_golden_laplace.py
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
    import torch.distributions.normal as normal_mod

    import psvi.inference.baselines as RB
    from psvi.models.logreg import laplace_precision, model
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
    gen = torch.Generator().manual_seed(2025)

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

    # ---- q1: run_laplace, fp32 and fp64 on the same draws
    def fit(name, T, Nu, d=3, S=4, lr=1e-2):
        x, y = data(Nu, d)
        w = 0.5 + 2.0 * torch.rand(Nu, generator=gen)
        theta0 = torch.randn(d, generator=gen)
        eps = torch.randn(S * d, generator=gen)
        cfg = dict(kind="q1", T=T, Nu=Nu, d=d, S=S, lr=lr)
        out = dict(x=npy(x, np.float32), y=npy(y, np.float32), w=npy(w, np.float32),
                   theta0=npy(theta0, np.float32), eps=npy(eps, np.float32))
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            c = lambda t: t.to(dtype)
            mu0, sigma0 = torch.zeros(d, dtype=dtype), torch.ones(d, dtype=dtype)
            theta = torch.nn.Parameter(c(theta0).clone(), requires_grad=True)
            ll0, prior0 = model(theta, mu0, sigma0, c(x), c(y), single=True)
            out["loss0_" + tag] = npy(-c(w).dot(ll0) - prior0)
            noise.replay(eps)
            smp = RB.run_laplace(theta, mu0, sigma0, c(x), c(y), c(w),
                                 torch.optim.Adam([theta], lr), inner_it=T, diagonal=True,
                                 mc_samples=S, seed=0)
            assert noise.o == eps.numel()
            noise.replay(None)
            out["theta" + tag] = npy(theta)
            out["prec" + tag] = npy(laplace_precision(c(x), theta.detach(), c(w), diagonal=True))
            out["samples" + tag] = npy(smp)
        cfg["gap"] = float(np.abs(out["theta32"] - out["theta64"]).max())
        # the fit is well conditioned: the reference alone stays far inside half a step
        assert cfg["gap"] < 0.5 * lr, cfg
        save(name, cfg, **out)

    for T in (1, 10, 200):
        for Nu in (0, 5):
            fit(f"q1_fit_T{T}_nu{Nu}", T, Nu)

    # ---- q2 / q3: log-likelihoods, scores and gradients
    def ll_of(smp, xc, yc, xb, yb):
        """model's (rows x S) log-likelihoods as [S][Nu + B], core first."""
        d = smp.shape[1]
        ll_all, _ = model(smp, torch.zeros(d, dtype=smp.dtype), torch.ones(d, dtype=smp.dtype),
                          torch.cat((xb, xc)), torch.cat((yb, yc)))
        B = xb.shape[0]
        return torch.cat((ll_all[B:], ll_all[:B])).T

    def single(kind, name, Nu, B=13, N=40, d=3, S=5):
        xc, yc = data(Nu, d)
        xb, yb = data(B, d)
        w = 0.5 + 2.0 * torch.rand(Nu, generator=gen)
        smp = torch.randn(d, generator=gen) + 0.4 * torch.randn(S, d, generator=gen)
        cfg = dict(kind=kind, Nu=Nu, B=B, N=N, d=d, S=S)
        out = dict(xc=npy(xc, np.float32), yc=npy(yc, np.float32), xb=npy(xb, np.float32),
                   yb=npy(yb, np.float32), w=npy(w, np.float32), samples=npy(smp, np.float32))
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            c = lambda t: t.to(dtype)
            ll = ll_of(c(smp), c(xc), c(yc), c(xb), c(yb))
            corr, corecorr, resid, gw = U.scores(ll, c(w), Nu, N / B)
            out["ll" + tag] = npy(ll)
            out["corr" + tag], out["corecorr" + tag] = npy(corr), npy(corecorr)
            out["resid" + tag], out["gradw" + tag] = npy(resid), npy(gw)
            if kind == "q3u":
                # baselines.py:798-805 on the reference's model
                u = c(xc).clone().requires_grad_(True)
                llu = ll_of(c(smp), u, c(yc), c(xb), c(yb)).T   # [rows][S]
                ll_core = llu[:Nu]
                cll_core = ll_core - ll_core.mean(axis=1).repeat(ll_core.shape[1], 1).T
                u_function = (torch.matmul(torch.einsum("m,ms->s", -c(w), cll_core),
                                           resid.detach()) / cll_core.shape[1])
                g = torch.autograd.grad(u_function, u)[0]
                g[:, -1] = 0
                out["gradu" + tag] = npy(g)
        if kind == "q2":
            tol = max(float(np.abs(out["corr32"] - out["corr64"]).max()),
                      float(np.abs(out["corecorr32"] - out["corecorr64"]).max()) if Nu else 0.0)
            mc, mcc = out["corr32"].max(), (out["corecorr32"].max() if Nu else -np.inf)
            s = np.sort(out["corr64"])
            cfg.update(tol_corr=tol, attach=bool(Nu == 0 or mc > mcc),
                       argmax=int(out["corr32"].argmax()),
                       gap=min(float(abs(mc - mcc)) if Nu else 1e30, 1e30),
                       top2=float(s[-1] - s[-2]))
            assert out["corr32"].argmax() == out["corr64"].argmax()
            assert cfg["gap"] > 400 * tol and cfg["top2"] > 400 * tol, cfg
        save(name, cfg, **out)

    single("q2", "q2_scores_nu0", 0)
    single("q2", "q2_scores_nu7", 7)
    single("q3w", "q3_gradw_nu7", 7)
    single("q3u", "q3_gradu_nu6", 6)

    # ---- q4: whole runs of the reference
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
        batches, choices, adam_params, cores, gaps, tols, top2s = [], [], [], [], [], [], []
        calls = [0]
        orig = (np.random.randint, random.choice, torch.optim.Adam, RB.model,
                RB.laplace_precision)

        def randint(*a, **k):
            r = orig[0](*a, **k)
            batches.append(np.asarray(r).copy())
            return r

        def choice(seq):
            r = orig[1](seq)
            choices.append(int(r))
            return r

        def adam(params, *a, **k):
            params = list(params)
            adam_params.append(params)
            return InPlaceAdam(params, *a, **k)

        def w_now():
            ws = [p[0] for p in adam_params if p[0].shape == (N,)]
            return ws[-1].detach() if ws else torch.zeros(N)

        def mdl(thetas, mu0, sigma0, xs, ys, single=False):
            r = orig[3](thetas, mu0, sigma0, xs, ys, single=single)
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
                ll = orig[3](thetas.to(dtype), mu0.to(dtype), sigma0.to(dtype), xs.to(dtype),
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
            return orig[4](z_core, theta, w, diagonal=diagonal)

        np.random.randint, random.choice, torch.optim.Adam = randint, choice, adam
        RB.model, RB.laplace_precision = mdl, prec
        kw = dict(x=x, y=y, xt=xt, yt=yt, mc_samples=S, data_minibatch=B, num_epochs=epochs,
                  log_every=log_every, N=N, D=2, seed=seed, lr0net=lr0net)
        try:
            if method == "random":
                res = RB.run_random(**kw)
            elif method == "sparsevi":
                res = RB.run_sparsevi(inner_it=inner_it, outer_it=outer_it, lr0v=lr0v, **kw)
            else:
                res = RB.run_opsvi(inner_it=inner_it, num_pseudo=num_pseudo, lr0u=lr0u,
                                   lr0v=lr0v_opsvi, register_elbos=True, log_pseudodata=True,
                                   **kw)
        finally:
            np.random.randint, random.choice, torch.optim.Adam = orig[:3]
            RB.model, RB.laplace_precision = orig[3:]
        draws = torch.cat(noise.rec)
        noise.rec = None
        last = lambda shape: [p[0] for p in adam_params if p[0].shape == shape][-1].detach()
        theta = last((3,))
        if method == "random":
            core = choices
            w = torch.zeros(N)
            w[core] = N / len(core)
        elif method == "sparsevi":
            core, w = cores[-1], last((N,))
        else:
            core, w = list(range(num_pseudo)), last((num_pseudo,))
        cfg = dict(kind="q4", method=method, N=N, S=S, B=B, epochs=epochs, inner_it=inner_it,
                   outer_it=outer_it, num_pseudo=num_pseudo, log_every=log_every, lr0net=lr0net,
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
                    batches=(np.stack(batches) if batches else np.zeros((0, B))).astype(np.int64),
                    choices=np.array(choices, np.int64), w=npy(w), theta=npy(theta),
                    core_idcs=np.array(core, np.int64), accs=np.array(res["accs"], np.float64),
                    nlls=np.array(res["nlls"], np.float64),
                    csizes=np.array(res["csizes"], np.int64))
        if method == "opsvi":
            arrs.update(u=npy(last((num_pseudo, 3))), elbos=np.array(res["elbos"], np.float64),
                        us=np.stack(res["us"]).astype(np.float64),
                        vs=np.stack(res["vs"]).astype(np.float64))
        else:
            arrs["wt_index"] = np.array(json.dumps(
                [{str(k): v for k, v in d.items()} for d in res["wt_index"]]))
        save("q4_run_" + method, cfg, **arrs)
        return True

    for method in ("random", "sparsevi", "opsvi"):
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
