#!/usr/bin/env python3
"""Golden vectors for sparse black-box VI (``run_sparsevi_with_bb_elbo``,
psvi/inference/sparsebbvi.py of the reference; ``elbo``,
``forward_through_coreset``, ``sparsevi_psvi_elbo``, ``predict_through_coreset``
of its psvi/inference/utils.py:85-141).

CPU only.  Like tools/gen_golden.py, the parent re-launches this script in a
child whose sys.path holds the reference tree (PSVI_REFERENCE, or the path
given as the first argument) and not this repo.  The child calls the
reference's own functions; the Monte-Carlo noise of every forward pass is
supplied (s1-s3, so that the same draws run in fp32 and in fp64) or recorded
(s4) through torch.distributions' ``_standard_normal``, and s4 also records
every ``np.random.randint`` minibatch.

  s1_*  one ``elbo`` value and gradient, at Nu = 0 and Nu = 5
  s2_*  ``forward_through_coreset`` outputs and the derived corr, corecorr and
        attach decision, at Nu = 0 and Nu = 7, B = 13
  s3_*  ``sparsevi_psvi_elbo`` and its gradient w.r.t. the core weights
  s4_*  whole runs of 3 epochs (logreg D = 2; fn D = 3, H = 10), S = 5, inner_it = 3,
        outer_it = 2, log_every = 1: final w, core_idcs, parameters, accs, nlls

Every fixture holds the fp32 reference values (what the reference computes)
and, for s1-s3, the same computation in fp64; ``tol_corr`` is the reference's
own fp32-against-fp64 gap of corr / corecorr, ``gap`` the margin |max corr -
max corecorr| of every attach decision.

Usage:  PSVI_REFERENCE=<reference tree> python tools/gen_golden_sbbvi.py
"""
import copy
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
    import numpy as np
    import torch
    import torch.distributions.normal as normal_mod
    import torch.nn as nn
    from torch.nn.utils import parameters_to_vector, vector_to_parameters

    import psvi.inference.sparsebbvi as SB
    from psvi.inference.utils import elbo, forward_through_coreset, sparsevi_psvi_elbo
    from psvi.models.neural_net import VILinear, make_fcnet
    import sbbvi_util as U   # the project's restatement of the scores (torch only)

    orig_normal = normal_mod._standard_normal

    class Noise:
        """_standard_normal: a supplied flat stream (replay) or torch's draws,
        recorded per forward pass."""

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
    gen = torch.Generator().manual_seed(2024)

    def make_net(arch, D, H, S, dtype):
        torch.set_default_dtype(dtype)
        net = (nn.Sequential(VILinear(D, 1, mc_samples=S)) if arch == "logreg"
               else make_fcnet(D, H, 1, n_layers=1, linear_class=VILinear, nonl_class=nn.ReLU,
                               mc_samples=S))
        torch.set_default_dtype(torch.float32)
        return net

    def layers_of(net):
        return [(m.in_features, m.out_features) for m in net.modules() if isinstance(m, VILinear)]

    def perturbed(net):
        p = parameters_to_vector(net.parameters()).detach().clone()
        o = 0
        for m in net.modules():
            if not isinstance(m, VILinear):
                continue
            n = m.weight.numel() + m.bias.numel()
            p[o:o + n] = 0.7 * torch.randn(n, generator=gen)
            p[o + n:o + 2 * n] = -3.0 + 2.0 * torch.rand(n, generator=gen)
            o += 2 * n
        return p

    def data(n, D):
        x = torch.randn(n, D, generator=gen)
        wt = torch.randn(D, generator=gen)
        y = (x @ wt + 0.3 * torch.randn(n, generator=gen) > 0).float()
        return x, y

    def scores(ll_core, ll_data, weights, w, sum_scaling):
        """corr and corecorr (None for an empty core) from
        forward_through_coreset's outputs, by the project's own statement of
        the selection scores (tests/sbbvi_util.py), in the inputs' precision."""
        Nu = ll_core.shape[0]
        ll = torch.cat((ll_core, ll_data)).T   # [S][Nu + B], core first
        _, corr, corecorr = U.scores_given_weights(ll, weights, w, Nu, sum_scaling)
        return corr, (corecorr if Nu else None)

    def nkl_of(net):
        """The layers' sampled KL terms of the last forward pass, summed: (S,)."""
        total = 0.0
        for layer in net.children():
            if isinstance(layer, VILinear):
                total = total + layer.sampled_nkl()
        return total

    def npy(t, dt=np.float64):
        return t.detach().numpy().astype(dt)

    def save(name, cfg, **arrs):
        np.savez_compressed(os.path.join(OUT, name + ".npz"), config=np.array(json.dumps(cfg)),
                            **arrs)
        print("wrote", name, {k: getattr(v, "shape", None) for k, v in arrs.items()})

    # ---- s1 / s2 / s3: single evaluations, fp32 and fp64 on the same draws
    def single(kind, name, arch, D, H, S, Nu, B, N):
        net32 = make_net(arch, D, H, S, torch.float32)
        p0 = perturbed(net32)
        layers = layers_of(net32)
        n_tot = sum(i * o + o for i, o in layers)
        eps = torch.randn(S * n_tot, generator=gen)
        u, z = data(Nu, D)
        xb, yb = data(B, D)
        w = 0.5 + 2.0 * torch.rand(Nu, generator=gen)
        cfg = dict(kind=kind, arch=arch, D=D, H=H, S=S, Nu=Nu, B=B, N=N, layers=layers)
        out = dict(params=npy(p0, np.float32), eps=npy(eps, np.float32), u=npy(u, np.float32),
                   z=npy(z, np.float32), xb=npy(xb, np.float32), yb=npy(yb, np.float32),
                   w=npy(w, np.float32))
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            net = make_net(arch, D, H, S, dtype)
            vector_to_parameters(p0.to(dtype), list(net.parameters()))
            c = lambda t: t.to(dtype)
            noise.replay(eps)
            if kind == "s1":
                for p in net.parameters():
                    p.grad = None
                loss = elbo(net, c(u), c(z), c(w))
                nkl = nkl_of(net)
                loss.backward()
                out["loss" + tag] = npy(loss)
                out["nkl" + tag] = npy(nkl)
                out["grad" + tag] = npy(torch.cat([p.grad.reshape(-1) for p in net.parameters()]))
            elif kind == "s2":
                llc, lld, W = forward_through_coreset(net, c(u), c(xb), c(z), c(yb), c(w))
                nkl = nkl_of(net)
                corrs, corecorrs = scores(llc, lld, W, c(w), N / B)
                out["ll" + tag] = npy(torch.cat((llc, lld)).T)   # [S][Nu + B], core first
                out["nkl" + tag] = npy(nkl)
                out["W" + tag] = npy(W)
                out["corr" + tag] = npy(corrs)
                out["corecorr" + tag] = npy(corecorrs) if corecorrs is not None else np.zeros(0)
            else:
                wv = c(w).clone().requires_grad_(True)
                loss = sparsevi_psvi_elbo(net, c(xb), c(u), c(yb), c(z), wv, N)
                loss.backward()
                out["loss" + tag] = npy(loss)
                out["gradw" + tag] = npy(wv.grad)
            assert noise.o == eps.numel()
            noise.replay(None)
        if kind == "s2":
            tol = max(float(np.abs(out["corr32"] - out["corr64"]).max()),
                      float(np.abs(out["corecorr32"] - out["corecorr64"]).max()) if Nu else 0.0)
            mc, mcc = out["corr32"].max(), (out["corecorr32"].max() if Nu else -np.inf)
            cfg.update(tol_corr=tol, attach=bool(Nu == 0 or mc > mcc),
                       argmax=int(out["corr32"].argmax()),
                       gap=float(abs(mc - mcc)) if Nu else float("inf"))
            assert out["corr32"].argmax() == out["corr64"].argmax()
            assert cfg["gap"] > 400 * tol, (cfg["gap"], tol)
            s = np.sort(out["corr64"])
            assert s[-1] - s[-2] > 400 * tol  # the argmax is clear of rounding too
            cfg["gap"] = min(cfg["gap"], 1e30)
        save(name, cfg, **out)

    single("s1", "s1_elbo_nu0", "fn", 3, 10, 5, 0, 1, 40)
    single("s1", "s1_elbo_nu5", "fn", 3, 10, 5, 5, 1, 40)
    single("s2", "s2_scores_nu0", "fn", 3, 10, 5, 0, 13, 40)
    single("s2", "s2_scores_nu7", "fn", 3, 10, 5, 7, 13, 40)
    single("s3", "s3_weights_nu7", "fn", 3, 10, 5, 7, 13, 40)
    single("s3", "s3_weights_logreg", "logreg", 2, 0, 5, 4, 13, 40)

    # ---- s4: whole runs of the reference
    def run(name, arch, D, H, S, N, Nt, B, epochs, lr0, seed):
        x, y = data(N, D)
        xt, yt = data(Nt, D)
        x, xt = 2.0 * x, 2.0 * xt
        noise.rec = []
        batches, adam_params, cores, gaps, tols = [], [], [], [], []
        orig_randint, orig_adam = np.random.randint, torch.optim.Adam
        orig_fwd, orig_pe = SB.forward_through_coreset, SB.sparsevi_psvi_elbo

        def randint(*a, **k):
            r = orig_randint(*a, **k)
            batches.append(np.asarray(r).copy())
            return r

        def adam(params, *a, **k):
            params = list(params)
            adam_params.append(params)
            return orig_adam(params, *a, **k)

        def fwd(net, u, xb, z, yb, w):
            r = orig_fwd(net, u, xb, z, yb, w)
            corrs, corecorrs = scores(r[0], r[1], r[2], w, N / B)
            # the same forward in fp64 on the draws it just consumed
            k = 2 * sum(isinstance(m, VILinear) for m in net.modules())
            net64 = copy.deepcopy(net).double()
            noise.replay(torch.cat(noise.rec[-k:]))
            d = lambda t: t.double()
            r64 = orig_fwd(net64, d(u), d(xb), d(z), d(yb), d(w))
            noise.replay(None)
            c64, cc64 = scores(r64[0], r64[1], r64[2], d(w), N / B)
            tols.append(float((corrs - c64).abs().max()))
            if corecorrs is not None:
                tols.append(float((corecorrs - cc64).abs().max()))
                gaps.append(float(abs(corrs.max() - corecorrs.max())))
            return r

        def pe(net, xb, u, yb, z, w, Nn):
            cores.append([int((x == row).all(1).nonzero()[0, 0]) for row in u])
            return orig_pe(net, xb, u, yb, z, w, Nn)

        np.random.randint, torch.optim.Adam = randint, adam
        SB.forward_through_coreset, SB.sparsevi_psvi_elbo = fwd, pe
        p0 = {}
        orig_vil, orig_fc = SB.VILinear, SB.make_fcnet

        def vil(*a, **k):
            m = orig_vil(*a, **k)
            p0["p"] = torch.cat([m.weight.reshape(-1), m.bias.reshape(-1),
                                 m._weight_sd.reshape(-1), m._bias_sd.reshape(-1)]).detach().clone()
            return m

        def fc(*a, **k):
            net = orig_fc(*a, **k)
            p0["p"] = parameters_to_vector(net.parameters()).detach().clone()
            return net

        SB.VILinear, SB.make_fcnet = vil, fc
        try:
            res = SB.run_sparsevi_with_bb_elbo(
                n_layers=1, logistic_regression=arch == "logreg", n_hidden=H, log_every=1,
                lr0=lr0, register_elbos=True, seed=seed, num_epochs=epochs, inner_it=3,
                outer_it=2, x=x, y=y, xt=xt, yt=yt, mc_samples=S, data_minibatch=B,
                scatterplot_coreset=False)
        finally:
            np.random.randint, torch.optim.Adam = orig_randint, orig_adam
            SB.forward_through_coreset, SB.sparsevi_psvi_elbo = orig_fwd, orig_pe
            SB.VILinear, SB.make_fcnet = orig_vil, orig_fc
        draws = torch.cat(noise.rec)
        noise.rec = None
        net_params, (w,) = adam_params
        pf = parameters_to_vector(net_params).detach()
        cfg = dict(kind="s4", arch=arch, D=D, H=H, S=S, N=N, B=B, epochs=epochs, lr0=lr0,
                   seed=seed, inner_it=3, outer_it=2,
                   layers=[(D, 1)] if arch == "logreg" else [(D, H), (H, 1)],
                   gap=min(gaps) if gaps else 1e30, tol_corr=max(tols))
        print(name, "seed", seed, "core", cores[-1], "csizes", res["csizes"], "accs",
              res["accs"], "gaps", gaps, "tol", max(tols))
        # every attach decision well clear of rounding: 100 x the tolerance (4 x the
        # reference's own fp32-against-fp64 gap); otherwise the caller tries the next seed
        if not cfg["gap"] > 400 * cfg["tol_corr"]:
            return False
        save(name, cfg, x=npy(x, np.float32), y=npy(y, np.float32), xt=npy(xt, np.float32),
             yt=npy(yt, np.float32), params0=npy(p0["p"], np.float32),
             draws=npy(draws, np.float32), batches=np.stack(batches).astype(np.int64),
             w=npy(w), core_idcs=np.array(cores[-1], np.int64), params=npy(pf),
             accs=np.array(res["accs"], np.float64), nlls=np.array(res["nlls"], np.float64),
             csizes=np.array(res["csizes"], np.int64),
             elbos=np.array(res["elbos"], np.float64))
        return True

    for seed in range(200):
        if run("s4_run_logreg", "logreg", 2, 0, 5, 40, 20, 13, 3, 5e-2, seed):
            break
    else:
        raise SystemExit("no seed with a clear attach margin (logreg)")
    for seed in range(200):
        if run("s4_run_fn", "fn", 3, 10, 5, 40, 20, 13, 3, 5e-2, seed):
            break
    else:
        raise SystemExit("no seed with a clear attach margin (fn)")


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
