#!/usr/bin/env python3
"""Golden vectors for the GIGA coreset baseline (``run_giga`` of the
reference's psvi/inference/baselines.py:207-423).

CPU only.  Like tools/gen_golden_laplace.py, the parent re-launches this script
in a child whose sys.path holds the reference tree (PSVI_REFERENCE, or the
path given as the first argument) and not this repo.  The child calls the
reference's own ``run_giga``, in fp32 and -- under
``torch.set_default_dtype(torch.float64)``, on the same recorded draws and
minibatches -- in fp64.  ``run_giga`` keeps its step in local variables; they
are read from its frame when it calls ``torch.clamp_`` at the end of a step.

  k1_*  single geodesic steps, S = 50, n_data = 32, d = 3: ``run_laplace`` is
        made to return the given samples, ``torch.zeros(S)`` the given lw and
        ``np.random.randint`` the given minibatch, so that one epoch of the
        reference runs exactly one step from those inputs
          k1_step_first   lw = 0
          k1_step_mid     lw after three steps of an fp32 run
  k2_*  whole runs, N = 200, D = 2, data_minibatch = 32, subset_size = 40,
        num_epochs = 6, 10 test points:
          k2_run_log1     log_every = 1
          k2_run_log2     log_every = 2 (the coreset grows on logging
                          iterations only)
        with every host draw and minibatch, and per logging step pt_idx, gamma,
        lw, w, the test probabilities, csizes, accs, nlls

Each fixture records the reference's own fp32-against-fp64 gaps ``tol_score``,
``tol_gamma``, ``tol_lw``, ``tol_w``.  Seeds are searched until, in the fp64
run alone, every step's best score is 100 x 4 x tol_score clear of the best
score of any other data point (the minibatch is drawn with replacement, so
copies of the winner tie), every gamma denominator exceeds that margin in
magnitude, and every test probability lies farther from 0.5 than 100 x 4 x its
own gap -- and the fp32 run picks the same points and logs the same accs.

Usage:  PSVI_REFERENCE=<reference tree> python tools/gen_golden_giga.py
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
    import numpy as np
    import torch
    import torch.distributions.normal as normal_mod

    import psvi.inference.baselines as RB
    import giga_util as G   # the project's restatement (torch only): top2_gap

    orig_normal = normal_mod._standard_normal
    S, D, B, SUB, NT = 50, 2, 32, 40, 10

    def npy(t, dt=np.float64):
        return np.asarray(t.detach() if torch.is_tensor(t) else t).astype(dt)

    def save(name, cfg, **arrs):
        np.savez_compressed(os.path.join(OUT, name + ".npz"), config=np.array(json.dumps(cfg)),
                            **arrs)
        print("wrote", name, {k: getattr(v, "shape", None) for k, v in arrs.items()})

    def data(N, seed):
        from sklearn.datasets import make_moons

        X, Y = make_moons(n_samples=N + NT, noise=0.1, random_state=seed)
        X, Y = torch.from_numpy(X.astype(np.float32)), torch.from_numpy(Y.astype(np.float32))
        return X[:N], Y[:N], X[N:], Y[N:]

    def run_ref(dtype, xs, epochs, log_every, seed, draws=None, batches=None, inject=None,
                lr0net=1e-2):
        """The reference's run_giga under default dtype ``dtype``: (results, the
        step's locals at each clamp_, draws, minibatches).  ``draws`` /
        ``batches`` replay a recording; ``inject`` = (samples, lw) replaces the
        posterior samples and the initial lw."""
        x, y, xt, yt = (t.to(dtype) for t in xs)
        N = x.shape[0]
        rec_d, rec_b, steps, o, calls = [], [], [], [0], [0]
        it_b = iter(batches) if batches is not None else None
        orig = (np.random.randint, torch.clamp_, RB.run_laplace, torch.zeros)

        def normal(shape, dtype, device):
            n = int(np.prod(shape)) if len(shape) else 1
            if draws is None:
                out = orig_normal(shape, dtype=dtype, device=device)
                rec_d.append(out.detach().clone().reshape(-1))
                return out
            out = draws[o[0]:o[0] + n].reshape(shape).to(dtype=dtype, device=device)
            assert out.numel() == n
            o[0] += n
            return out

        def randint(*a, **k):
            r = orig[0](*a, **k) if it_b is None else np.asarray(next(it_b))
            assert r.shape == (k["size"],)
            rec_b.append(np.asarray(r).copy())
            return r

        def clamp_(t, *a, **k):
            r = orig[1](t, *a, **k)
            loc = sys._getframe(1).f_locals
            n = len(loc["sub_idcs"])
            steps.append(dict(
                pt_idx=int(loc["pt_idx"]), sub=np.asarray(loc["sub_idcs"]).copy(),
                score=npy(loc["dns"] @ loc["d"]), ll=npy(loc["ll_all"][:n].T),
                zeta0=float(loc["zeta0"]), zeta1=float(loc["zeta1"]), zeta2=float(loc["zeta2"]),
                gamma=float(loc["gamma"]), lw=npy(loc["lw"]), w=npy(loc["w"]),
                probs=npy(loc["test_probs"]), samples=npy(loc["param_samples"]),
                core=[int(i) for i in loc["core_idcs"]]))
            return r

        def laplace(*a, **k):
            calls[0] += 1
            if inject is not None and calls[0] == 1:
                return inject[0].to(dtype)
            return orig[2](*a, **k)

        def zeros(*a, **k):
            if inject is not None and a == (S,) and not k:
                return inject[1].to(dtype).clone()
            return orig[3](*a, **k)

        old = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        normal_mod._standard_normal = normal
        np.random.randint, torch.clamp_, RB.run_laplace, torch.zeros = randint, clamp_, laplace, zeros
        try:
            res = RB.run_giga(x=x, y=y, xt=xt, yt=yt, mc_samples=S, data_minibatch=B,
                              num_epochs=epochs, log_every=log_every, N=N, D=D, seed=seed,
                              subset_size=SUB, lr0net=lr0net)
        finally:
            np.random.randint, torch.clamp_, RB.run_laplace, torch.zeros = orig
            normal_mod._standard_normal = orig_normal
            torch.set_default_dtype(old)
        if draws is not None:
            assert o[0] == draws.numel()
        if it_b is not None:
            assert next(it_b, None) is None
        return res, steps, (torch.cat(rec_d) if rec_d else None), rec_b

    def den_of(s):
        return s["zeta0"] - s["zeta1"] * s["zeta2"] + s["zeta1"] - s["zeta0"] * s["zeta2"]

    def top2(s):
        return G.top2_gap(torch.as_tensor(s["score"]), s["sub"])

    # ---- k1: single steps, the reference's own code in fp32 and in fp64
    def single(name, xs, samples, sub, lw_in, seed):
        N = xs[0].shape[0]
        out = {}
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            _, steps, _, _ = run_ref(dtype, xs, 1, 1, seed, batches=[np.zeros(SUB, np.int64), sub],
                                     inject=(samples, lw_in))
            (out[tag],) = steps
        a, b = out["32"], out["64"]
        for s in (a, b):   # w starts at zero: w[pt] = gamma scale
            s["scale"] = float(s["w"][s["pt_idx"]] / s["gamma"])
        cfg = dict(kind="k1", S=S, n_data=B, d=D + 1, N=N, seed=seed,
                   tol_score=float(np.abs(a["score"] - b["score"]).max()),
                   tol_gamma=abs(a["gamma"] - b["gamma"]),
                   tol_lw=float(np.abs(a["lw"] - b["lw"]).max()),
                   tol_w=float(np.abs(a["w"] - b["w"]).max()),
                   top2=top2(b), den=abs(den_of(b)), argmax=int(b["score"].argmax()))
        print(name, cfg)
        margin = 400 * cfg["tol_score"]
        if not (cfg["top2"] > margin and cfg["den"] > margin and a["pt_idx"] == b["pt_idx"]
                and int(a["score"].argmax()) == cfg["argmax"]):
            return False
        x_aug = torch.cat((xs[0], torch.ones(N, 1)), dim=1)
        arrs = dict(samples=npy(samples, np.float32), rows=npy(x_aug[sub], np.float32),
                    labels=npy(xs[1][sub], np.float32), lw_in=npy(lw_in, np.float32),
                    sub=np.asarray(sub, np.int64))
        for tag, s in out.items():
            arrs.update({k + tag: np.asarray(s[k], np.float64) for k in
                         ("ll", "score", "zeta0", "zeta1", "zeta2", "gamma", "lw", "scale", "w")})
            arrs["pt_idx" + tag] = np.array(s["pt_idx"], np.int64)
        save(name, cfg, **arrs)
        return True

    def k1(seed):
        xs = data(100, seed)
        _, steps, _, batches = run_ref(torch.float32, xs, 3, 1, seed)
        samples = torch.as_tensor(steps[0]["samples"], dtype=torch.float32)
        lw3 = torch.as_tensor(steps[2]["lw"], dtype=torch.float32)
        nxt = np.random.RandomState(seed + 1000).randint(100, size=B)
        return (single("k1_step_first", xs, samples, batches[1], torch.zeros(S), seed)
                and single("k1_step_mid", xs, samples, nxt, lw3, seed))

    # ---- k2: whole runs
    def k2(name, xs, seed, log_every, epochs=6):
        N = xs[0].shape[0]
        r32, s32, draws, batches = run_ref(torch.float32, xs, epochs, log_every, seed)
        r64, s64, _, _ = run_ref(torch.float64, xs, epochs, log_every, seed, draws=draws,
                                 batches=batches)
        if [s["pt_idx"] for s in s32] != [s["pt_idx"] for s in s64]:
            return None
        gap = lambda k: max(float(np.abs(np.asarray(a[k]) - np.asarray(b[k])).max())
                            for a, b in zip(s32, s64))
        cfg = dict(kind="k2", N=N, D=D, S=S, B=B, subset_size=SUB, epochs=epochs,
                   log_every=log_every, seed=seed, lr0net=1e-2, tol_score=gap("score"),
                   tol_gamma=gap("gamma"), tol_lw=gap("lw"), tol_w=gap("w"),
                   top2=min(top2(s) for s in s64), den=min(abs(den_of(s)) for s in s64))
        p32, p64 = np.stack([s["probs"] for s in s32]), np.stack([s["probs"] for s in s64])
        print(name, "seed", seed, "pts", [s["pt_idx"] for s in s64], "csizes", r64["csizes"],
              "accs", r64["accs"], cfg)
        margin = 400 * cfg["tol_score"]
        if not (cfg["top2"] > margin and cfg["den"] > margin and r32["accs"] == r64["accs"]
                and r32["csizes"] == r64["csizes"]
                and (np.abs(p64 - 0.5) > 400 * np.abs(p32 - p64)).all()):
            return None
        arrs = dict(x=npy(xs[0], np.float32), y=npy(xs[1], np.float32), xt=npy(xs[2], np.float32),
                    yt=npy(xs[3], np.float32), draws=npy(draws, np.float32),
                    subset=batches[0].astype(np.int64), batches=np.stack(batches[1:]).astype(np.int64),
                    samples=s32[0]["samples"].astype(np.float32),
                    pt_idx=np.array([s["pt_idx"] for s in s64], np.int64),
                    gamma=np.array([s["gamma"] for s in s64]),
                    lw=np.stack([s["lw"] for s in s64]), w=np.stack([s["w"] for s in s64]),
                    probs32=p32, probs64=p64, top2s=np.array([top2(s) for s in s64]),
                    dens=np.array([den_of(s) for s in s64]),
                    core_idcs=np.array(s64[-1]["core"], np.int64),
                    accs=np.array(r64["accs"]), nlls=np.array(r64["nlls"]),
                    csizes=np.array(r64["csizes"], np.int64))
        return name, cfg, arrs

    for seed in range(200):
        if k1(seed):
            break
    else:
        raise SystemExit("no seed with clear margins (k1)")
    for seed in range(200):
        xs = data(200, seed)
        a = k2("k2_run_log1", xs, seed, 1)
        b = a and k2("k2_run_log2", xs, seed, 2)
        # the second run logs on every other iteration: half the steps, half the points
        if a and b and 2 * len(b[2]["core_idcs"]) == len(a[2]["core_idcs"]):
            for name, cfg, arrs in (a, b):
                save(name, cfg, **arrs)
            break
    else:
        raise SystemExit("no seed with clear margins (k2)")


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
