#!/usr/bin/env python3
"""Per-phase times of one sparse-BBVI epoch on the HIP path (HIP events) and on
a dense torch CPU path (the project's modules under autograd), at mc_samples = 64, B = 128, Nu = 50 (fn, D = 2,
H = 40): the inner loop (inner_it ELBO steps), the scoring (row
log-likelihoods + selection scores) and the weight steps (outer_it row
log-likelihoods + weight gradient).  Prints one JSON line.

Usage:  python tools/sbbvi_probe.py [--reps 20] [--inner-it 10] [--outer-it 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "blackbox-coresets-vi_amd"))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner-it", type=int, default=10)
    ap.add_argument("--outer-it", type=int, default=10)
    a = ap.parse_args()
    from psvi.inference.sparsebbvi import _SparseBBVI
    from psvi.models import VILinear, make_fcnet
    from psvi.runtime import select_scores, select_weight_grad

    S, B, Nu, D, H, N = 64, 128, 50, 2, 40, 1000
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, D, generator=g)
    y = (x[:, 0] * x[:, 1] > 0).float()
    w = torch.rand(Nu, generator=g) * N / Nu
    net = make_fcnet(D, H, 1, n_layers=1, linear_class=VILinear, nonl_class=nn.ReLU, mc_samples=S)

    # ---- HIP path
    dev = torch.device("cuda")
    st = _SparseBBVI(net, dev, 1e-3, 0, None)
    xc, yc = x[:Nu].to(dev), y[:Nu].to(dev, torch.int32)
    xb, yb = x[Nu:Nu + B].to(dev), y[Nu:Nu + B].to(dev, torch.int32)
    wc = w.to(dev)

    def hip_inner():
        st.inner_loop(xc, yc, wc, a.inner_it)

    def hip_score():
        ll, _, nkl = st.loglik(xc, yc, xb, yb)
        select_scores(ll, nkl, wc, Nu, N / B)

    def hip_weights():
        for _ in range(a.outer_it):
            ll, _, nkl = st.loglik(xc, yc, xb, yb)
            select_weight_grad(ll, nkl, wc, N)

    def hip_time(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    hip = {k: hip_time(f) for k, f in (("inner_ms", hip_inner), ("score_ms", hip_score),
                                       ("weights_ms", hip_weights))}

    # ---- the same three phases as dense torch ops on the CPU (the project's
    # VILinear modules under autograd; formulas as in DESIGN §4 "Sparse-BBVI")
    cnet = make_fcnet(D, H, 1, n_layers=1, linear_class=VILinear, nonl_class=nn.ReLU, mc_samples=S)
    opt = torch.optim.Adam(cnet.parameters(), 1e-3)
    z_all = y[:Nu + B]

    def row_ll(rows, labels):
        """(ll [S, rows], nkl [S]) of one forward pass: ll = z f - softplus(f)."""
        f = cnet(rows)[..., 0]
        nkl = torch.zeros(S)
        for layer in cnet.children():
            if isinstance(layer, VILinear):
                nkl = nkl + layer.sampled_nkl()
        return labels * f - F.softplus(f), nkl

    def cpu_inner():
        opt.zero_grad()   # once: the epoch's gradients accumulate
        for _ in range(a.inner_it):
            ll, nkl = row_ll(x[:Nu], z_all[:Nu])
            loss = -S * (ll @ w).sum() - nkl.sum()   # the weighted NLL counts S times
            loss.backward()
            opt.step()

    def cpu_score():
        with torch.no_grad():
            ll, nkl = row_ll(x[:Nu + B], z_all)
            W = torch.softmax(ll[:, :Nu] @ w + nkl, 0)
            scaled = ll * (1 - W)[:, None]
            resid = N / B * scaled[:, Nu:].sum(1) - scaled[:, :Nu] @ w
            score = (scaled.T @ resid) / scaled.norm(dim=0) / S
            score[Nu:].max(), score[:Nu].abs().max()

    def cpu_weights():
        wv = w.clone().requires_grad_(True)
        for _ in range(a.outer_it):
            ll, nkl = row_ll(x[:Nu + B], z_all)
            a_s = -N / Nu * (ll[:, :Nu] @ wv)
            r_s = -N / B * ll[:, Nu:].sum(1) - a_s
            lw = nkl - a_s
            loss = (torch.softmax(lw, 0) * r_s).sum() - lw.mean()
            loss.backward()

    def cpu_time(fn):
        fn()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        return 1e3 * (time.perf_counter() - t0) / a.reps

    cpu = {k: cpu_time(f) for k, f in (("inner_ms", cpu_inner), ("score_ms", cpu_score),
                                       ("weights_ms", cpu_weights))}
    print(json.dumps(dict(S=S, B=B, Nu=Nu, D=D, H=H, inner_it=a.inner_it, outer_it=a.outer_it,
                          reps=a.reps, cpu_threads=torch.get_num_threads(), hip=hip, cpu=cpu)))


if __name__ == "__main__":
    main()
