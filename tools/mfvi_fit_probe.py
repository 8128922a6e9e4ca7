#!/usr/bin/env python3
"""Steps per second of the MFVI regressor fit: one psvi_mfvi_fit call against the
step-by-step path it replaces (psvi_randn + psvi_elbo_grad + psvi_adam_update
and a host read of the loss per step, _MFVIStepper's sequence), at the default
regressor (D = 13, H = 50 x 2, B = 128, S = 4), T = 2000, for G = 1 and G = 3
(the step-by-step path runs its G fits one after another).  Timed with device
events after a warm-up; prints one JSON line.

Usage:  python tools/mfvi_fit_probe.py [--steps 2000] [--reps 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "blackbox-coresets-vi_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch

    from psvi.runtime import InnerLoopPlan, adam_update_, mfvi_fit, mfvi_fit_query, randn_

    dev = "cuda"
    D, H, B, S, T = 13, 50, 128, 4, a.steps
    layers = [(D, H), (H, H), (H, 1)]
    q = mfvi_fit_query(layers, S, B)
    P, E = q["param_count"], q["eps_count"]
    stride = (E + 3) // 4 * 4
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, D, generator=g).to(dev)
    y = torch.randn(B, generator=g).to(dev)
    p0 = (0.1 * torch.randn(P, generator=g)).to(dev)
    taus = [0.1, 1.0, 10.0]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e-3)
        return best

    def fused(G):
        params = p0.repeat(G, 1).contiguous()
        mfvi_fit(layers, S, x, y, 3.0, taus[:G], params, T, 1e-3, seed=1,
                 offsets=[g_ * T * stride for g_ in range(G)])

    def stepwise(G):
        for gi in range(G):
            plan = InnerLoopPlan("meanfield", layers, S, B, likelihood=("gaussian", taus[gi]))
            params = p0.clone()
            m, v = torch.zeros_like(params), torch.zeros_like(params)
            w = torch.full((B,), 3.0, device=dev)
            eps = torch.empty(E, device=dev)
            ws = plan.workspace(dev)
            for t in range(T):
                randn_(eps, 1, (gi * T + t) * stride)
                loss, grad = plan.elbo_grad(x, y, w, eps, params, ws=ws)
                adam_update_(params, grad, m, v, step=t + 1, lr=1e-3, kind="torch")
                loss.item()

    out = {"shape": dict(D=D, H=H, B=B, S=S, T=T), "placement": q["placement"]}
    for G in (1, 3):
        tf, ts = timed(lambda: fused(G)), timed(lambda: stepwise(G))
        out[f"G{G}"] = {"fused_s": tf, "fused_steps_per_s": G * T / tf,
                        "stepwise_s": ts, "stepwise_steps_per_s": G * T / ts}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
