#!/usr/bin/env python3
"""Time of the MFVI selection's scoring pass: one psvi_predict_scores launch over
N = 60,000 rows (fn 64-100-4, C2's net; S = 32, 128 rows per draw; entropy,
correct and the statistics) against the same pass as the model's torch forward on the device in 128-row batches (what baselines._evaluate does:
mean logit, argmax, Categorical log-prob per batch).  The kernel's time includes
drawing its eps with psvi_randn; the torch forward draws its own.  Timed with
device events after a warm-up; prints one JSON line.

Usage:  python tools/predict_scores_probe.py [--rows 60000] [--reps 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "blackbox-coresets-vi_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch

    from psvi.inference.baselines import _MFVIStepper
    from psvi.models import categorical_fn, make_fcnet

    dev = torch.device("cuda")
    D, H, C, S, N, B = 64, 100, 4, 32, a.rows, 128
    torch.manual_seed(0)
    net = make_fcnet(D, H, C, n_layers=1, mc_samples=S).to(dev)  # C2's net: 64-100-4
    x = torch.randn(N, D, device=dev)
    y = torch.randint(0, C, (N,), device=dev).float()
    stepper = _MFVIStepper(net, dev, 1e-3, 0)

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

    def kernel():
        return stepper.predict(x, y, B, want=("entropy", "correct"), stats=True)

    from psvi.runtime import randn_
    eps = torch.empty(-(-N // B) * stepper._plan(1).eps_count, device=dev)
    randn_(eps, 1, 0)

    def kernel_given_eps():
        from psvi.runtime import predict_scores
        return predict_scores(stepper._plan(1), x, y.to(torch.int32), eps, stepper.params, B,
                              want=("entropy", "correct"), stats=True)

    def torch_forward():
        corrects, nll = 0.0, 0.0
        with torch.no_grad():
            for lo in range(0, N, B):
                logits = net(x[lo:lo + B]).squeeze(-1).mean(0)
                corrects += logits.argmax(-1).float().eq(y[lo:lo + B]).float().sum()
                nll += -categorical_fn(logits=logits).log_prob(y[lo:lo + B]).sum()
        return corrects, nll

    out = {"shape": dict(layers=stepper.layers, S=S, N=N, rows_per_draw=B),
           "kernel_with_draw_s": timed(kernel), "kernel_s": timed(kernel_given_eps),
           "torch_forward_s": timed(torch_forward)}
    out["speedup_with_draw"] = out["torch_forward_s"] / out["kernel_with_draw_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
