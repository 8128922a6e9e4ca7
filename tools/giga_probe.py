#!/usr/bin/env python3
"""Times one geodesic-ascent step of GIGA (psvi_giga_step) at S = 100,
n_data = 512, d = 65 -- run_giga's defaults on a 64-feature dataset -- with
hipEvents, and the same step written in torch ops (fp32, as the reference
runs it) on this CPU.  Not a test and not read by bench.py.

  python tools/giga_probe.py          the kernel (needs a HIP device)
  python tools/giga_probe.py --cpu    the torch ops on this CPU

One process, warm-up launches first, the median of the timed repeats reported;
each mode prints one JSON line with the machine it ran on."""
import argparse
import json
import os
import platform
import statistics
import sys
import time

import torch

S, N, D = 100, 512, 65


def problem():
    g = torch.Generator().manual_seed(0)
    rows = torch.cat((torch.randn(N, D - 1, generator=g), torch.ones(N, 1)), dim=1)
    labels = (torch.rand(N, generator=g) > 0.5).float()
    samples = (torch.randn(D, generator=g) + 0.5 * torch.randn(S, D, generator=g)) / D ** 0.5
    lw = torch.randn(S, generator=g)
    return samples, rows, labels, lw / lw.norm()


def gpu(warmup, reps):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                    "blackbox-coresets-vi_amd"))
    from psvi.runtime import giga_step

    samples, rows, labels, lw = (t.cuda().contiguous() for t in problem())
    times = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        giga_step(samples, rows, labels, lw)
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    print(json.dumps(dict(what="psvi_giga_step", S=S, n_data=N, d=D, reps=reps,
                          median_ms=statistics.median(times), min_ms=min(times),
                          max_ms=max(times), device=torch.cuda.get_device_name(0))))


def cpu(warmup, reps):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import giga_util as G

    samples, rows, labels, lw = problem()
    bce = torch.nn.BCEWithLogitsLoss(reduction="none")
    times = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        G.step(-bce(samples @ rows.T, labels.repeat(S, 1)), lw)
        if i >= warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps(dict(what="torch ops (CPU, fp32)", S=S, n_data=N, d=D, reps=reps,
                          median_ms=statistics.median(times), min_ms=min(times),
                          threads=torch.get_num_threads(), machine=platform.processor()
                          or platform.machine(), torch=torch.__version__)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    cpu(a.warmup, a.reps) if a.cpu else gpu(a.warmup, a.reps)
