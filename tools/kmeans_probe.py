"""Time psvi_kmeans on the device at the selection's shapes.

One process, device events, a warm-up, the median of several windows.  Per
shape (N, D, K) on unstructured normal rows (Lloyd needs many iterations
there, so a call with max_iter = m makes exactly m updates):

  * us per Lloyd iteration, from calls with max_iter = 2 and max_iter = 10 on
    the same initial centres: (t10 - t2) / 8, and the GB/s that implies over
    the 4 N D bytes of x;
  * the seeding: a call with max_iter = 0 that seeds, less one that is given
    its centres;
  * as context, one torch iteration in fp64 (cdist, argmin, index_add_).

Run on the GPU:  python tools/kmeans_probe.py [--windows 7] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "blackbox-coresets-vi_amd"))

SHAPES = [(6000, 784, 5), (60000, 784, 50)]


def timed(fn, windows, reps):
    """Median over windows of the mean time of reps calls, in us."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(out)


def torch_iteration(x64, c):
    labels = torch.cdist(x64, c).argmin(dim=1)
    sums = torch.zeros_like(c).index_add_(0, labels, x64)
    counts = torch.bincount(labels, minlength=c.shape[0]).clamp(min=1)
    return sums / counts[:, None].double()


def main():
    from psvi.runtime import kmeans, kmeans_query

    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for N, D, K in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(N + K)
        x = torch.randn(N, D, generator=g).to(dev)
        c0 = x[torch.randperm(N, generator=g)[:K].to(dev)].double().contiguous()
        full, least, DT, G = kmeans_query(N, D, K)
        res = {"N": N, "D": D, "K": K, "tile_columns": DT, "workgroups": G}
        for path, ws in (("one_pass", full), ("second_pass", least)):
            t = {}
            for m in (0, 2, 10):
                out = kmeans(x, K, centres=c0, max_iter=m, ws_bytes=ws)
                assert out["n_iter"] == m, (m, out["n_iter"])
                t[m] = timed(lambda m=m: kmeans(x, K, centres=c0, max_iter=m, ws_bytes=ws),
                             args.windows, args.reps)
            it = (t[10] - t[2]) / 8
            res[path] = {"ws_bytes": ws, "us_per_iteration": it,
                         "gbps_over_x": 4.0 * N * D / it / 1e3, "us_call_max_iter_0": t[0]}
        t_seed = timed(lambda: kmeans(x, K, seed=1, max_iter=0, ws_bytes=full), args.windows,
                       args.reps)
        res["us_seeding"] = t_seed - res["one_pass"]["us_call_max_iter_0"]
        x64 = x.double()
        res["us_torch_fp64_iteration"] = timed(lambda: torch_iteration(x64, c0), args.windows,
                                               args.reps)
        rows.append(res)
        print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
