#!/usr/bin/env python3
"""Times psvi_coreset_draw with device events at the two shapes run_psvi meets
on MNIST-shaped data, and -- as context only -- torch.multinomial +
index_select of the same shapes on the same device.  Not a test and not read
by bench.py; no threshold.

  REPLACE    M = 4096, n = 60,000, D = 784   (an increment's summary rows)
  NOREPLACE  M = 4096, n = 1,024,  D = 784   (a prune)

One process; every shape is warmed up first; a timed window is `batch`
back-to-back calls between two events (so that the window is not a single
launch's enqueue), divided by `batch`; the median, minimum and maximum over
`reps` windows are printed, one JSON line per shape.  The library is called
through the C ABI without the wrapper's host read of the status word, which is
checked once after the timing; `wrapper_us` is psvi.runtime.coreset_draw
with that read, on a host clock around the synchronising call."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

SHAPES = [("REPLACE", True, 4096, 60_000, 784), ("NOREPLACE", False, 4096, 1024, 784)]


def windows(fn, warmup, reps, batch):
    out = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            out.append(1e3 * a.elapsed_time(b) / batch)
    return dict(median_us=statistics.median(out), min_us=min(out), max_us=max(out))


def main(warmup, reps, batch):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                    "blackbox-coresets-vi_amd"))
    from psvi.runtime import _lib, coreset_draw
    from psvi.runtime.engine import _ptr, _stream

    if not torch.cuda.is_available():
        raise SystemExit("coreset_draw_probe needs a HIP device")
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    for name, replacement, M, n, D in SHAPES:
        w = torch.softmax(torch.randn(M, generator=g), 0).cuda()
        rows = torch.randn(M, D, generator=g).cuda()
        z = torch.randint(0, 10, (M,), generator=g).float().cuda()
        idx = torch.empty(n, dtype=torch.int32, device="cuda")
        rows_out = torch.empty(n, D, device="cuda")
        z_out = torch.empty(n, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        req = _lib.CoresetDrawReq(_ptr(w), M, n,
                                  _lib.DRAW_REPLACE if replacement else _lib.DRAW_NOREPLACE, 7, 0,
                                  _ptr(rows), D, _ptr(z), _ptr(idx), _ptr(rows_out), _ptr(z_out),
                                  _ptr(status))
        stream = _stream()

        def ours():
            rc = lib.psvi_coreset_draw(ctypes.byref(req), stream)
            assert rc == 0, rc

        def torch_ops():
            i = torch.multinomial(w, n, replacement=replacement)
            return rows.index_select(0, i), z.index_select(0, i)

        res = dict(what="psvi_coreset_draw", mode=name, M=M, n=n, D=D, reps=reps, batch=batch,
                   bytes_moved=2 * n * D * 4, **windows(ours, warmup, reps, batch))
        assert int(status.item()) == 0
        wrap = []
        for i in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            coreset_draw(w, n, replacement, 7, 0, rows=rows, targets=z)   # ends in a host read
            if i >= warmup:
                wrap.append(1e6 * (time.perf_counter() - t0))
        res["wrapper_us"] = statistics.median(wrap)
        res["torch_multinomial_index_select"] = windows(torch_ops, warmup, reps, batch)
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--batch", type=int, default=20)
    a = ap.parse_args()
    main(a.warmup, a.reps, a.batch)
