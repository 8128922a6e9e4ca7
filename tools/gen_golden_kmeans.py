"""Fixtures of psvi_kmeans (tests/golden/x*_kmeans_*.npz): inputs, initial
centres and what sklearn's Lloyd makes of them,

    KMeans(K, init=C0, n_init=1, algorithm="lloyd", max_iter=300, tol=0).fit(x.astype(float64))

(labels, centres, inertia, n_iter), with the minimum relative margin
(d_second - d_best) / (d_best + d_second) over all iterations and rows of the
float64 restatement (tests/kmeans_util.py).  The generator walks data seeds
until the margin is >= 1e-6 -- fp64 order effects are ~ D 2^-53 ~ 1e-13, so
every implementation of the rules must then give the same labels -- and no
cluster goes empty in any iteration (sklearn would relocate its centre, the
library keeps it), and checks that the restatement reproduces sklearn.

Needs scikit-learn (1.7.2 wrote the committed files).  Run from the repository
root:  python tools/gen_golden_kmeans.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_util as KM  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-6
# name, N, D, K, kind
CASES = [("x1_kmeans_n257_d3_k2", 257, 3, 2, "normal"),
         ("x2_kmeans_n1000_d70_k7", 1000, 70, 7, "blobs"),
         ("x3_kmeans_n2051_d784_k5", 2051, 784, 5, "pixels"),
         ("x4_kmeans_n64_d5_k64", 64, 5, 64, "normal")]


def make(kind, N, D, K, rng):
    if kind == "normal":
        return rng.standard_normal((N, D)).astype(np.float32)
    if kind == "blobs":       # overlapping blobs: a few dozen iterations
        mu = 1.5 * rng.standard_normal((K, D))
        return (mu[rng.integers(0, K, N)] + rng.standard_normal((N, D))).astype(np.float32)
    # "pixels": small integers around K prototypes, stored as int8 (the file
    # stays under the size limit)
    mu = rng.integers(0, 12, (K + 2, D))
    return (mu[rng.integers(0, K + 2, N)] + rng.integers(-3, 4, (N, D))).astype(np.int8)


def main():
    from sklearn import __version__ as skv
    from sklearn.cluster import KMeans

    for name, N, D, K, kind in CASES:
        for data_seed in range(1000):
            rng = np.random.default_rng([20261021, N, D, K, data_seed])
            x = make(kind, N, D, K, rng)
            xf = x.astype(np.float32)
            c0 = xf[rng.permutation(N)[:K]].astype(np.float64)
            if np.unique(c0, axis=0).shape[0] < K:
                continue
            r = KM.lloyd(xf, c0, max_iter=300, tol=0.0)
            if r["margin"] < MARGIN or r["min_count"] == 0:
                continue
            break
        else:
            raise SystemExit(f"{name}: no data seed gives the margin")
        km = KMeans(K, init=c0, n_init=1, algorithm="lloyd", max_iter=300, tol=0).fit(
            xf.astype(np.float64))
        assert np.array_equal(km.labels_, r["labels"]) and km.n_iter_ == r["n_iter"], name
        assert np.abs(km.cluster_centers_ - r["centres"]).max() <= 1e-9 * np.abs(r["centres"]).max()
        assert abs(km.inertia_ - r["inertia"]) <= 1e-9 * r["inertia"] or r["inertia"] == 0.0
        cfg = dict(N=N, D=D, K=K, kind=kind, data_seed=data_seed, sklearn=skv, margin=r["margin"])
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), config=json.dumps(cfg), x=x, c0=c0,
                            labels=km.labels_.astype(np.int32), centres=km.cluster_centers_,
                            inertia=np.float64(km.inertia_), n_iter=np.int32(km.n_iter_),
                            margin=np.float64(r["margin"]))
        size = os.path.getsize(os.path.join(GOLDEN, name + ".npz"))
        print(f"{name}: data seed {data_seed}, n_iter {km.n_iter_}, margin {r['margin']:.3e}, "
              f"{size} bytes")
        assert size < 1 << 20


if __name__ == "__main__":
    main()
