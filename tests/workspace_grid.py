"""The plans and k-means shapes whose workspace sizes are pinned
(tests/golden/w1_workspace_sizes.json, written by tools/gen_golden_workspace.py
and checked by tests/test_workspace_layout.py).  Plans are created through the
C ABI; no device is needed to create or query one."""
import ctypes

C3 = [64, 40, 40, 2]
LENET = [(25, 6), (150, 16), (400, 120), (120, 84), (84, 10)]
QUERIES = ("WS_BYTES", "LOOP_WS_BYTES", "TILED_FLOATS", "OUTER_WS_BYTES", "HVP_WS_BYTES",
           "EVAL_WS_BYTES")
# the k-means fixtures' shapes (tests/golden/x*_kmeans_*.npz): N, D, K
KMEANS = [(257, 3, 2), (1000, 70, 7), (2051, 784, 5), (64, 5, 64)]


def _ranks(world):
    return sorted({0, world - 1})


def plan_grid():
    """[(family, dims or None, S, M, world, rank, likelihood)]"""
    g = []
    # full-cov: S = 4 has no stream table, 160 and 256 no tiled state, 256 one R-op slot
    for S in (4, 32, 64, 128, 160, 256):
        g.append(("fullcov", C3, S, 100, 1, 0, None))
    g.append(("fullcov", [12, 20, 4], 128, 8, 1, 0, None))
    g.append(("fullcov", [3, 5, 2], 4, 3, 1, 0, None))
    for world in (2, 3, 8):
        for rank in _ranks(world):
            g.append(("fullcov", C3, 128, 100, world, rank, None))
    g.append(("meanfield", [2, 5, 2], 4, 3, 1, 0, None))
    g.append(("meanfield", C3, 32, 100, 1, 0, None))
    g.append(("meanfield", [5, 8, 1], 4, 3, 1, 0, ("gaussian", 2.0)))
    g.append(("meanfield", [5, 8, 1], 4, 3, 1, 0, "bernoulli"))
    for S in (8, 256):
        for M in (4, 500):
            for world in (1, 8):
                for rank in _ranks(world):
                    g.append(("lenet", None, S, M, world, rank, None))
    return g


def plan_key(family, dims, S, M, world, rank, lik):
    name = "lenet" if dims is None else "-".join(str(d) for d in dims)
    kind = lik if isinstance(lik, str) else (lik[0] if lik else "categorical")
    return f"{family} {name} S={S} M={M} world={world} rank={rank} {kind}"


def plan_sizes(family, dims, S, M, world, rank, lik):
    from psvi.runtime import InnerLoopPlan, _lib

    layers = LENET if dims is None else list(zip(dims[:-1], dims[1:]))
    p = InnerLoopPlan(family, layers, S, M, world=world, rank=rank, likelihood=lik)
    return {q: p._query(getattr(_lib, "Q_" + q)) for q in QUERIES}


def kmeans_sizes(N, D, K):
    from psvi.runtime import _lib

    out = (ctypes.c_int64 * 4)()
    rc = _lib.load().psvi_kmeans_query(N, D, K, out)
    assert rc == 0, rc
    return [int(v) for v in out]


def measure():
    plans = {plan_key(*c): plan_sizes(*c) for c in plan_grid()}
    kmeans = {f"N={N} D={D} K={K}": kmeans_sizes(N, D, K) for N, D, K in KMEANS}
    return {"plans": plans, "kmeans_query": kmeans}
