"""The shapes whose LDS-sized solver results are pinned
(tests/golden/w2_lds_shapes.json, written by tools/gen_golden_lds_shapes.py and
checked by tests/test_lds_shapes.py): what psvi_mfvi_fit_query and
psvi_kmeans_query report where the row chunk, the state's placement and the
column tile are solved from the kernels' LDS layouts (csrc/lds_layout.hpp).
No device is needed for either query."""
import ctypes


def mfvi_grid():
    """[(dims, B, S)]: 2 and 4 affine layers, the widths' corners up to
    kMfFitMaxD = 128 / kMfFitMaxH = 64, the state in LDS and in the workspace."""
    g = []
    for L in (2, 4):
        for D in (1, 13, 128):
            for H in (1, 50, 64):
                for B in (1, 16, 512):
                    for S in (1, 64):
                        g.append(([D] + [H] * (L - 1) + [1], B, S))
    return g


def mfvi_key(dims, B, S):
    return "-".join(str(d) for d in dims) + f" B={B} S={S}"


def mfvi_query(dims, B, S):
    """[rc, placement, ws_bytes, param_count, eps_count]"""
    from psvi.runtime import _lib
    from psvi.runtime.engine import _mfvi_desc

    d = _mfvi_desc(list(zip(dims[:-1], dims[1:])), S, B, 1.0)
    out = (ctypes.c_int64 * 4)()
    rc = _lib.load().psvi_mfvi_fit_query(ctypes.byref(d), out)
    return [int(rc)] + [int(v) for v in out]


# N, D, K: the corners of K and D, D = 784 between them, few and many row tiles
KMEANS = [(N, D, K) for N in (128, 100000) for D in (1, 784, 4096) for K in (1, 128)]


def kmeans_key(N, D, K):
    return f"N={N} D={D} K={K}"


def kmeans_query(N, D, K):
    """[rc, full_bytes, min_bytes, DT, G]"""
    from psvi.runtime import _lib

    out = (ctypes.c_int64 * 4)()
    rc = _lib.load().psvi_kmeans_query(N, D, K, out)
    return [int(rc)] + [int(v) for v in out]


def measure():
    return {"mfvi_fit_query": {mfvi_key(*c): mfvi_query(*c) for c in mfvi_grid()},
            "kmeans_query": {kmeans_key(*c): kmeans_query(*c) for c in KMEANS}}
