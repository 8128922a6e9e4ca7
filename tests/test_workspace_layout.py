"""Every workspace size the library reports stays what it was.

tests/golden/w1_workspace_sizes.json holds PSVI_Q_WS_BYTES, LOOP_WS_BYTES,
TILED_FLOATS, OUTER_WS_BYTES, HVP_WS_BYTES and EVAL_WS_BYTES of the plans of
tests/workspace_grid.py, and psvi_kmeans_query of the k-means fixtures' shapes,
as recorded at the commit the file names (tools/gen_golden_workspace.py).  The
sizes are part of the ABI: callers allocate by them.  Equality, no tolerance;
no device needed."""
import json
import os

import pytest

import workspace_grid as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "w1_workspace_sizes.json")
with open(GOLDEN) as f:
    RECORDED = json.load(f)


def test_grid_is_the_recorded_one():
    assert sorted(G.plan_key(*c) for c in G.plan_grid()) == sorted(RECORDED["plans"])
    assert sorted(f"N={N} D={D} K={K}" for N, D, K in G.KMEANS) == sorted(RECORDED["kmeans_query"])
    for sizes in RECORDED["plans"].values():
        assert sorted(sizes) == sorted(G.QUERIES)


@pytest.mark.parametrize("case", G.plan_grid(), ids=lambda c: G.plan_key(*c))
def test_plan_workspace_sizes(case):
    assert G.plan_sizes(*case) == RECORDED["plans"][G.plan_key(*case)]


@pytest.mark.parametrize("shape", G.KMEANS, ids=lambda s: "N=%d D=%d K=%d" % s)
def test_kmeans_query(shape):
    assert G.kmeans_sizes(*shape) == RECORDED["kmeans_query"]["N=%d D=%d K=%d" % shape]
