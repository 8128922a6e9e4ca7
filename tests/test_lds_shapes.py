"""What the LDS-sized shape solvers report stays what it was.

tests/golden/w2_lds_shapes.json holds psvi_mfvi_fit_query (the state's
placement, the workspace bytes, the counts) and psvi_kmeans_query (the
workspace bytes, the column tile, the grid) of the shapes of
tests/lds_shapes_grid.py, as recorded at the commit the file names
(tools/gen_golden_lds_shapes.py).  Both are solved from the kernels' LDS byte
counts (csrc/lds_layout.hpp): a layout that moved a byte count moves them.
Equality, no tolerance; no device needed."""
import json
import os

import pytest

import lds_shapes_grid as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "w2_lds_shapes.json")
with open(GOLDEN) as f:
    RECORDED = json.load(f)


def test_grid_is_the_recorded_one():
    assert sorted(G.mfvi_key(*c) for c in G.mfvi_grid()) == sorted(RECORDED["mfvi_fit_query"])
    assert sorted(G.kmeans_key(*c) for c in G.KMEANS) == sorted(RECORDED["kmeans_query"])


def test_both_placements_are_recorded():
    placed = {v[1] for v in RECORDED["mfvi_fit_query"].values() if v[0] == 0}
    assert placed == {0, 1}


@pytest.mark.parametrize("case", G.mfvi_grid(), ids=lambda c: G.mfvi_key(*c))
def test_mfvi_fit_query(case):
    assert G.mfvi_query(*case) == RECORDED["mfvi_fit_query"][G.mfvi_key(*case)]


@pytest.mark.parametrize("shape", G.KMEANS, ids=lambda s: G.kmeans_key(*s))
def test_kmeans_query(shape):
    assert G.kmeans_query(*shape) == RECORDED["kmeans_query"][G.kmeans_key(*shape)]
