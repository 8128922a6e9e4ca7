"""Records what the shape solvers that size their row blocks from the kernels'
LDS layouts report for the shapes of tests/lds_shapes_grid.py:
tests/golden/w2_lds_shapes.json, with the commit the library was built from.
tests/test_lds_shapes.py holds later commits to these values exactly: an LDS
layout change that moves one changes what callers allocate and how the
kernels tile, and rewrites the file on purpose.

Needs the built library; no device.  Run from the repository root:
    python tools/gen_golden_lds_shapes.py
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "blackbox-coresets-vi_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import lds_shapes_grid as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "w2_lds_shapes.json")


def main():
    git = lambda *a: subprocess.run(("git", "-C", ROOT) + a, capture_output=True, text=True,
                                    check=True).stdout.strip()
    dirty = git("status", "--porcelain", "--", "blackbox-coresets-vi_amd/csrc", "include")
    doc = {"commit": git("rev-parse", "HEAD") + (" (csrc modified)" if dirty else "")}
    doc.update(G.measure())
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{OUT}: {len(doc['mfvi_fit_query'])} MFVI fit shapes, {len(doc['kmeans_query'])} "
          f"k-means shapes at {doc['commit']}")


if __name__ == "__main__":
    main()
