"""Records every workspace size the library reports for the plans of
tests/workspace_grid.py: tests/golden/w1_workspace_sizes.json, with the commit
the library was built from.  tests/test_workspace_layout.py holds later
commits to these values exactly: a layout change that moves a size is an ABI
change and rewrites the file on purpose.

Needs the built library; no device.  Run from the repository root:
    python tools/gen_golden_workspace.py
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "blackbox-coresets-vi_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import workspace_grid as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "w1_workspace_sizes.json")


def main():
    git = lambda *a: subprocess.run(("git", "-C", ROOT) + a, capture_output=True, text=True,
                                    check=True).stdout.strip()
    dirty = git("status", "--porcelain", "--", "blackbox-coresets-vi_amd/csrc", "include")
    doc = {"commit": git("rev-parse", "HEAD") + (" (csrc modified)" if dirty else "")}
    doc.update(G.measure())
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{OUT}: {len(doc['plans'])} plans, {len(doc['kmeans_query'])} k-means shapes "
          f"at {doc['commit']}")


if __name__ == "__main__":
    main()
