"""The work lists of a plan hold what the kernels assume of them.

plan_tables.cpp builds every table of a plan on the host.  The stand-alone
program tests/cpp/plan_tables_check.cpp builds the plans of a list of shapes
(no GPU use) and checks the streaming run table, the K-split and segmented
tables, the forward items and the update chunks, and holds the R-op geometry of
every plan of a grid to tests/golden/w3_rop_geometry.json; `make check-tables` compiles
both with the address and undefined-behaviour sanitizers and runs the program.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "blackbox-coresets-vi_amd")


def test_plan_tables_check():
    r = subprocess.run(["make", "-C", PKG, "-j", "2", "check-tables"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "plans ok" in r.stdout
