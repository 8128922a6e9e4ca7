"""Every kernel compiles for gfx950 without scratch memory or VGPR spills.

A per-lane index into a by-value kernel-argument struct makes the compiler
copy the whole struct to scratch and turns every argument read into a
dependent memory load (this happened once to the network kernel, silently:
results stay right, the kernel gets slower).  hipcc's kernel-resource-usage
remarks expose it at build time, so the CPU suite guards it.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blackbox-coresets-vi_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _resources(src, tmp_path):
    out = tmp_path / (os.path.basename(src) + ".o")
    cmd = [HIPCC, "--offload-arch=gfx950", "-munsafe-fp-atomics", "-O3", "-std=c++17", "-fPIC",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", src, "-o", str(out),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            kernels[cur][m.group(1).strip()] = int(m.group(2))
    return kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("src", ["kernels_net.hip", "kernels_mvn_fwd.hip", "kernels_mvn_update.hip",
                                 "kernels_mvn_kstream.hip", "kernels_mvn_stream.hip", "kernels_mf.hip",
                                 "kernels_outer.hip", "kernels_rop.hip", "kernels_lenet.hip"])
def test_no_scratch_no_spills(src, tmp_path):
    """No scratch memory traffic anywhere.  A VGPR spill is tolerated only into the
    accumulation registers (ScratchSize 0): at one wave per SIMD the kernel
    owns all 512 registers of the lane, and hipcc parks a few values in AGPRs
    (a register move) once the 256 architectural VGPRs are full."""
    kernels = _resources(os.path.join(CSRC, src), tmp_path)
    assert kernels, "no kernel resource remarks parsed"
    touching = _scratch_users(os.path.join(CSRC, src), tmp_path)
    bad = {k: v for k, v in kernels.items()
           if (v.get("ScratchSize", 0) and k in touching)
           or (v.get("VGPRs Spill", 0) and v.get("Occupancy", 2) > 1)}
    assert not bad, f"kernels using scratch or spilling VGPRs: {bad}"


# private-memory instructions of gfx950 code: scratch_* (flat scratch) and
# buffer accesses through the private segment descriptor s[0:3]
_SCRATCH_INSN = re.compile(r"^\s*(scratch_\w+|buffer_(load|store)\w*\s.*\bs\[0:3\])")


def _scratch_users(src, tmp_path):
    """Kernels whose ISA contains an instruction that touches private memory.
    A non-zero ScratchSize with no such instruction is the register
    scavenger's emergency slot, reserved under register pressure and never
    used (the network kernel's looped-chunk instantiation): no scratch traffic."""
    out = tmp_path / (os.path.basename(src) + ".s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-munsafe-fp-atomics", "-O3", "-std=c++17", "-fPIC",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only", src,
           "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    users, cur = set(), None
    for line in open(out):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur and _SCRATCH_INSN.match(line):
            users.add(cur)
    return users
