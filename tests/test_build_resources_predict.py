"""kernels_predict.hip under the build-resources guard of
tests/test_build_resources.py: no scratch memory traffic, no VGPR spills."""
import os

import pytest

from test_build_resources import CSRC, HIPCC, _resources, _scratch_users


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_predict_unit_no_scratch_no_spills(tmp_path):
    src = os.path.join(CSRC, "kernels_predict.hip")
    kernels = _resources(src, tmp_path)
    assert len(kernels) == 3, kernels
    touching = _scratch_users(src, tmp_path)
    bad = {k: v for k, v in kernels.items()
           if (v.get("ScratchSize", 0) and k in touching)
           or (v.get("VGPRs Spill", 0) and v.get("Occupancy", 2) > 1)}
    assert not bad, f"kernels using scratch or spilling VGPRs: {bad}"
