"""bench.py's plain one-GPU run (no --full), in process: the headline alone --
warm-up call, K timed steps, the result line with every side line empty -- and
--dump-outputs, which writes what the timed call left its caller.  The dumped
state must be that of one psvi_inner_loop call over the W + K steps from the
reference init on the bench's inputs (the timed call continues the warm-up)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_headline_alone_and_dumps_it(tmp_path):
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    for leg in ("c4_timings", "cpu_baseline", "c2_timings", "trainer_timings", "lenet_timings",
                "kernel_roofline"):
        setattr(b, leg, lambda *a, _leg=leg, **k: pytest.fail(f"{_leg} ran in a plain run"))
    K, W = 7, 3
    args = b.parse_args(["--gpus", "1", "--steps", str(K), "--warmup", str(W),
                         "--dump-outputs", str(tmp_path / "d")])
    dev = torch.device("cuda", 0)
    line = b.run(b.Runtime(dev, 1, 0), args)
    assert line["steps"] == K and line["warmup"] == W and line["n_gpus"] == 1
    assert line["value"] > 0 and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"] + 0.01
    assert line["config"]["elbo_finite"] and line["config"]["workload"].startswith("C3")
    assert line["step_roofline"]["frac"] > 0
    for k in ("roofline", "cold_call", "cpu_baseline", "c4_1gpu", "c2", "trainers", "lenet_c5"):
        assert line[k] is None, k
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert sorted(got) == ["adam_m", "adam_v", "neg_elbo", "params"]
    assert got["neg_elbo"].dtype == np.float64 and got["neg_elbo"].shape == (K,)
    # one call over the W + K steps, same seed: the numbers of the resumed
    # call bit for bit (tests/test_hip_loop_resident.py holds the loop to that)
    from psvi.runtime import InnerLoopPlan

    plan = InnerLoopPlan("fullcov", b.LAYERS, b.S_PER_GPU, b.M)
    u, z, w = b.synthetic_inputs(dev)
    p = b.reference_init_params(b.LAYERS, dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    elbo = plan.inner_loop(u, z, w, p, m, v, W + K, b.LR, seed=20251015)
    torch.cuda.synchronize()
    for name, t in (("params", p), ("adam_m", m), ("adam_v", v)):
        assert got[name].dtype == np.float32 and got[name].shape == (line["config"]["params"],)
        assert np.array_equal(got[name], t.cpu().numpy()), name
    # the negative ELBO is a float64 sum of at most P = 4.73e6 terms whose
    # order the two calls need not share (another workspace): n * 2^-53
    # relative, 5.3e-10, bounds the difference of two orders
    want = elbo[W:].cpu().numpy()
    err = np.abs(got["neg_elbo"] - want).max() / np.abs(want).max()
    print(f"neg_elbo: max rel difference {err:.3e}")
    assert err < 1e-9
