"""Host side of the MFVI regression baselines, no GPU: the float64 restatement
against the reference's own fit (fixtures m*, 1e-4 relative), the argument
checks of psvi_mfvi_fit at the header's ranges, the host functions' refusals
and the offline regression data."""
import ctypes

import numpy as np
import pytest
import torch

import mfvi_regr_util as R
from golden_util import fixture_names, load_fixture, rel

TOL = 1e-4


@pytest.mark.parametrize("name", fixture_names("m"))
def test_restatement_reproduces_reference_fit(name):
    f = load_fixture(name)
    c = f["cfg"]
    L, p, _, _ = R.fit(c["layers"], c["S"], f["x"], f["y"], c["scale"], c["tau"], f["params0"],
                       f["eps"], c["lr"])
    e_loss, e_par = rel(L, f["losses"]), rel(p, f["params"])
    print(f"{name}: losses {e_loss:.2e}, params {e_par:.2e}")
    assert e_loss < TOL and e_par < TOL
    tb, se, sl = c["test_batch"], 0.0, 0.0
    for b in range(f["eps_eval"].shape[0]):
        yt = f["yt"][b * tb:(b + 1) * tb]
        r, l = R.predict(c["layers"], p, f["eps_eval"][b], c["S"], f["xt"][b * tb:(b + 1) * tb], yt,
                         c["tau"], c["y_mean"], c["y_std"])
        se, sl = se + r * r * len(yt), sl + l * len(yt)
    n = len(f["yt"])
    assert rel(np.sqrt(se / n), f["rmse"]) < TOL and rel(sl / n, f["ll"]) < TOL


def test_fixture_names_present():
    assert fixture_names("m") == ["m1_regr_d3_h4", "m2_regr_d7_h9x2"]


def _req(**over):
    from psvi.runtime import _lib

    d = _lib.NetDesc()
    dims = over.pop("dims", [13, 50, 50, 1])
    d.n_layers = over.pop("n_layers", len(dims) - 1)
    for i, v in enumerate(dims):
        d.dims[i] = v
    d.S, d.M, d.prior_sd = over.pop("S", 4), over.pop("M", 128), over.pop("prior_sd", 1.0)
    tau = (ctypes.c_float * 16)(*([1.0] * 16))
    off = (ctypes.c_uint64 * 16)()
    if "tau0" in over:
        tau[0] = over.pop("tau0")
    if "off0" in over:
        off[0] = over.pop("off0")
    b = ctypes.c_void_p(256)  # never dereferenced: every call below fails its checks first
    kw = dict(desc=ctypes.pointer(d), G=1, T=1, step0=0, x=b, y=b, scale=1.0,
              tau=ctypes.cast(tau, ctypes.c_void_p), params=b, adam_m=b, adam_v=b, lr=1e-3,
              beta1=0.9, beta2=0.999, adam_eps=1e-8, eps=None, seed=0,
              offset=ctypes.cast(off, ctypes.c_void_p), loss_out=None, ws=None, ws_bytes=0)
    kw.update(over)
    r = _lib.MfviFitReq(**kw)
    r._keep = (d, tau, off)
    return r


def test_mfvi_fit_argument_checks():
    from psvi.runtime import _lib

    lib = _lib.load()
    call = lambda r: lib.psvi_mfvi_fit(ctypes.byref(r), None)
    EINVAL, ENOSPC = -1, -2
    assert lib.psvi_mfvi_fit(None, None) == EINVAL
    bad = [dict(desc=None), dict(dims=[13, 1]), dict(dims=[13, 8, 8, 8, 8, 1]), dict(dims=[129, 8, 1]),
           dict(dims=[13, 65, 1]), dict(dims=[13, 8, 65, 1]), dict(dims=[13, 8, 2]),
           dict(dims=[0, 8, 1]), dict(M=0), dict(M=513), dict(S=0), dict(S=65),
           dict(prior_sd=0.0), dict(G=0), dict(G=17), dict(T=-1), dict(T=(1 << 20) + 1),
           dict(step0=-1), dict(step0=(1 << 30), T=1), dict(scale=0.0), dict(scale=float("nan")),
           dict(lr=0.0), dict(beta1=1.0), dict(beta2=0.0), dict(adam_eps=-1.0), dict(x=None),
           dict(y=None), dict(tau=None), dict(params=None), dict(adam_m=None), dict(adam_v=None),
           dict(offset=None), dict(tau0=0.0), dict(tau0=float("inf")), dict(off0=2)]
    for kw in bad:
        assert call(_req(**kw)) == EINVAL, kw
        assert lib.psvi_last_error()
    # the global placement needs its workspace: D = 90, H = 50 x 2
    assert call(_req(dims=[90, 50, 50, 1])) == EINVAL                       # ws NULL
    assert call(_req(dims=[90, 50, 50, 1], ws=ctypes.c_void_p(256), ws_bytes=8)) == ENOSPC
    # the corners of the accepted range pass the query
    out = (ctypes.c_int64 * 4)()
    r = _req(dims=[128, 64, 64, 64, 1], S=64, M=512)
    assert lib.psvi_mfvi_fit_query(r.desc, out) == 0 and list(out) == [0, 4 * 33282, 33282, 64 * 16641]
    r = _req()
    assert lib.psvi_mfvi_fit_query(r.desc, out) == 0 and list(out) == [1, 0, 6602, 4 * 3301]
    assert lib.psvi_mfvi_fit_query(r.desc, None) == EINVAL
    assert lib.psvi_mfvi_fit_query(None, out) == EINVAL


def test_runtime_query_placements():
    from psvi.runtime import mfvi_fit_query

    assert mfvi_fit_query(R.layer_table(13, 50, 2), 4, 128)["placement"] == "lds"
    assert mfvi_fit_query(R.layer_table(90, 50, 2), 4, 128)["placement"] == "global"
    assert mfvi_fit_query(R.layer_table(3, 4, 1), 3, 5) == dict(
        placement="lds", ws_bytes=0, param_count=42, eps_count=63)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the refusals without a device")
def test_baselines_raise_without_gpu():
    from psvi.experiments import read_regression_dataset
    from psvi.inference.baselines import fit, run_mfvi_regressor, run_mfvi_subset_regressor

    d = read_regression_dataset("synth_regr", dict(synth_regr_n=60))
    kw = dict(mc_samples=2, data_minibatch=16, num_epochs=1, D=d[7], n_hidden=4,
              train_dataset=d[8], val_dataset=d[9], test_dataset=d[10], y_mean=d[11], y_std=d[12],
              taus=d[13])
    for fn in (lambda: run_mfvi_regressor(**kw), lambda: run_mfvi_subset_regressor(num_pseudo=8, **kw),
               lambda: fit(lr=1e-3)):
        with pytest.raises(RuntimeError, match="no HIP device"):
            fn()


def test_regression_datasets(tmp_path):
    from psvi.experiments import (hyperparams_for_regression, read_regression_dataset,
                                  update_hyperparams_dict)

    grids = hyperparams_for_regression()
    assert grids["boston"] == [0.1, 0.15, 0.2] and grids["kin8nm"] == [150, 200, 250]
    assert set(grids) >= {"concrete", "energy", "power", "kin8nm", "protein", "naval", "yacht",
                          "boston", "wine", "year", "synth_regr"}
    for dnm in ("boston", "concrete"):
        with pytest.raises(NotImplementedError, match="offline"):
            read_regression_dataset(dnm, dict(seed=42, num_test=0.15, data_folder=str(tmp_path)))
    args = dict(seed=42, num_test=0.15, synth_regr_n=200, synth_regr_d=5)
    out = read_regression_dataset("synth_regr", args)
    assert len(out) == 14
    x, y, xv, yv, xt, yt, N, D, tr, va, te, y_mean, y_std, taus = out
    assert (N, D) == x.shape == (150, 5) and y.shape == (150, 1)
    assert len(xv) == 20 and len(xt) == 30 and taus == grids["synth_regr"]
    assert tr.data.dtype == torch.float32 and tr.targets.shape == (150, 1)
    assert torch.allclose(tr.data.mean(0), torch.zeros(5), atol=1e-5)
    assert torch.allclose(tr.data.std(0, unbiased=False), torch.ones(5), atol=1e-4)
    assert abs(float(tr.targets.mean())) < 1e-5
    assert abs(float(tr.targets.std(unbiased=False)) - 1) < 1e-4
    # validation / test targets stay in original units, inputs use the training statistics
    assert np.allclose(te.targets.numpy(), yt.astype(np.float32))
    assert np.allclose(va.data.numpy(), ((xv - x.mean(0)) / x.std(0)).astype(np.float32))
    assert float(y_mean) == pytest.approx(y.mean()) and float(y_std) == pytest.approx(y.std())
    again = read_regression_dataset("synth_regr", args)
    assert np.array_equal(again[0], x) and np.array_equal(again[4], xt)
    # a local file of a UCI name is read
    rs = np.random.RandomState(0)
    np.savetxt(tmp_path / "housing.data", rs.randn(40, 14))
    b = read_regression_dataset("boston", dict(seed=1, num_test=0.15, data_folder=str(tmp_path)))
    assert b[7] == 13 and b[13] == grids["boston"]
    got = update_hyperparams_dict("boston", 0.15, results_folder=str(tmp_path / "res"))
    got = update_hyperparams_dict("yacht", 0.5, results_folder=str(tmp_path / "res"))
    assert got == {"boston": 0.15, "yacht": 0.5}
    assert (tmp_path / "res" / "opt_regr_hyperparams.json").exists()


def test_driver_tables():
    from psvi.experiments import inf_dict, regressor_experiment_driver, regressor_inf_dict

    assert sorted(regressor_inf_dict) == ["mfvi_regressor", "mfvi_subset_regressor",
                                          "psvi_alpha_v_regressor", "psvi_learn_v_regressor",
                                          "psvi_regressor"]
    assert sorted(inf_dict) == ["mfvi", "mfvi_subset", "opsvi", "psvi", "psvi_ablated",
                                "psvi_alpha_fixed_u", "psvi_alpha_v", "psvi_fixed_u",
                                "psvi_free_v", "psvi_learn_v", "psvi_no_iw", "psvi_no_rescaling",
                                "random", "sparsebbvi", "sparsevi"]
    with pytest.raises(NotImplementedError):
        regressor_experiment_driver(["synth_regr"], ["giga"], dict(num_trials=1), write=False)
