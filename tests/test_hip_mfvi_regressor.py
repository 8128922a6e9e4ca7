"""The MFVI regression baselines end to end on "synth_regr": the tau that
run_mfvi_regressor selects, its rmses / lls / elbos against the float64
restatement fed with the same noise, the subset variant and one pass of
regressor_experiment_driver."""
import os

import numpy as np
import pytest
import torch

import mfvi_regr_util as R

pytestmark = pytest.mark.gpu

TOL = 1e-4
TAUS = [0.01, 1.0, 100.0]
S, H, NL, MB, EPOCHS, SEED = 3, 6, 2, 64, 6, 3


def _data():
    from psvi.experiments import read_regression_dataset

    return read_regression_dataset("synth_regr", dict(seed=42, num_test=0.15, synth_regr_n=300))


def _restate(d, draws):
    """run_mfvi_regressor's sequence in float64: one fit per tau logged on the
    validation set, the strict > rule, the final fit logged on the test set."""
    from psvi.models import make_regressor_net

    tr, va, te, y_mean, y_std = d[8], d[9], d[10], float(d[11]), float(d[12])
    D, n_train = d[7], len(d[8])
    layers = R.layer_table(D, H, NL)
    P, E = R.counts(layers, S)
    T = EPOCHS * max(1, int(n_train / MB))
    x, y = tr.data[:MB].numpy(), tr.targets[:MB, 0].numpy()
    torch.manual_seed(SEED)
    it = iter(draws)

    def one(tau, pred):
        net = make_regressor_net(D, H, 1, n_layers=NL, mc_samples=S, init_sd=0.05)
        p0 = torch.nn.utils.parameters_to_vector(net.parameters()).detach().numpy()
        eps = np.stack([next(it) for _ in range(T)])
        L, p, _, _ = R.fit(layers, S, x, y, n_train / MB, tau, p0, eps, 1e-2)
        se = sl = 0.0
        for b in range(0, len(pred), MB):
            yt = pred.targets[b:b + MB, 0].numpy()
            r, l = R.predict(layers, p, next(it), S, pred.data[b:b + MB].numpy(), yt, tau, y_mean,
                             y_std)
            se, sl = se + r * r * len(yt), sl + l * len(yt)
        return L, float(np.sqrt(se / len(pred))), sl / len(pred)

    best_tau, best_ll, val = TAUS[0], -float("inf"), []
    for tau in TAUS:
        _, _, ll = one(tau, va)
        val.append(ll)
        if ll > best_ll:
            best_tau, best_ll = tau, ll
    return best_tau, val, one(best_tau, te)


def test_model_selection_matches_restatement():
    from psvi.inference.baselines import run_mfvi_regressor

    d = _data()
    E = R.counts(R.layer_table(d[7], H, NL), S)[1]
    rng = np.random.default_rng(11)
    draws = []

    def eps_source(n):
        out = rng.standard_normal(n).astype(np.float32)
        draws.extend(out.reshape(-1, E))
        return torch.from_numpy(out)

    res = run_mfvi_regressor(mc_samples=S, data_minibatch=MB, num_epochs=EPOCHS, log_every=-1,
                             D=d[7], lr0net=1e-2, seed=SEED, n_hidden=H, n_layers=NL,
                             train_dataset=d[8], val_dataset=d[9], test_dataset=d[10],
                             y_mean=d[11], y_std=d[12], taus=TAUS, init_sd=0.05,
                             model_selection=True, eps_source=eps_source)
    best_tau, val, (L, rmse, ll) = _restate(d, draws)
    print(f"validation lls {val} -> tau {best_tau}; test rmse {rmse} ll {ll}; "
          f"device rmse {res['rmses']} ll {res['lls']}")
    # no near tie: the candidates' validation log-likelihoods are far apart
    top = sorted(val)
    assert top[-1] - top[-2] > 1e3 * TOL * abs(top[-1])
    assert res["scale"] == pytest.approx(1.0 / np.sqrt(best_tau))
    assert len(res["rmses"]) == len(res["lls"]) == len(res["times"]) == 1
    assert len(res["elbos"]) == len(L)
    assert np.abs(np.array(res["elbos"]) + L).max() < TOL * np.abs(L).max()
    assert abs(res["rmses"][0] - rmse) < TOL * abs(rmse)
    assert abs(res["lls"][0] - ll) < TOL * abs(ll)


def test_subset_and_driver(tmp_path):
    from psvi.experiments import regressor_experiment_driver
    from psvi.inference.baselines import run_mfvi_subset_regressor

    d = _data()
    res = run_mfvi_subset_regressor(mc_samples=S, data_minibatch=MB, num_epochs=2, log_every=3,
                                    D=d[7], lr0net=1e-2, seed=1, n_hidden=H, train_dataset=d[8],
                                    val_dataset=d[9], test_dataset=d[10], y_mean=d[11],
                                    y_std=d[12], taus=TAUS, num_pseudo=20)
    T = 2 * (len(d[8]) // MB)
    assert res["csizes"] == [20] and len(res["elbos"]) == T
    assert len(res["rmses"]) == len(range(0, T, 3)) and np.isfinite(res["lls"]).all()
    args = dict(mc_samples=S, num_epochs=2, data_minibatch=MB, inner_it=2, trainer="nested",
                log_every=1, lr0u=1e-3, lr0net=1e-2, lr0v=1e-2, init_sd=0.05, coreset_sizes=[5],
                num_trials=1, n_hidden=H, n_layers=NL, synth_regr_n=300, fnm="regr",
                results_folder=str(tmp_path))
    out = regressor_experiment_driver(["synth_regr"], ["mfvi", "psvi"], args)
    assert os.path.exists(tmp_path / "regr.json") and os.path.exists(tmp_path / "regr.pk")
    assert os.path.exists(tmp_path / "opt_regr_hyperparams.json")
    assert len(out["synth_regr"]["mfvi"]["-1"]["0"]["rmses"]) >= 1
    assert len(out["synth_regr"]["psvi"]["5"]["0"]["rmses"]) == 2
