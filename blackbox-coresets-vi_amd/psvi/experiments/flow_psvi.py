"""flow_psvi.experiment_driver (psvi/experiments/flow_psvi.py:357-454) over the
methods the HIP path runs: the PSVI variants' run_psvi, the MFVI baselines,
the sparse black-box VI coreset construction and, from the extended driver
(psvi_experiments.py), the MFVI selection by predictive scores.  No CLI: method_args is the reference's dict of parsed arguments.

Multi-GPU (one process per GPU): every rank calls
experiment_driver with the same arguments and its ``world`` / ``rank`` (or
``method_args["world"]`` / ``["rank"]``) and, optionally, a collective
backend ``comm`` (psvi.runtime.sharded: TorchDistComm over RCCL by default,
HostStagedComm for gloo).  The PSVI methods then split their MC samples over
the ranks (the objectives, HVPs and trainers all-reduce the ranks' shares:
every rank holds the same u, v and network after every step); the MFVI
baselines have no sample-sharded form and run whole on every rank.  Rank 0
alone writes the results files."""
from ..inference import (PSVI, PSVIAV, PSVIAFixedU, PSVIFixedU, PSVIFreeV, PSVILearnV,
                         PSVI_Ablated, PSVI_No_IW, PSVI_No_Rescaling, PSVI_regressor,
                         PSVIAV_regressor, PSVILearnV_regressor, run_mfvi, run_mfvi_regressor,
                         run_mfvi_subset, run_mfvi_subset_regressor, run_opsvi, run_random,
                         run_selection_with_mfvi, run_sparsevi, run_sparsevi_with_bb_elbo)
from .experiments_utils import read_dataset, read_regression_dataset, rec_dd, write_to_files


def _psvi(cls):
    return lambda *a, **kw: cls(*a, **kw).run_psvi(*a, **kw)


# flow_psvi.py:306-354.  The regression variants have their own table and
# driver below (regressor_inf_dict, regressor_experiment_driver).  Not wired
# here: giga (psvi.inference.run_giga runs on the HIP path; call it directly).  sparsebbvi runs on it
# (Bernoulli plans, one output), and so do the Laplace baselines random,
# sparsevi and opsvi (psvi_laplace_fit, psvi_laplace_scores).
inf_dict = {
    "psvi": _psvi(PSVI),
    "psvi_ablated": _psvi(PSVI_Ablated),
    "psvi_learn_v": _psvi(PSVILearnV),
    "psvi_alpha_v": _psvi(PSVIAV),
    "psvi_no_iw": _psvi(PSVI_No_IW),
    "psvi_free_v": _psvi(PSVIFreeV),
    "psvi_no_rescaling": _psvi(PSVI_No_Rescaling),
    "psvi_fixed_u": _psvi(PSVIFixedU),
    "psvi_alpha_fixed_u": _psvi(PSVIAFixedU),
    "mfvi": run_mfvi,
    "mfvi_subset": run_mfvi_subset,
    "sparsebbvi": run_sparsevi_with_bb_elbo,
    "random": run_random,
    "sparsevi": run_sparsevi,
    "opsvi": run_opsvi,
}


# psvi_experiments.py:430-460, the extended driver's additions to that table
# that run on the HIP path (its "el2n" does not: ten-seed score files nothing
# writes).  "mfvi_selection" with a k-means method -- "kmeans" is the default --
# runs when method_args["clustering"] == "hip" (psvi_kmeans on the device in
# place of sklearn) and is refused without it.  A table of its own: inf_dict is flow_psvi.py's, and
# tests/test_giga_cpu.py and tests/test_mfvi_regr_cpu.py pin its keys.
# experiment_driver looks a method up in both.
extended_inf_dict = {
    "mfvi_selection": run_selection_with_mfvi,
}


def experiment_driver(datasets, methods, method_args, write=True, world=None, rank=None,
                      comm=None):
    """For each dataset, method, trial and coreset size: run the method with
    the reference's keyword set and store its results dict at
    results[dataset][method][size][trial]; coreset-free methods use size -1.
    world / rank / comm: this process's place in a multi-GPU run (above)."""
    world = int(method_args.get("world", 1) if world is None else world)
    rank = int(method_args.get("rank", 0) if rank is None else rank)
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside world {world}")
    shard = dict(world=world, rank=rank, comm=comm) if world > 1 else {}
    results = rec_dd()
    for dnm in datasets:
        x, y, xt, yt, N, D, train_dataset, test_dataset, nc = read_dataset(dnm, method_args)
        for nm_alg in methods:
            if nm_alg not in inf_dict and nm_alg not in extended_inf_dict:
                raise NotImplementedError(f"method {nm_alg!r} is not on the HIP path")
            inf_alg = inf_dict.get(nm_alg) or extended_inf_dict[nm_alg]
            logistic_regression = method_args.get(
                "logistic_regression", method_args.get("architecture") == "logreg")
            compute_weights_entropy = (not nm_alg.startswith(("opsvi", "mfvi_subset"))
                                       and method_args.get("compute_weights_entropy", True))
            sizes = (method_args["coreset_sizes"]
                     if nm_alg.startswith(("psvi", "opsvi", "mfvi_subset", "mfvi_selection"))
                     else [-1])
            extra = dict(shard) if nm_alg.startswith("psvi") else {}
            if nm_alg == "mfvi_selection":
                # psvi_experiments.py:558-566, with its parser's defaults
                extra.update(
                    mfvi_selection_method=method_args.get("mfvi_selection_method", "kmeans"),
                    pretrain_epochs=method_args.get("pretrain_epochs", 5),
                    data_folder=method_args.get("data_folder"),
                    load_from_saved=method_args.get("load_from_saved", False),
                    loaded_from_psvi=method_args.get("loaded_from_psvi", True),
                    clustering=method_args.get("clustering"))
            if nm_alg.startswith("psvi"):
                # flow_psvi.py's continual-learning arguments; absent: off, as before
                extra.update({k: method_args.get(k, False)
                              for k in ("prune", "increment", "reset", "retrain_on_coreset")})
                extra.update({k: method_args.get(k)
                              for k in ("prune_interval", "prune_sizes", "increment_interval",
                                        "increment_sizes")})
                extra.update(reset_interval=method_args.get("reset_interval", 10),
                             lr0joint=method_args.get("lr0joint", 1e-3))
            for t in range(method_args["num_trials"]):
                for ps in sizes:
                    results[dnm][nm_alg][ps][t] = inf_alg(
                        **extra,
                        mc_samples=method_args["mc_samples"],
                        num_epochs=method_args["num_epochs"],
                        data_minibatch=method_args["data_minibatch"],
                        D=D, N=N, tr=t, x=x, y=y, xt=xt, yt=yt,
                        inner_it=method_args["inner_it"],
                        logistic_regression=logistic_regression,
                        trainer=method_args["trainer"],
                        log_every=method_args["log_every"],
                        register_elbos=method_args.get("register_elbos", False),
                        lr0u=method_args["lr0u"], lr0net=method_args["lr0net"],
                        lr0v=method_args["lr0v"], lr0z=method_args.get("lr0z", 1e-2),
                        lr0alpha=method_args.get("lr0alpha", 1e-3),
                        init_args=method_args.get("init_at", "subsample"),
                        init_sd=method_args["init_sd"], num_pseudo=ps, seed=t,
                        compute_weights_entropy=compute_weights_entropy,
                        architecture=method_args.get("architecture"),
                        log_pseudodata=method_args.get("log_pseudodata", False),
                        n_hidden=method_args.get("n_hidden", 40),
                        n_layers=method_args.get("n_layers", 1),
                        train_dataset=train_dataset, test_dataset=test_dataset, dnm=dnm, nc=nc,
                        learn_z=method_args.get("learn_z", False),
                        **(dict(outer_it=method_args["outer_it"], scatterplot_coreset=False)
                           if nm_alg == "sparsebbvi" else {}),
                        **(dict(outer_it=method_args["outer_it"])
                           if nm_alg == "sparsevi" else {}))
    if write and rank == 0:
        return write_to_files(results, method_args.get("fnm", "results"),
                              method_args.get("results_folder", "results"))
    return results


# flow_psvi.py:336-353: the regression methods, looked up as nm_alg + "_regressor"
regressor_inf_dict = {
    "psvi_regressor": _psvi(PSVI_regressor),
    "psvi_learn_v_regressor": _psvi(PSVILearnV_regressor),
    "psvi_alpha_v_regressor": _psvi(PSVIAV_regressor),
    "mfvi_regressor": run_mfvi_regressor,
    "mfvi_subset_regressor": run_mfvi_subset_regressor,
}


def regressor_experiment_driver(datasets, methods, method_args, write=True):
    """flow_psvi.regressor_experiment_driver (flow_psvi.py:459-549): BNN
    regression over read_regression_dataset's sets ("synth_regr", or a UCI set
    read from method_args["data_folder"]).  methods name the algorithms without
    the suffix ("psvi", "psvi_learn_v", "psvi_alpha_v", "mfvi", "mfvi_subset");
    results[dataset][method][size][trial].  As in the reference the dataset's
    split uses seed 42 and num_test 0.15, the architecture is 'regressor_net'
    and the PSVI regressors run at their own tau (method_args["tau"], default
    0.1) while the MFVI baselines search the dataset's tau grid."""
    results = rec_dd()
    for dnm in datasets:
        method_args["seed"], method_args["num_test"] = 42, .15
        (x, y, xv, yv, xt, yt, N, D, train_dataset, val_dataset, test_dataset, y_mean, y_std,
         taus) = read_regression_dataset(dnm, method_args)
        for nm_alg in methods:
            if nm_alg + "_regressor" not in regressor_inf_dict:
                raise NotImplementedError(f"method {nm_alg!r} has no regression form on the "
                                          "HIP path")
            inf_alg = regressor_inf_dict[nm_alg + "_regressor"]
            compute_weights_entropy = (not nm_alg.startswith("mfvi_subset")
                                       and method_args.get("compute_weights_entropy", True))
            sizes = (method_args["coreset_sizes"]
                     if nm_alg.startswith(("psvi", "mfvi_subset")) else [-1])
            extra = dict(tau=method_args["tau"]) if (
                nm_alg.startswith("psvi") and "tau" in method_args) else {}
            for t in range(method_args["num_trials"]):
                for ps in sizes:
                    results[dnm][nm_alg][ps][t] = inf_alg(
                        **extra,
                        mc_samples=method_args["mc_samples"],
                        num_epochs=method_args["num_epochs"],
                        data_minibatch=method_args["data_minibatch"],
                        D=D, N=N, tr=t, x=x, y=y, xv=xv, yv=yv, xt=xt, yt=yt,
                        inner_it=method_args["inner_it"],
                        logistic_regression=False,
                        trainer=method_args["trainer"],
                        log_every=method_args["log_every"],
                        register_elbos=method_args.get("register_elbos", False),
                        lr0u=method_args["lr0u"], lr0net=method_args["lr0net"],
                        lr0v=method_args["lr0v"],
                        init_args=method_args.get("init_at", "subsample"),
                        init_sd=method_args["init_sd"], num_pseudo=ps, seed=t,
                        compute_weights_entropy=compute_weights_entropy,
                        architecture=method_args.get("architecture", "regressor_net"),
                        log_pseudodata=method_args.get("log_pseudodata", False),
                        n_hidden=method_args.get("n_hidden", 40),
                        n_layers=method_args.get("n_layers", 1),
                        train_dataset=train_dataset, val_dataset=val_dataset,
                        test_dataset=test_dataset, dnm=dnm, y_mean=y_mean, y_std=y_std,
                        taus=taus, results_folder=method_args.get("results_folder", "results"))
    if write:
        return write_to_files(results, method_args.get("fnm", "results"),
                              method_args.get("results_folder", "results"))
    return results
