"""run_psvi's pruning, incremental tasks, resets and retraining on the HIP path
(psvi_classes.py:823-832, 928-1003, 1110-1128, 1177-1217): tiny runs on the
offline datasets, called as flow_psvi's inf_dict does."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

_DATA = {}


def dataset(dnm):
    """read_dataset's (N, D, train, test, nc), built once per session."""
    if dnm not in _DATA:
        from psvi.experiments.experiments_utils import read_dataset

        torch.manual_seed(1234)     # four_blobs is drawn from torch's generator
        _, _, _, _, N, D, tr, te, nc = read_dataset(dnm, dict(test_ratio=0.2))
        _DATA[dnm] = (N, D, tr, te, nc)
    return _DATA[dnm]


def kwargs(dnm, **over):
    N, D, tr, te, nc = dataset(dnm)
    kw = dict(mc_samples=4, num_epochs=7, data_minibatch=64, D=D, N=N, inner_it=2,
              logistic_regression=True, trainer="nested", log_every=1, register_elbos=False,
              lr0u=1e-3, lr0net=1e-3, lr0v=1e-2, lr0alpha=1e-3, lr0joint=1e-3,
              init_args="subsample", init_sd=1e-2, num_pseudo=8, seed=0, architecture=None,
              n_hidden=8, n_layers=1, train_dataset=tr, test_dataset=te, dnm=dnm, nc=nc,
              device_id=0)
    kw.update(over)
    return kw


def arch_kw(arch):
    return dict(logistic_regression=arch == "logreg", architecture=None if arch == "logreg" else arch)


def finite(res):
    return (all(math.isfinite(x) for x in res["nlls"]) and all(0.0 <= a <= 1.0 for a in res["accs"])
            and all(np.isfinite(v).all() for v in res["vs"]))


def pvec(ps):
    return nn.utils.parameters_to_vector(ps.model.parameters()).detach().clone()


def rows_of(a, b):
    """Every row of a is bitwise a row of b."""
    a = a.detach().cpu().reshape(a.shape[0], -1).view(torch.int32)
    b = b.detach().cpu().reshape(b.shape[0], -1).view(torch.int32)
    return all((b == r).all(1).any() for r in a)


def run_prune(seed, arch="logreg"):
    from psvi.inference import PSVIAFixedU

    kw = kwargs("halfmoon", seed=seed, prune=True, prune_sizes=[6, 4], prune_interval=2,
                **arch_kw(arch))
    ps = PSVIAFixedU(**kw)
    first_u, orig = [], ps.prune_coreset

    def hooked(**a):
        first_u.append(ps.u.detach().clone())
        return orig(**a)

    ps.prune_coreset = hooked
    return ps, ps.run_psvi(**kw), first_u[0]


@pytest.mark.parametrize("arch", ["logreg", "fn"])
def test_prune(arch):
    ps, res, u0 = run_prune(0, arch)
    assert res["csizes"] == [8, 8, 8, 6, 6, 4, 4]        # pruned after steps 2 and 4
    assert ps.num_pseudo == 4 and tuple(ps.u.shape) == (4, 2) and ps.v.numel() == 4
    assert ps.z.numel() == 4 and [v.shape[0] for v in res["vs"]] == res["csizes"]
    assert u0.shape[0] == 8 and rows_of(ps.u, u0)
    assert [(k, it, tuple(i.shape)) for k, it, i in ps.draw_log] == [("prune", 2, (6,)),
                                                                    ("prune", 4, (4,))]
    assert all(i.unique().numel() == i.numel() for _, _, i in ps.draw_log)
    assert finite(res)


@pytest.mark.parametrize("init_args", ["random", "subsample"])
def test_increment(init_args):
    from psvi.inference import PSVIAV

    sizes = [4, 6, 8]
    kw = kwargs("four_blobs", increment=True, increment_sizes=sizes, increment_interval=2,
                init_args=init_args)
    ps = PSVIAV(**kw)
    assert ps.num_pseudo == 4
    seen, orig = [], ps._increment_task

    def hooked(idx, *a):
        before = dict(u=ps.u.detach().clone(), so_far=ps.train_data_so_far, M=ps.num_pseudo,
                      optims=(ps.optim_v, ps.optim_u, ps.optim_net, ps.optim_alpha))
        orig(idx, *a)
        seen.append((idx, before))
        task_len = len(ps.incremental_train_datasets[idx])
        data = ps.train_loader.dataset
        assert ps.nc == idx + 2 and ps.model[-1].out_features == ps.nc
        assert ps.num_pseudo == sizes[idx] == ps.u.shape[0] == ps.v.numel() == ps.z.numel()
        assert (ps.z[before["M"]:] == idx + 1).all()              # the new class's points
        assert len(data) == task_len + before["so_far"] == ps.train_data_so_far
        drawn = ps.draw_log[-1][2].long()
        assert drawn.numel() == before["so_far"] and int(drawn.max()) < before["M"]
        appended = torch.as_tensor(data.data[task_len:])
        assert rows_of(appended, before["u"])
        assert torch.equal(appended.view(torch.int32),
                           before["u"].cpu()[drawn].view(torch.int32))
        assert set(torch.as_tensor(data.targets[task_len:]).long().tolist()) <= set(range(idx + 1))
        assert all(new is not old for new, old in
                   zip((ps.optim_v, ps.optim_u, ps.optim_net, ps.optim_alpha), before["optims"]))
        assert set(ps.test_loader.dataset.targets.long().tolist()) == set(range(ps.nc))

    ps._increment_task = hooked
    res = ps.run_psvi(**kw)
    assert [i for i, _ in seen] == [1, 2] and ps.nc == 4
    assert res["csizes"] == [4, 4, 4, 6, 6, 8, 8]
    assert finite(res)


@pytest.mark.parametrize("arch", ["logreg", "fn"])
def test_reset(arch):
    from psvi.inference import PSVILearnV

    kw = kwargs("halfmoon", reset=True, reset_interval=3, **arch_kw(arch))
    ps = PSVILearnV(**kw)
    sds, orig = [], ps.weight_reset

    def hooked():
        orig()
        sds.append(torch.cat([nn.functional.softplus(p.detach()).reshape(-1)
                              for n, p in ps.model.named_parameters() if n.endswith("_sd")]))

    ps.weight_reset = hooked
    res = ps.run_psvi(**kw)
    assert len(sds) == 3                                         # before steps 0, 3 and 6
    # softplus(inverse_softplus(init_sd)) in fp32: a few ulp of 1e-2
    assert all(torch.allclose(s, torch.full_like(s, kw["init_sd"]), rtol=1e-5, atol=0) for s in sds)
    assert finite(res)


@pytest.mark.parametrize("arch", ["logreg", "fn"])
def test_retrain_equals_the_step_by_step_loop(arch):
    """retrain(T, lr) = weight_reset, then T steps of psvi_elbo_grad +
    psvi_adam_update (torch arithmetic) on the same Philox draws."""
    from psvi.inference import PSVIAFixedU
    from psvi.runtime import adam_update_, randn_

    kw = kwargs("halfmoon", num_epochs=2, log_every=2, **arch_kw(arch))
    ps = PSVIAFixedU(**kw)
    ps.run_psvi(**kw)
    T, lr, off0 = 5, 3e-3, ps._eps_offset
    torch.manual_seed(99)
    ps.retrain(T, lr)                       # chunks of log_every = 2: 2 + 2 + 1 steps
    got = pvec(ps)
    plan = ps._plan(ps.model)
    assert ps._eps_offset == off0 + T * plan.eps_stride
    torch.manual_seed(99)
    ps.weight_reset()
    p = pvec(ps).to(torch.float32)
    assert not torch.equal(p, got)
    u, z, w = ps._data(plan)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    eps = torch.empty(plan.eps_count, device=p.device)
    for t in range(T):
        randn_(eps, ps.seed, off0 + t * plan.eps_stride)
        _, g = plan.elbo_grad(u, z, w, eps, p)
        adam_update_(p, g, m, v, t + 1, lr, kind="torch")
    err = float((got - p).abs().max() / p.abs().max())
    print(f"retrain vs step-by-step ({arch}): max-norm relative {err:.2e}")
    assert err <= 1e-4


def test_retrain_on_coreset_doubles_the_evaluations():
    from psvi.inference import PSVIAFixedU

    kw = kwargs("halfmoon", num_epochs=4, log_every=2, retrain_on_coreset=True, lr0joint=2e-3)
    ps = PSVIAFixedU(**kw)
    res = ps.run_psvi(**kw)
    assert len(res["accs"]) == len(res["nlls"]) == len(res["csizes"]) == len(res["vs"]) == 4
    assert res["csizes"] == [8] * 4 and finite(res)
    fv = ps.f(ps.v, 0).detach().cpu().numpy()                   # the tail logs f(v), not v
    assert all(np.array_equal(v, fv) for v in res["vs"][2:])
    assert not np.array_equal(res["vs"][1], fv)
    plain = kwargs("halfmoon", num_epochs=4, log_every=2)
    assert len(PSVIAFixedU(**plain).run_psvi(**plain)["accs"]) == 2


def test_runs_are_functions_of_the_seed():
    a_ps, a, _ = run_prune(3)
    b_ps, b, _ = run_prune(3)
    for key in ("vs", "csizes", "accs", "nlls"):
        assert len(a[key]) == len(b[key])
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[key], b[key])), key
    assert all(torch.equal(x[2], y[2]) for x, y in zip(a_ps.draw_log, b_ps.draw_log))
    assert torch.equal(a_ps.u, b_ps.u) and a_ps._eps_offset == b_ps._eps_offset
    c_ps, _, _ = run_prune(4)
    assert not all(torch.equal(x[2], y[2]) for x, y in zip(a_ps.draw_log, c_ps.draw_log))
