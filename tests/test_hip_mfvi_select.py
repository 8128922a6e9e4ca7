"""MFVI selection by predictive scores through the public classes, replaying the
reference's own runs (fixtures z1-z3, tools/gen_golden_mfvi_select.py) with its
recorded noise injected by ``eps_source``: parameters and elbos within the
project's parity bound (1e-4 relative), the forgetting state and the chosen
indices exactly (the generator asserts their margins); then seeded end-to-end
runs of run_selection_with_mfvi and of experiment_driver."""
import numpy as np
import pytest
import torch
from torch.nn.utils import parameters_to_vector

import mfvi_select_util as R
from golden_util import load_fixture, rel

pytestmark = pytest.mark.gpu


class _Stream:
    def __init__(self, flat):
        self.flat, self.o = torch.tensor(flat), 0

    def take(self, n):
        out = self.flat[self.o:self.o + n]
        assert out.numel() == n, "draw stream exhausted"
        self.o += n
        return out


class _Rows(torch.utils.data.Dataset):
    def __init__(self, x, y):
        self.data, self.targets = torch.as_tensor(x), torch.as_tensor(y)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


def _flat(net):
    return parameters_to_vector(net.parameters()).detach().cpu().numpy()


def test_meanfieldvi_replays_reference_forgetting_run():
    from psvi.inference.utils import MeanFieldVI

    f = load_fixture("z2_forgetting")
    c, st = f["cfg"], _Stream(f["draws"])
    vi = MeanFieldVI(mc_samples=c["S"], data_minibatch=c["data_minibatch"],
                     num_epochs=c["num_epochs"], log_every=c["log_every"], N=len(f["x"]), D=c["D"],
                     lr0net=c["lr"], mul_fact=1, seed=c["seed"], architecture="fn",
                     n_hidden=c["n_hidden"], nc=c["nc"], train_dataset=_Rows(f["x"], f["y"]),
                     test_dataset=_Rows(f["xt"], f["yt"]), init_sd=c["init_sd"],
                     forgetting_score_flag=True, eps_source=st.take)
    vi.before_train()
    assert np.array_equal(_flat(vi.net), f["params0"])  # the same seeded initialisation
    vi.run()
    assert st.o == st.flat.numel()
    assert rel(vi.elbos_mfvi, f["elbos"]) < 1e-4
    assert rel(_flat(vi.net), f["params"]) < 1e-4
    assert np.array_equal(vi.last_acc.cpu().numpy(), f["last_acc"])
    assert np.array_equal(vi.forgetting_events.cpu().numpy(), f["forgetting"])
    assert np.array_equal(vi.never_learnt_events.cpu().numpy(), f["never_learnt"])
    nt = len(f["yt"])
    assert np.array_equal(np.round(np.array(vi.accs_mfvi) * nt), np.round(f["accs"] * nt))
    assert np.allclose(vi.nlls_mfvi, f["nlls"], rtol=1e-4)


def test_evaluate_coreset_replays_reference():
    from psvi.inference.baselines import MfviSelect
    from psvi.inference.utils import WeightedSubset

    f = load_fixture("z3_evaluate")
    c, st = f["cfg"], _Stream(f["draws"])
    train = _Rows(f["x"], f["y"])
    ms = MfviSelect(train_dataset=train, test_dataset=_Rows(f["xt"], f["yt"]),
                    data_minibatch=c["data_minibatch"], num_pseudo=c["num_pseudo"], nc=c["nc"],
                    architecture="fn", D=c["D"], n_hidden=c["n_hidden"], mc_samples=c["S"],
                    init_sd=c["init_sd"], lr0net=c["lr"], num_epochs=c["num_epochs"],
                    log_every=c["log_every"], seed=c["seed"], mul_fact=1, score_method="entropy",
                    eps_source=st.take)
    assert np.array_equal(_flat(ms.net), f["params0"])
    ms.chosen_dataset = WeightedSubset(train, f["chosen"].tolist(), torch.tensor(f["weights"]))
    ms.wt_index = {}
    res = ms.evaluate_coreset()
    assert st.o == st.flat.numel()
    assert rel(res["elbos"], f["elbos"]) < 1e-4
    assert rel(_flat(ms.net), f["params"]) < 1e-4
    nt = len(f["yt"])
    assert np.array_equal(np.round(np.array(res["accs"]) * nt), np.round(f["accs"] * nt))
    assert np.allclose(res["nlls"], f["nlls"], rtol=1e-4)
    assert res["times"] == 0 and res["csizes"] == [c["num_pseudo"]] * c["num_epochs"]


def test_evaluate_coreset_accumulates_gradients_across_batches():
    """130 chosen rows are two batches (128 + 2) under ONE zero_grad per
    iteration: the second step of an iteration takes the sum of both batches'
    gradients.  Against torch.optim.Adam driven that way on the library's own
    per-batch gradients (psvi_elbo_grad at the parameters of the moment, the
    same noise); a run that zeroes before every step ends elsewhere."""
    from psvi.inference.baselines import MfviSelect
    from psvi.inference.utils import WeightedSubset
    from psvi.models import model_spec
    from psvi.runtime import InnerLoopPlan

    g = torch.Generator().manual_seed(5)
    n, D, nc, H, S, iters = 160, 4, 3, 6, 3, 3
    x = torch.randn(n, D, generator=g)
    train = _Rows(x, (x @ torch.randn(D, nc, generator=g)).argmax(1).float())
    chosen = torch.randperm(n, generator=g)[:130].tolist()
    wts = (n / 130.0) * (1.0 + 0.01 * torch.arange(130.0))
    noise = torch.randn(200000, generator=g)

    def select(stream):
        ms = MfviSelect(train_dataset=train, test_dataset=_Rows(x[:8], train.targets[:8]),
                        data_minibatch=64, num_pseudo=130, nc=nc, architecture="fn", D=D,
                        n_hidden=H, mc_samples=S, init_sd=0.3, lr0net=0.02, num_epochs=iters,
                        log_every=100, seed=0, mul_fact=1, score_method="entropy",
                        eps_source=stream.take)
        ms.chosen_dataset, ms.wt_index = WeightedSubset(train, chosen, wts), {}
        return ms

    ms = select(_Stream(noise.numpy()))
    p0 = torch.tensor(_flat(ms.net), device="cuda")
    fam, layers, sd, _ = model_spec(ms.net)
    # iteration 0 tests once (one draw after its two steps); no other test runs
    st = _Stream(noise.numpy())
    plans = {B: InnerLoopPlan(fam, layers, S, B, prior_sd=sd) for B in (128, 2)}
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], 0.02)
    xs, ys = x[chosen].cuda(), train.targets[chosen].to(torch.int32).cuda()
    want_elbos = []
    for it in range(iters):
        opt.zero_grad()
        for lo, B in ((0, 128), (128, 2)):
            eps = st.take(plans[B].eps_count).cuda().contiguous()
            loss, grad = plans[B].elbo_grad(xs[lo:lo + B].contiguous(), ys[lo:lo + B].contiguous(),
                                            wts[lo:lo + B].cuda().contiguous(), eps,
                                            p.detach().contiguous())
            p.grad = grad if p.grad is None else p.grad + grad
            opt.step()
        want_elbos.append(-loss.item())
        if it == 0:
            st.take(plans[2].eps_count)  # the test's draw
    res = ms.evaluate_coreset()
    assert rel(res["elbos"], want_elbos) < 1e-4
    assert rel(_flat(ms.net), p.detach().cpu().numpy()) < 1e-4
    # zeroing before every step (what a per-step zero_grad would do) is another run
    q = p0.clone().requires_grad_(True)
    opt, st = torch.optim.Adam([q], 0.02), _Stream(noise.numpy())
    for it in range(iters):
        for lo, B in ((0, 128), (128, 2)):
            eps = st.take(plans[B].eps_count).cuda().contiguous()
            _, q.grad = plans[B].elbo_grad(xs[lo:lo + B].contiguous(), ys[lo:lo + B].contiguous(),
                                           wts[lo:lo + B].cuda().contiguous(), eps,
                                           q.detach().contiguous())
            opt.step()
        if it == 0:
            st.take(plans[2].eps_count)
    # ... by more than ten times the bound the accumulating run is matched to
    assert rel(_flat(ms.net), q.detach().cpu().numpy()) > 1e-3


@pytest.mark.parametrize("st", ["least_confidence", "entropy"])
def test_score_selection_picks_the_reference_rows(st, tmp_path):
    from psvi.inference.baselines import set_up_model
    from psvi.inference.utils import ScoreSelection

    f = load_fixture("z1_scores")
    c = f["cfg"]
    net = set_up_model(architecture="fn", D=c["layers"][0][0], n_hidden=c["layers"][0][1],
                       nc=c["nc"], mc_samples=c["S"])
    torch.nn.utils.vector_to_parameters(torch.tensor(f["params"]), list(net.parameters()))
    stream = _Stream(np.concatenate((f["eps_" + st], f["eps_select_" + st])))
    sel = ScoreSelection(_Rows(f["x"], f["y"]), c["num_pseudo"], c["nc"], 0, score_type=st,
                         data_folder=str(tmp_path), dnm="toy", loaded=False, eps_source=stream.take)
    sel.pretrained_net = net
    score = sel._get_uncertainty_score().numpy().astype(np.float64)
    cap = 1.0 if st == "least_confidence" else np.log(c["nc"])
    assert (np.abs(score - f["score_" + st]) <= 1e-4 * np.abs(f["score_" + st]) + 1e-4 * cap).all()
    assert sel.select() == f["select_" + st].tolist()
    assert stream.o == stream.flat.numel()
    assert (tmp_path / f"{st}_toy_10_0.csv").exists()


@pytest.mark.parametrize("method", ["least_confidence", "entropy", "el2n", "forgetting"])
def test_run_selection_end_to_end(method):
    from psvi.experiments import read_dataset
    from psvi.inference.baselines import run_selection_with_mfvi

    x, y, xt, yt, N, D, train, test, nc = read_dataset("four_blobs", dict(test_ratio=0.2))
    num_pseudo = 10
    res = run_selection_with_mfvi(
        x=x, y=y, xt=xt, yt=yt, mc_samples=4, data_minibatch=128, num_epochs=3, log_every=2, D=D,
        lr0net=1e-2, mul_fact=1, seed=1, train_dataset=train, test_dataset=test,
        num_pseudo=num_pseudo, architecture="fn", n_hidden=8, nc=nc, dnm="four_blobs",
        init_sd=1e-2, mfvi_selection_method=method, pretrain_epochs=1, loaded_from_psvi=False)
    assert sorted(res) == ["accs", "csizes", "elbos", "nlls", "times", "wt_index"]
    idx = [int(k) for k in res["wt_index"]]
    assert len(set(idx)) == num_pseudo
    ty = np.asarray(train.targets)
    assert [int((ty[idx] == c).sum()) for c in range(nc)] == R.class_split(num_pseudo, nc)
    assert np.allclose(list(res["wt_index"].values()), len(train) / num_pseudo)
    assert len(res["elbos"]) == 3 and np.isfinite(res["elbos"]).all()
    assert len(res["accs"]) == 1 and 0.0 <= res["accs"][0] <= 1.0 and np.isfinite(res["nlls"][0])
    assert res["times"] == 0 and res["csizes"] == [num_pseudo] * 3


def test_experiment_driver_runs_mfvi_selection(tmp_path):
    from psvi.experiments import experiment_driver

    args = dict(mc_samples=4, num_epochs=2, data_minibatch=128, inner_it=2, trainer="nested",
                log_every=1, lr0u=1e-3, lr0net=1e-2, lr0v=1e-2, init_sd=1e-2,
                coreset_sizes=[8, 12], num_trials=1, test_ratio=0.2, architecture="fn",
                n_hidden=8, mfvi_selection_method="entropy", pretrain_epochs=1,
                loaded_from_psvi=False, fnm="sel", results_folder=str(tmp_path))
    res = experiment_driver(["four_blobs"], ["mfvi_selection"], args, write=False)
    for ps in (8, 12):
        r = res["four_blobs"]["mfvi_selection"][ps][0]
        assert len(r["wt_index"]) == ps and len(r["elbos"]) == 4
    with pytest.raises(NotImplementedError, match="k-means"):  # the parser's default method
        experiment_driver(["four_blobs"], ["mfvi_selection"],
                          {k: v for k, v in args.items() if k != "mfvi_selection_method"},
                          write=False)
