#!/usr/bin/env python3
"""Golden vectors for the MFVI selection by predictive scores
(psvi_predict_scores; the reference's psvi/inference/utils.py:221-452, 941-1084
and psvi/inference/baselines.py:1515-1727).

Runs ONLY in the development container.  Like tools/gen_golden_mfvi.py, the
parent re-launches this script in a child whose sys.path holds the reference
and not this repo; the child calls the reference's own classes on small
in-memory datasets and records every Normal draw in order, the initial
parameters (by wrapping the set_up_model the modules call) and the results:

  z1_scores     ScoreSelection._get_uncertainty_score (loaded=False) for
                least_confidence and entropy, _el2n_score on the least-confidence
                pass's probabilities, and ScoreSelection.select's indices for both
  z2_forgetting MeanFieldVI(forgetting_score_flag=True).run(), 3 iterations (with
                the parameters each after_epoch scored with)
  z3_evaluate   MfviSelect.evaluate_coreset, 4 iterations on 7 chosen rows

The discrete outputs are compared exactly, so the generator asserts their
margins: no row of any recorded no-grad forward has a top-two mean-logit gap
below 1e-3, and every class leaves more than 1e-3 between its last kept and its
first dropped score.

Usage:  python tools/gen_golden_mfvi_select.py    (writes tests/golden/z*.npz)
"""
import json
import os
import subprocess
import sys
import tempfile

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
GAP = 1e-3


def _child():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from gen_golden import _install_stubs, _Recorder

    _install_stubs()
    import numpy as np
    import torch
    from torch.nn.utils import parameters_to_vector
    from torch.utils.data import Dataset

    import psvi.inference.baselines as B
    import psvi.inference.utils as U

    torch.set_default_dtype(torch.float32)
    rec = _Recorder()
    captured = {"gaps": []}

    def hook(_, __, out):
        # the predictive forwards run under no_grad: their mean logits' top-two gap
        if not torch.is_grad_enabled():
            ml = out.squeeze(-1).mean(0)
            if ml.shape[-1] > 1:
                top = ml.topk(2, dim=-1).values
                captured["gaps"].append(float((top[:, 0] - top[:, 1]).min()))

    def wrap(mod):
        orig = mod.set_up_model

        def setup_wrapper(**kw):
            net = orig(**kw)
            captured["p0"] = parameters_to_vector(net.parameters()).detach().clone()
            net.register_forward_hook(hook)
            return net

        mod.set_up_model = setup_wrapper

    wrap(B)
    wrap(U)

    class Rows(Dataset):
        def __init__(self, x, y):
            self.data, self.targets = x, y

        def __len__(self):
            return len(self.data)

        def __getitem__(self, i):
            return self.data[i], self.targets[i]

    gen = torch.Generator().manual_seed(2024)

    def dataset(n, D, nc, Wt):
        x = torch.randn(n, D, generator=gen)
        return Rows(x, (x @ Wt).argmax(1).float())

    def flat(net):
        return parameters_to_vector(net.parameters()).detach().cpu().numpy()

    def check_gaps(what):
        g = min(captured["gaps"])
        assert g >= GAP, f"{what}: a top-two mean-logit gap of {g:.2e}: pick another seed"
        captured["gaps"] = []
        return g

    # ---- z1: the scores of one net over 150 rows (two eps blocks), and select
    D, nc, H, S, n = 5, 3, 8, 3, 150
    Wt = torch.randn(D, nc, generator=gen)
    train = dataset(n, D, nc, Wt)
    torch.manual_seed(3)
    net = U.set_up_model(architecture="fn", D=D, n_hidden=H, nc=nc, mc_samples=S, init_sd=0.05)
    with torch.no_grad():  # a spread of logits a fresh net does not have
        for p in list(net.parameters())[::2]:
            p.mul_(6.0)
    p0 = flat(net)
    out = dict(x=train.data.numpy(), y=train.targets.numpy(), params=p0)
    tmp = tempfile.mkdtemp()
    num_pseudo = 10
    for st in ("least_confidence", "entropy"):
        sel = U.ScoreSelection(train, num_pseudo, nc, 0, score_type=st, data_folder=tmp,
                               dnm="toy", loaded=False)
        sel.pretrained_net, sel.device = net, torch.device("cpu")
        probs = []
        if st == "least_confidence":
            orig = sel._least_confidence_score
            sel._least_confidence_score = lambda p: (probs.append(p.clone()), orig(p))[1]
        rec.start()
        score = sel._get_uncertainty_score()
        out["eps_" + st] = rec.stop().numpy().astype(np.float32)
        out["score_" + st] = score.numpy().astype(np.float64)
        if probs:
            out["score_el2n"] = sel._el2n_score(torch.cat(probs), train.targets).numpy().astype(
                np.float64)
        check_gaps("z1 " + st)
        # select draws again; the scores it ranks are kept for the margin check
        kept = {}
        orig_get = sel._get_uncertainty_score
        sel._get_uncertainty_score = lambda: kept.setdefault("s", orig_get())
        rec.start()
        idx = sel.select()
        out["eps_select_" + st] = rec.stop().numpy().astype(np.float32)
        out["select_" + st] = np.array(idx, np.int64)
        captured["gaps"] = []
        s_np, y_np = kept["s"].numpy().astype(np.float64), train.targets.numpy()
        for c in range(nc):
            sc = np.sort(s_np[y_np == c])[::-1]
            k = sum(1 for i in idx if y_np[i] == c)
            assert k < len(sc) and sc[k - 1] - sc[k] > GAP, (st, c, sc[k - 1] - sc[k])
    cfg = dict(layers=[[D, H], [H, H], [H, nc]], S=S, nc=nc, rows_per_draw=128, num_pseudo=num_pseudo)
    np.savez_compressed(os.path.join(OUT, "z1_scores.npz"), config=np.array(json.dumps(cfg)), **out)
    print("wrote z1_scores:", {k: v.shape for k, v in out.items()})

    # ---- z2: MeanFieldVI with forgetting events, 3 iterations
    D, nc, H, S, n, nt, mb = 4, 3, 6, 3, 50, 12, 16
    Wt = torch.randn(D, nc, generator=gen)
    train, test = dataset(n, D, nc, Wt), dataset(nt, D, nc, Wt)
    vi = U.MeanFieldVI(mc_samples=S, data_minibatch=mb, num_epochs=3, log_every=2, N=n, D=D,
                       lr0net=0.05, mul_fact=1, seed=0, architecture="fn", n_hidden=H, nc=nc,
                       train_dataset=train, test_dataset=test, init_sd=0.3,
                       forgetting_score_flag=True, data_path=tmp, dnm="toy")
    # the parameters every after_epoch scores with
    epoch_params = []
    orig_after = vi.after_epoch
    vi.after_epoch = lambda: (epoch_params.append(flat(vi.net)), orig_after())[1]
    rec.start()
    vi.run()
    draws = rec.stop().numpy().astype(np.float32)
    g = check_gaps("z2")
    cfg = dict(layers=[[D, H], [H, H], [H, nc]], S=S, nc=nc, D=D, n_hidden=H, data_minibatch=mb,
               num_epochs=3, log_every=2, lr=0.05, init_sd=0.3, seed=0)
    np.savez_compressed(
        os.path.join(OUT, "z2_forgetting.npz"), config=np.array(json.dumps(cfg)),
        x=train.data.numpy(), y=train.targets.numpy(), xt=test.data.numpy(),
        yt=test.targets.numpy(), params0=captured["p0"].numpy(), draws=draws,
        params=flat(vi.net), epoch_params=np.stack(epoch_params),
        elbos=np.array(vi.elbos_mfvi, np.float64),
        accs=np.array(vi.accs_mfvi, np.float64), nlls=np.array(vi.nlls_mfvi, np.float64),
        last_acc=vi.last_acc.cpu().numpy(), forgetting=vi.forgetting_events.cpu().numpy(),
        never_learnt=vi.never_learnt_events.cpu().numpy())
    print(f"wrote z2_forgetting: elbos {vi.elbos_mfvi[:2]}..., accs {vi.accs_mfvi}, min gap {g:.2e}, "
          f"forgetting {vi.forgetting_events.tolist()}")

    # ---- z3: MfviSelect.evaluate_coreset on 7 chosen rows, unequal weights
    ms = B.MfviSelect(train_dataset=train, test_dataset=test, data_minibatch=64, num_pseudo=7,
                      nc=nc, architecture="fn", D=D, n_hidden=H, mc_samples=S, init_sd=0.3,
                      lr0net=0.02, num_epochs=4, log_every=2, seed=0, mul_fact=1,
                      score_method="entropy")
    chosen = [3, 41, 17, 8, 29, 45, 12]
    wts = (n / 7.0) * (1.0 + 0.1 * torch.arange(7.0))

    class Chosen(U.WeightedSubset):
        # torch >= 2.1 batches a Subset through __getitems__, which would skip
        # the reference's __getitem__ and its (idx, data, target, weight) items
        def __getitems__(self, indices):
            return [self[i] for i in indices]

    ms.chosen_dataset = Chosen(train, chosen, wts)
    ms.wt_index = {}
    rec.start()
    res = ms.evaluate_coreset()
    draws = rec.stop().numpy().astype(np.float32)
    g = check_gaps("z3")
    cfg = dict(layers=[[D, H], [H, H], [H, nc]], S=S, nc=nc, D=D, n_hidden=H, data_minibatch=64,
               num_epochs=4, log_every=2, lr=0.02, init_sd=0.3, seed=0, num_pseudo=7)
    np.savez_compressed(
        os.path.join(OUT, "z3_evaluate.npz"), config=np.array(json.dumps(cfg)),
        x=train.data.numpy(), y=train.targets.numpy(), xt=test.data.numpy(),
        yt=test.targets.numpy(), params0=captured["p0"].numpy(), draws=draws,
        chosen=np.array(chosen, np.int64), weights=wts.numpy(), params=flat(ms.net),
        elbos=np.array(res["elbos"], np.float64), accs=np.array(res["accs"], np.float64),
        nlls=np.array(res["nlls"], np.float64))
    print(f"wrote z3_evaluate: elbos {res['elbos']}, accs {res['accs']}, min gap {g:.2e}")


def main():
    if "--child" in sys.argv:
        _child()
        return
    os.makedirs(OUT, exist_ok=True)
    env = dict(os.environ)
    env["PYTHONPATH"] = REF
    env["PYTHONDONTWRITEBYTECODE"] = "1"
    subprocess.run([sys.executable, "-B", os.path.abspath(__file__), "--child"],
                   env=env, check=True, cwd="/tmp")


if __name__ == "__main__":
    main()
