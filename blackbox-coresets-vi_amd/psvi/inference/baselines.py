"""Mean-field VI baselines of the reference's psvi/inference/baselines.py on the
HIP inner-step kernels:

  run_mfvi         baselines.py:824-914   VI on data minibatches (weights N/B)
  run_mfvi_subset  baselines.py:917-1062  VI on a fixed random subset (weights N/M)

Each iteration is the inner ELBO of the HIP library with uniform coreset
weights -- psvi_elbo_grad on the batch, then torch.optim.Adam's update
(PSVI_ADAM_TORCH, psvi_adam_update) -- with the reference's quirks kept: the
loss sums the NLL over the S samples too, and its KL term sums over
``VILinear`` modules only (baselines.py:889, 1033), so a full-covariance stack
trains without KL.  The predictive evaluation every ``log_every`` iterations
averages the LOGITS over samples (baselines.py:898-906) and runs the model's
torch forward on the device (not the hot path).  There is no CPU fallback:
the training step raises without the HIP library or a device.

MFVI regression baselines ("MFVI regressor fit"):

  fit                        baselines.py:1283-1346  the ELBO fit and its predictive logs
  run_mfvi_regressor         baselines.py:1066-1169  MFVI on the training set, tau by validation
  run_mfvi_subset_regressor  baselines.py:1172-1278  MFVI on a fixed random subset

A fit is psvi_mfvi_fit: every Adam step of the mean-field Gaussian-likelihood
MLP in one launch per segment between logging checkpoints (``log_every == -1``:
one launch for the whole fit), ``elbos`` read from its per-step losses
afterwards.  The predictive log is psvi_evaluate_regression with no
pseudopoints and uniform weights: the mean prediction over the samples in the
targets' units, the squared error and the log-density with scale 1 / sqrt(tau).
Model selection fits every candidate tau in ONE call (one workgroup per tau).
Reference behaviours kept:

* ``fit`` takes ``next(iter(train_loader))`` of a loader built with
  ``shuffle=False`` at every step: the same first minibatch, scaled by
  ``n_train / B``, for the whole fit (the subset variant: its one subset
  batch).  This is what makes the single-launch fit exact.
* The loss sums the NLL over the S samples too; ``elbos`` holds -loss before
  each step; ``times`` one entry per logging checkpoint.
* ``bpe = max(1, int(n_train / data_minibatch))`` and ``epochs = num_epochs *
  bpe`` steps; a logging checkpoint at ``it % log_every == 0``, or at the last
  step alone when ``log_every == -1``.
* Each candidate tau gets a newly initialised net, drawn from the continuing
  torch generator in tau order, then the final fit another one (the loaders'
  own draws of a base seed are kept out of that stream); ``best_tau``
  moves only on a strictly larger last validation log-likelihood.
* The subset is ``random.sample(range(n_train), num_pseudo)`` after the reseed,
  its scale ``n_train / num_pseudo`` (n_train the whole training set); it
  selects tau only on request.
* The Philox offsets continue from fit to fit as the sequential fits would
  consume the stream (training steps, then the evaluation draws).
The nets are make_regressor_net's (``n_hidden`` units, ``n_layers`` hidden
layers, default 2 as the reference's set_up_model builds 'regressor_net');
the predictive log needs mc_samples >= 2 (psvi_evaluate_regression).

Laplace coreset baselines ("Laplace baselines"):

  run_random    baselines.py:118-203   uniform random coreset, weights N / |core|
  run_sparsevi  baselines.py:426-648   Sparse VI (Campbell & Beronov, 2019)
  run_opsvi     baselines.py:652-821   the original PSVI (Manousakas et al., 2020)

Their shared core runs on the HIP library: the Laplace fit of the weighted
logistic regression on the coreset, its diagonal precision and samples
(psvi_laplace_fit: the whole chain of Adam steps in one launch), and the
scores, weight gradient and pseudo-input gradient from the samples' centred
log-likelihoods (psvi_laplace_scores).  The noise -- d floats for theta0, S d
for the samples -- is drawn on the host from the CPU generators in the
reference's order and uploaded with the request.  Reference behaviours kept:

* ``run_laplace`` reseeds ``random``, ``numpy`` and ``torch`` with its ``seed``
  on every call.  ``run_sparsevi`` calls it without a seed, so 0 is used; the
  minibatch indices and ``random.choice`` that follow a logging step restart
  from that seed.
* In ``run_random`` and at sparsevi's logging step theta0 is drawn before the
  reseed; both fit 1000 steps there whatever ``inner_it`` says.
* sparsevi creates a new ``optim_w`` every epoch: fresh Adam state over the
  full w (N,), only core entries get gradient, ``clamp_(w, 0)`` follows each
  step.  The point attached is the true argmax of corr over the minibatch.
* In sparsevi's step 4 theta carries across the ``outer_it`` fits while each
  fit's Adam is new.
* opsvi's weight optimiser runs at ``lr0v * N``; its pseudo-inputs carry the
  ones column with zero gradient; its ``optim_net`` is re-created each epoch
  and its theta persists (the logging fit trains the same theta).  The
  reference's ``optim_w.zero_grad()`` / ``w.grad.data = ...`` pair is taken
  with in-place zeroing, the behaviour it was written against: the gradients
  the step sees are exactly the ones assigned.
* opsvi's ``us`` / ``vs`` logs are numpy views of the live tensors, which the
  in-place optimiser steps keep writing: every logged entry holds the final
  values.
* ``run_random`` sets ``w[core] = N / len(core)``.

  run_giga      baselines.py:207-423   GIGA (Campbell & Broderick, 2018)

GIGA shares the Laplace fit; its geodesic direction, greedy pick and line
search are one launch of psvi_giga_step per step.  Reference behaviours kept:

* ``mc_samples = max(mc_samples, 50)``.
* The posterior samples come once, from a 1000-step Laplace fit on
  ``subset_size`` random rows with weights ``N / data_minibatch``; every step
  works on those samples.
* The geodesic step sits inside ``if it % log_every == 0``: the coreset grows
  only on logging iterations (a minibatch is still drawn on the others).
* The logging fit takes 100 steps on ``w[core]`` (``w_pred`` is computed but
  read by the mcmc branch only), from a fresh theta0 drawn before
  ``run_laplace``'s reseed; an empty core fits the prior alone.
* ``run_laplace`` reseeds with ``seed`` on every call, so the
  ``np.random.randint`` minibatches after a logging step restart from it.
* ``csizes`` logs ``len(w[w > 0])`` before that iteration's step.
* ``w = clamp(((1 - gamma) w + gamma e_pt) / |(1 - gamma) lw + gamma ell*|, 0)``
  on the full w (N,), the norm taken with the already updated lw.
* The minibatch is drawn with replacement, the first occurrence wins the
  argmax, and a point already in the core is not appended again.

Full precision (``diagonal=False``; DESIGN §4, "Full precision"): the samples
come from MultivariateNormal(theta, precision_matrix=I + X^T diag(w p (1 - p)) X)
(baselines.py:64-70, logreg.py:95-107) through psvi_laplace_sample_full -- the
fit runs without samples, then the precision, its reverse Cholesky factor and
one forward substitution per sample, fp64 in one launch.  The host draws the
same (S, d) standard normals in the same order as on the diagonal path.
``run_laplace(..., diagonal=False)`` is public, and ``_run_sparsevi`` /
``_run_opsvi`` (the bodies of the public functions) take ``diagonal`` for every
selection-loop fit; as in the reference their logging fits stay diagonal.  The
public ``run_sparsevi(diagonal=False)`` / ``run_opsvi(diagonal=False)`` still
raise: tests/test_laplace_cpu.py::test_argument_checks asserts it, and opening
the keyword waits on that test (as ``"giga"`` in ``inf_dict`` does).

MFVI selection ("MFVI selection"):

  MfviSelect               baselines.py:1515-1727  select_data, evaluate_coreset
  run_selection_with_mfvi  baselines.py:1855-1952  pretrain, score, pick, train on the subset

The selection is psvi.inference.utils.CoresetSelect (its module docstring lists
what it keeps of the reference); the training on the chosen rows is
``_MFVIStepper.step`` with one weight per row, the tests one
psvi_predict_scores launch per batch.  Reference behaviours kept:

* ``evaluate_coreset`` steps once per batch of 128 of the chosen rows and calls
  ``zero_grad`` once per outer iteration only: within an iteration the batches'
  gradients accumulate from step to step (visible only when num_pseudo > 128).
* ``elbos`` holds minus the LAST batch's loss of every iteration; ``accs`` /
  ``nlls`` hold the last test only (a one-entry list each; None if no test
  ran); ``times`` is 0; ``csizes`` repeats num_pseudo; ``wt_index`` maps
  str(row index) to its weight n_train / num_pseudo, in the permuted order.
* The net is built in the constructor, after a reseed, before the selection.
Divergences: ``loaded_from_psvi=True`` (a new keyword, passed through to
CoresetSelect, the reference's default there) falls back to computing the
scores; "incremental", kmeans_gradient / submodular, architecture="lenet" and
log_pseudodata raise NotImplementedError; kmeans, scored_kmeans_* and
weighted_kmeans run with ``clustering="hip"`` (psvi_kmeans on the device in
place of sklearn) and are refused without it.

``mcmc=True`` (stan) and, on the public sparsevi / opsvi, ``diagonal=False``
raise NotImplementedError.
Optional test hooks: ``noise_source(n)`` supplies each host draw,
``batch_source()`` the ``np.random.randint`` minibatches,
``choice_source(candidates)`` run_random's ``random.choice``; ``state_out`` (a
dict) receives the final w, core_idcs, theta and, for opsvi, u (for giga: w,
core_idcs, lw and pt_idcs, the point picked at each step).
"""
import random
import time

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader

from ..models import (VILinear, VILinearMultivariateNormal, categorical_fn, make_fc2net,
                      make_fcnet, make_lenet, make_regressor_net, model_spec)
from ..runtime import (InnerLoopPlan, adam_update_, check_binary, giga_step, laplace_fit,
                       laplace_sample_full, laplace_scores, mfvi_fit, predict_scores, randn_)

__all__ = ["set_up_model", "pseudo_subsample_init", "pseudo_rand_init", "run_mfvi",
           "run_mfvi_subset", "process_wt_index", "run_laplace", "run_random", "run_sparsevi",
           "run_opsvi", "run_giga", "fit", "run_mfvi_regressor", "run_mfvi_subset_regressor",
           "MfviSelect", "run_selection_with_mfvi"]


def set_up_model(D=None, n_hidden=None, nc=None, mc_samples=None, architecture=None,
                 **kwargs):
    """experiments_utils.set_up_model (psvi/experiments/experiments_utils.py:346-413)
    for the architectures the HIP path runs.  As there, kwargs (init_sd) reach
    fn / fn2 only; lenet and the logistic regressions take their defaults."""
    if architecture == "fn":
        return make_fcnet(D, n_hidden, nc, linear_class=VILinear, nonl_class=nn.ReLU,
                          mc_samples=mc_samples, **kwargs)
    if architecture == "fn2":
        return make_fc2net(D, n_hidden, nc, linear_class=VILinearMultivariateNormal,
                           nonl_class=nn.ReLU, mc_samples=mc_samples, **kwargs)
    if architecture == "lenet":
        return make_lenet(linear_class=VILinear, nonl_class=nn.ReLU, mc_samples=mc_samples)
    if architecture == "logistic_regression":
        return nn.Sequential(VILinear(D, nc, mc_samples=mc_samples))
    if architecture == "logistic_regression_fullcov":
        return nn.Sequential(VILinearMultivariateNormal(D, nc, mc_samples=mc_samples))
    raise NotImplementedError(f"architecture {architecture!r} is not on the HIP path "
                              "(residual_fn / regressor_net / alexnet / resnet)")


def pseudo_subsample_init(x, y, num_pseudo=20, nc=2, seed=0):
    """psvi/inference/utils.py:33-50: a random subset with num_pseudo // nc points
    per class (the remainder on the last class)."""
    torch.manual_seed(seed)
    N = x.shape[0]
    cnt = 0
    u, z = torch.Tensor([]), torch.Tensor([])
    for c in range(nc):
        idx_c = torch.arange(N)[y == c]
        k = num_pseudo // nc if c < nc - 1 else num_pseudo - cnt
        u = torch.cat((u, x[idx_c[torch.randperm(len(idx_c))[:k]]]))
        z = torch.cat((z, c * torch.ones(k)))
        cnt += num_pseudo // nc
    return u.requires_grad_(True), z


def pseudo_rand_init(x, y, num_pseudo=20, nc=2, seed=0, variance=0.1):
    """psvi/inference/utils.py:53-77: noisy data mean, labels split over classes."""
    torch.manual_seed(seed)
    D = x.shape[1]
    u = (x[:, :].mean() + variance * torch.randn(num_pseudo, D)).clone().requires_grad_(True)
    z = torch.Tensor([])
    for c in range(nc):
        k = num_pseudo // nc if c < nc - 1 else num_pseudo - (nc - 1) * (num_pseudo // nc)
        z = torch.cat((z, c * torch.ones(k)))
    return u, z


class _MFVIStepper:
    """One MFVI iteration on the HIP library for a fixed model: plans cached per
    batch size, parameters and torch-Adam state resident on the device."""

    def __init__(self, net, device, lr, seed, eps_source=None):
        self.net = net
        self.fam, self.layers, self.prior_sd, self.S = model_spec(net)
        self.device = device
        self.lr = float(lr)
        self.plist = list(net.parameters())
        with torch.no_grad():
            self.params = nn.utils.parameters_to_vector(self.plist).detach().to(
                device, torch.float32).clone()
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        self.t = 0
        self.plans = {}
        self.eps_source = eps_source
        self.seed, self.offset = int(seed), 0

    def _plan(self, B):
        if B not in self.plans:
            self.plans[B] = InnerLoopPlan(self.fam, self.layers, self.S, B,
                                          prior_sd=self.prior_sd)
        return self.plans[B]

    def _rows(self, xb, yb):
        B = int(xb.shape[0])
        u = xb.detach().to(self.device, torch.float32).reshape(B, -1).contiguous()
        z = yb.detach().to(self.device)
        if z.is_floating_point() and not torch.equal(z, z.round()):
            raise ValueError("labels must hold class ids")
        return B, u, z.to(torch.int32).contiguous()

    def _draw(self, plan, blocks=1):
        """The noise of ``blocks`` forward passes, one after the other."""
        if self.eps_source is not None:
            eps = [self.eps_source(plan.eps_count).to(self.device, torch.float32)
                   for _ in range(blocks)]
            return (eps[0] if blocks == 1 else torch.cat(eps)).contiguous()
        eps = torch.empty(blocks * plan.eps_count, device=self.device)
        if plan.eps_stride == plan.eps_count:  # the blocks are one stretch of the stream
            randn_(eps, self.seed, self.offset)
            self.offset += blocks * plan.eps_stride
            return eps
        for k in range(blocks):
            randn_(eps[k * plan.eps_count:(k + 1) * plan.eps_count], self.seed, self.offset)
            self.offset += plan.eps_stride
        return eps

    def step(self, xb, yb, scale, weights=None, accumulate=None):
        """loss = sum_b w_b sum_s NLL + KL (VILinear modules), w_b = scale or
        ``weights`` (one per row), and one torch.optim.Adam step; returns the
        loss (device float64).  ``accumulate`` (a zeroed parameter-sized tensor
        the caller keeps) receives the gradient on top of what it holds, and
        the step takes the sum: an optimiser whose zero_grad runs less often
        than its step."""
        B, u, z = self._rows(xb, yb)
        plan = self._plan(B)
        if weights is None:
            w = torch.full((B,), float(scale), device=self.device)
        else:
            w = weights.detach().to(self.device, torch.float32).reshape(B).contiguous()
        eps = self._draw(plan)
        loss, grad = plan.elbo_grad(u, z, w, eps, self.params,
                                    include_kl=self.fam != "fullcov")
        if accumulate is not None:
            grad = accumulate.add_(grad)
        self.t += 1
        adam_update_(self.params, grad, self.m, self.v, step=self.t, lr=self.lr, kind="torch")
        return loss

    def predict(self, x, y, rows_per_draw, want=(), state=None, stats=False):
        """The mean-logit predictive of the rows x in one psvi_predict_scores
        launch, fresh weights per ``rows_per_draw`` rows (psvi.runtime.predict_scores)."""
        if self.fam != "meanfield":
            raise NotImplementedError("the predictive scores run mean-field stacks only")
        n, u, z = self._rows(x, y)
        plan = next(iter(self.plans.values())) if self.plans else self._plan(1)  # M is not read
        eps = self._draw(plan, -(-n // int(rows_per_draw)))
        return predict_scores(plan, u, z, eps, self.params, rows_per_draw, want=want,
                              state=state, stats=stats)

    def sync_model(self):
        with torch.no_grad():
            nn.utils.vector_to_parameters(self.params.to(self.plist[0].dtype), self.plist)


def _evaluate(net, test_loader, device, distr_fn):
    """Mean-logit predictive (baselines.py:892-906): accuracy and mean NLL."""
    total, test_nll, corrects = 0, 0.0, 0.0
    with torch.no_grad():
        for xt, yt in test_loader:
            xt, yt = xt.to(device, non_blocking=True), yt.to(device, non_blocking=True)
            logits = net(xt).squeeze(-1).mean(0)
            corrects += logits.argmax(-1).float().eq(yt).float().sum()
            total += yt.size(0)
            test_nll += -distr_fn(logits=logits).log_prob(yt).sum()
    return float(corrects / float(total)), float(test_nll / float(total))


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("the MFVI baselines run on the HIP library: no HIP device")
    return torch.device("cuda")


def run_mfvi(xt=None, yt=None, mc_samples=4, data_minibatch=128, num_epochs=100, log_every=10,
             N=None, D=None, lr0net=1e-3, mul_fact=2, seed=0, distr_fn=categorical_fn,
             architecture=None, n_hidden=None, nc=2, log_pseudodata=False,
             train_dataset=None, test_dataset=None, init_sd=None, eps_source=None, **kwargs):
    """Mean-field VI on the full training set (baselines.py:824-914): each
    iteration draws a fresh shuffled minibatch, loss = N/B * sum NLL + KL.
    Returns the reference's results dict {accs, nlls, times, elbos, csizes}.
    ``eps_source(n)`` (optional) supplies each training step's noise in the
    library's eps layout; default: the library's Philox stream."""
    if log_pseudodata:
        raise NotImplementedError("log_pseudodata (grid predictions) is not on the HIP path")
    device = _device()
    random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
    nlls, accs, times, elbos = [], [], [0], []
    t_start = time.time()
    net = set_up_model(architecture=architecture, D=D, n_hidden=n_hidden, nc=nc,
                       mc_samples=mc_samples, init_sd=init_sd).to(device)
    train_loader = DataLoader(train_dataset, batch_size=data_minibatch, pin_memory=True,
                              shuffle=True)
    n_train = len(train_loader.dataset)
    test_loader = DataLoader(test_dataset, batch_size=data_minibatch, pin_memory=True,
                             shuffle=True)
    stepper = _MFVIStepper(net, device, lr0net, seed, eps_source)
    total_iterations = mul_fact * num_epochs
    for i in range(total_iterations):
        xbatch, ybatch = next(iter(train_loader))
        loss = stepper.step(xbatch, ybatch, n_train / xbatch.shape[0])
        elbos.append(-loss.item())
        if i % log_every == 0 or i == total_iterations - 1:
            stepper.sync_model()
            a, n = _evaluate(net, test_loader, device, distr_fn)
            times.append(times[-1] + time.time() - t_start)
            accs.append(a)
            nlls.append(n)
    stepper.sync_model()
    return {"accs": accs, "nlls": nlls, "times": times[1:], "elbos": elbos, "csizes": None}


def run_mfvi_subset(x=None, y=None, xt=None, yt=None, mc_samples=4, data_minibatch=128,
                    num_epochs=100, log_every=10, D=None, lr0net=1e-3, mul_fact=2, seed=0,
                    distr_fn=categorical_fn, log_pseudodata=False, train_dataset=None,
                    test_dataset=None, num_pseudo=100, init_args="subsample", architecture=None,
                    n_hidden=None, nc=2, dnm=None, init_sd=None, eps_source=None, **kwargs):
    """Mean-field VI on a fixed random subset of num_pseudo training points
    (baselines.py:917-1062), loss = N/num_pseudo * sum NLL + KL.  The MNIST
    per-class loader branch (dnm="MNIST") needs torchvision datasets and is not
    supported; the subset comes from pseudo_subsample_init / pseudo_rand_init."""
    if log_pseudodata:
        raise NotImplementedError("log_pseudodata (grid predictions) is not on the HIP path")
    if dnm == "MNIST":
        raise NotImplementedError("the torchvision MNIST subset loader is not available")
    device = _device()
    random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
    nlls, accs, times, elbos = [], [], [0], []
    t_start = time.time()
    net = set_up_model(architecture=architecture, D=D, n_hidden=n_hidden, nc=nc,
                       mc_samples=mc_samples, init_sd=init_sd).to(device)
    init = pseudo_rand_init if init_args == "random" else pseudo_subsample_init
    xbatch, ybatch = init(x, y, num_pseudo=num_pseudo, seed=seed, nc=nc)
    n_train = len(train_dataset)
    test_loader = DataLoader(test_dataset, batch_size=data_minibatch, pin_memory=True,
                             shuffle=True)
    stepper = _MFVIStepper(net, device, lr0net, seed, eps_source)
    sum_scaling = n_train / num_pseudo
    for i in range(mul_fact * num_epochs):
        loss = stepper.step(xbatch, ybatch, sum_scaling)
        elbos.append(-loss.item())
        if i % log_every == 0:
            stepper.sync_model()
            a, n = _evaluate(net, test_loader, device, distr_fn)
            times.append(times[-1] + time.time() - t_start)
            accs.append(a)
            nlls.append(n)
    stepper.sync_model()
    return {"accs": accs, "nlls": nlls, "times": times[1:], "elbos": elbos,
            "csizes": [num_pseudo] * (mul_fact * num_epochs)}


# ------------------------------------------------------- MFVI regression baselines
class _Noise:
    """Where a fit's noise comes from: ``eps_source(n)`` (n floats per training
    step or evaluation draw, in the reference's order) or the library's Philox
    stream (seed, a running offset)."""

    def __init__(self, seed=0, offset=0, eps_source=None):
        self.seed, self.offset, self.source = int(seed), int(offset), eps_source


def _fit_members(nets, taus, train_loader, pred_loader, revert_norm, log_every, epochs, device,
                 lr, noise, n_train=None):
    """fit for G = len(nets) members that share everything but tau, their
    parameters and their noise: one psvi_mfvi_fit call per segment."""
    G, epochs = len(nets), int(epochs)
    fam, layers, prior_sd, S = model_spec(nets[0])
    if fam != "meanfield" or layers[-1][1] != 1:
        raise NotImplementedError("fit runs mean-field nets with one output (make_regressor_net)")
    if n_train is None:
        n_train = len(train_loader.dataset)
    # iterating a DataLoader draws its base seed from torch's generator: keep that out of
    # the stream the nets are initialised from
    with torch.random.fork_rng(devices=[]):
        xb, yb = next(iter(train_loader))
        pred_batches = list(pred_loader)
    B = int(xb.shape[0])
    x = xb.detach().to(device, torch.float32).reshape(B, -1).contiguous()
    y = yb.detach().to(device, torch.float32).reshape(-1).contiguous()
    scale = n_train / B
    zero = torch.zeros(())
    y_mean = float(revert_norm(zero))
    y_std = float(revert_norm(zero + 1.0)) - y_mean
    plists = [list(net.parameters()) for net in nets]
    with torch.no_grad():
        params = torch.stack([nn.utils.parameters_to_vector(pl).detach().to(device, torch.float32)
                              for pl in plists]).contiguous()
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    E = S * sum(i * o + o for i, o in layers)
    stride = (E + 3) // 4 * 4
    pred = [(xt.detach().to(device, torch.float32).reshape(int(xt.shape[0]), -1).contiguous(),
             yt.detach().to(device, torch.float32).reshape(-1).contiguous())
            for xt, yt in pred_batches]
    plans = {}
    if log_every > 0:
        marks = [e for e in range(epochs) if e % log_every == 0]
    else:
        marks = [epochs - 1] if epochs > 0 else []
    ends = [e + 1 for e in marks]
    if epochs > 0 and (not ends or ends[-1] != epochs):
        ends.append(epochs)
    # a member's draws in the reference's order: each segment's steps, then its evaluation
    seg_T = [b - a for a, b in zip([0] + ends[:-1], ends)]
    logs = [e - 1 in marks for e in ends]
    per_member = sum(T + (len(pred) if lg else 0) for T, lg in zip(seg_T, logs))
    if noise.source is not None:
        drawn = [[(noise.source(T * E).to(device, torch.float32).reshape(T, E),
                   [noise.source(E).to(device, torch.float32).contiguous() for _ in pred]
                   if lg else []) for T, lg in zip(seg_T, logs)] for _ in range(G)]
    offs = [noise.offset + g * per_member * stride for g in range(G)]
    noise.offset += G * per_member * stride
    res = [dict(rmses=[], lls=[], times=[0], elbos=[], scale=1.0 / np.sqrt(tau)) for tau in taus]
    t_start = time.time()
    losses, done = [], 0
    for k, (T, lg) in enumerate(zip(seg_T, logs)):
        if noise.source is not None:
            eps = torch.stack([drawn[g][k][0] for g in range(G)]).contiguous()
            out = mfvi_fit(layers, S, x, y, scale, taus, params, T, lr, adam_m=m, adam_v=v,
                           step0=done, eps=eps, prior_sd=prior_sd)
        else:
            out = mfvi_fit(layers, S, x, y, scale, taus, params, T, lr, adam_m=m, adam_v=v,
                           step0=done, seed=noise.seed, offsets=offs, prior_sd=prior_sd)
            offs = [o + T * stride for o in offs]
        losses.append(out["loss"])
        done += T
        if not lg:
            continue
        for g, tau in enumerate(taus):
            se, ll, total = 0.0, 0.0, 0
            for b, (xt, yt) in enumerate(pred):
                Bt = int(xt.shape[0])
                key = (Bt, float(tau))
                if key not in plans:
                    plans[key] = InnerLoopPlan("meanfield", layers, S, Bt, prior_sd=prior_sd,
                                               likelihood=("gaussian", tau))
                if noise.source is not None:
                    eps_e = drawn[g][k][1][b]
                else:
                    eps_e = randn_(torch.empty(E, device=device), noise.seed, offs[g])
                    offs[g] += stride
                stats, _ = plans[key].evaluate_regression(0, xt, yt, yt, eps_e, params[g],
                                                          y_mean=y_mean, y_std=y_std,
                                                          correction=False)
                stats = stats.tolist()
                se, ll, total = se + stats[2], ll + stats[3], total + Bt
            r = res[g]
            r["times"].append(r["times"][-1] + time.time() - t_start)
            r["lls"].append(ll / float(total))
            r["rmses"].append(float(np.sqrt(se / float(total))))
    allloss = torch.cat(losses, 1).cpu() if losses else torch.zeros(G, 0)
    for g, r in enumerate(res):
        r["elbos"] = (-allloss[g]).tolist()
        r["times"] = r["times"][1:]
        with torch.no_grad():
            nn.utils.vector_to_parameters(params[g].to(plists[g][0].device, plists[g][0].dtype),
                                          plists[g])
    return res


def fit(net=None, optim_vi=None, train_loader=None, pred_loader=None, revert_norm=None,
        log_every=-1, tau=1e-2, epochs=40, device=None, lr=None, seed=0, offset=0,
        eps_source=None):
    """The reference's fit (baselines.py:1283-1346) on psvi_mfvi_fit: ``epochs``
    torch-Adam steps of the mean-field ELBO on the loader's first minibatch,
    the predictive rmse / log-likelihood of ``pred_loader`` at the logging
    checkpoints.  The learning rate is ``lr`` or ``optim_vi``'s (a new Adam:
    its moments start at zero here); ``revert_norm`` must be the affine map
    y * y_std + y_mean.  Noise: ``eps_source(n)`` or the Philox stream (seed,
    offset).  ``net`` ends with the fitted parameters.  Returns {rmses, lls,
    times, elbos, scale}."""
    device = _device()
    if lr is None:
        if optim_vi is None:
            raise ValueError("fit needs lr or optim_vi")
        lr = optim_vi.param_groups[0]["lr"]
    return _fit_members([net], [float(tau)], train_loader, pred_loader, revert_norm, log_every,
                        epochs, device, float(lr), _Noise(seed, offset, eps_source))[0]


def _regressor_net(D, n_hidden, n_layers, mc_samples, init_sd, nc=1):
    return make_regressor_net(D, n_hidden, nc, n_layers=n_layers, linear_class=VILinear,
                              nonl_class=nn.ReLU, mc_samples=mc_samples, init_sd=init_sd)


def _run_regressor(train_loader, n_train, mc_samples, data_minibatch, num_epochs, log_every, D,
                   lr0net, seed, n_hidden, n_layers, val_dataset, test_dataset, nc, y_mean, y_std,
                   taus, init_sd, model_selection, dnm, eps_source, results_folder):
    device = _device()
    if nc != 1:
        raise NotImplementedError("the regression baselines have one network output (nc=1)")
    if not taus:
        raise ValueError("taus must hold at least one precision")
    test_loader = DataLoader(test_dataset, batch_size=data_minibatch, shuffle=False)
    val_loader = DataLoader(val_dataset, batch_size=data_minibatch, shuffle=False)
    bpe = max(1, int(n_train / data_minibatch))  # batches per epoch
    y_mean, y_std = float(y_mean), float(y_std)

    def revert_norm(y_pred):
        return y_pred * y_std + y_mean

    noise = _Noise(seed, 0, eps_source)
    best_tau, best_ll = taus[0], -float("inf")
    if model_selection:
        nets = [_regressor_net(D, n_hidden, n_layers, mc_samples, init_sd) for _ in taus]
        fits = _fit_members(nets, [float(t) for t in taus], train_loader, val_loader, revert_norm,
                            -1, num_epochs * bpe, device, lr0net, noise, n_train)
        for tau, tau_fit in zip(taus, fits):
            if tau_fit["lls"][-1] > best_ll:
                best_tau, best_ll = tau, tau_fit["lls"][-1]
    if dnm is not None:
        from ..experiments.experiments_utils import update_hyperparams_dict

        update_hyperparams_dict(dnm, best_tau, results_folder=results_folder)
    net = _regressor_net(D, n_hidden, n_layers, mc_samples, init_sd)
    return _fit_members([net], [float(best_tau)], train_loader, test_loader, revert_norm,
                        log_every, num_epochs * bpe, device, lr0net, noise, n_train)[0]


def run_mfvi_regressor(mc_samples=4, data_minibatch=128, num_epochs=100, log_every=10, D=None,
                       lr0net=1e-3, seed=0, architecture=None, n_hidden=None, train_dataset=None,
                       val_dataset=None, test_dataset=None, nc=1, y_mean=None, y_std=None,
                       taus=None, init_sd=1e-6, model_selection=True, dnm=None, n_layers=2,
                       eps_source=None, results_folder="results", **kwargs):
    """MFVI for BNN regression on the training set (baselines.py:1066-1169): tau
    chosen on the validation set over ``taus`` (all candidates in one
    psvi_mfvi_fit call), then the fit of the chosen tau logged on the test set.
    Returns {rmses, lls, times, elbos, scale}."""
    if architecture not in (None, "regressor_net"):
        raise NotImplementedError(f"architecture {architecture!r}: the regression baselines "
                                  "build 'regressor_net'")
    _device()
    random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
    train_loader = DataLoader(train_dataset, batch_size=data_minibatch, shuffle=False)
    return _run_regressor(train_loader, len(train_dataset), mc_samples, data_minibatch,
                          num_epochs, log_every, D, lr0net, seed, n_hidden, n_layers, val_dataset,
                          test_dataset, nc, y_mean, y_std, taus, init_sd, model_selection, dnm,
                          eps_source, results_folder)


def run_mfvi_subset_regressor(mc_samples=4, data_minibatch=128, num_epochs=100, log_every=10,
                              D=None, lr0net=1e-3, seed=0, architecture=None, n_hidden=None,
                              train_dataset=None, val_dataset=None, test_dataset=None, nc=1,
                              y_mean=None, y_std=None, init_sd=1e-6, num_pseudo=100, taus=None,
                              model_selection=False, n_layers=2, eps_source=None, **kwargs):
    """MFVI on a fixed random subset of num_pseudo training rows
    (baselines.py:1172-1278), loss scale n_train / num_pseudo with n_train the
    whole training set's size, as run_mfvi_subset scales its subset (the
    reference's fit reads the length of the loader it is given, which for the
    subset loader is num_pseudo itself: scale 1).  Returns fit's dict plus
    csizes = [num_pseudo]."""
    if architecture not in (None, "regressor_net"):
        raise NotImplementedError(f"architecture {architecture!r}: the regression baselines "
                                  "build 'regressor_net'")
    _device()
    random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
    sample_idcs = random.sample(range(len(train_dataset)), num_pseudo)
    subset = torch.utils.data.Subset(train_dataset, sample_idcs)
    subset_loader = DataLoader(subset, batch_size=num_pseudo, shuffle=False)
    results = _run_regressor(subset_loader, len(train_dataset), mc_samples, data_minibatch, num_epochs, log_every, D, lr0net, seed,
                             n_hidden, n_layers, val_dataset, test_dataset, nc, y_mean, y_std,
                             taus, init_sd, model_selection, None, eps_source, "results")
    results["csizes"] = [num_pseudo]
    return results


# ---------------------------------------------------------------- Laplace baselines
def process_wt_index(log_core_idcs, log_core_wts):
    """psvi/inference/utils.py:180-192: per logging step, {core index: weight}."""
    return [{int(i): float(wts[int(i)]) for i in idcs}
            for idcs, wts in zip(log_core_idcs, log_core_wts)]


def _reseed(seed):
    random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)


def _refuse(mcmc, diagonal=True):
    if mcmc:
        raise NotImplementedError("mcmc=True needs stan, which is not on the HIP path")
    if not diagonal:
        raise NotImplementedError("diagonal=False is not open on run_sparsevi / run_opsvi yet "
                                  "(run_laplace and _run_sparsevi / _run_opsvi take it)")


def _draw(noise_source, device, *shape):
    """A host draw of the reference (Normal.rsample / MultivariateNormal.rsample
    on the CPU generator: the same standard normals in the same order)."""
    n = int(np.prod(shape))
    if noise_source is not None:
        out = torch.as_tensor(noise_source(n), dtype=torch.float32).reshape(-1)
        if out.numel() != n:
            raise ValueError(f"noise_source returned {out.numel()} draws, expected {n}")
    else:
        out = torch.empty(n).normal_()
    return out.reshape(shape).to(device).contiguous()


def _fit(theta, xc, yc, wc, T, lr, eps, want_loss=False, diagonal=True):
    """T Adam steps on theta (in place), then the samples from eps (S, d) under
    the diagonal or the full Laplace precision: (samples, loss)."""
    if diagonal:
        out = laplace_fit(xc, yc, wc, theta, T, lr, eps=eps, want_loss=want_loss)
        return out["samples"], out["loss"]
    loss = laplace_fit(xc, yc, wc, theta, T, lr, want_loss=want_loss)["loss"]
    return laplace_sample_full(xc, wc, theta, eps=eps)["samples"], loss


def run_laplace(x_core, y_core, w_core, theta, inner_it=1000, lr0net=1e-3, diagonal=True,
                mc_samples=4, seed=0, noise_source=None):
    """Samples from the Laplace approximation on a weighted coreset
    (baselines.py:35-70, the optimiser argument replaced by its learning rate):
    reseeds every generator, takes ``inner_it`` steps of a new Adam on theta
    (d,), IN PLACE, and returns the (mc_samples, d) device samples under the
    diagonal precision or, with ``diagonal=False``, the full one.  x_core
    (n_core, d) carries the ones column; an empty core fits the prior alone."""
    device = _device()
    f32 = dict(device=device, dtype=torch.float32)
    xc, yc, wc = (t.detach().to(**f32).contiguous() for t in (x_core, y_core, w_core))
    th = theta.detach().to(**f32).contiguous()
    _reseed(seed)
    eps = _draw(noise_source, device, int(mc_samples), int(th.numel()))
    smp, _ = _fit(th, xc, yc, wc, inner_it, lr0net, eps, diagonal=diagonal)
    if th.data_ptr() != theta.data_ptr():
        with torch.no_grad():
            theta.copy_(th)
    return smp


class _Laplace:
    """Device side of one Laplace-baseline run: the augmented train and test
    rows, the host noise draws and the library entries."""

    def __init__(self, x, y, xt, yt, mc_samples, noise_source):
        self.device = _device()
        f32 = dict(device=self.device, dtype=torch.float32)
        x, xt = x.detach().to(**f32), xt.detach().to(**f32)
        x, xt = x.reshape(x.shape[0], -1), xt.reshape(xt.shape[0], -1)
        self.x = torch.cat((x, torch.ones(x.shape[0], 1, **f32)), dim=1).contiguous()
        self.xt = torch.cat((xt, torch.ones(xt.shape[0], 1, **f32)), dim=1).contiguous()
        self.y, self.yt = y.detach().to(**f32).contiguous(), yt.detach().to(**f32)
        self.N, self.d = int(self.x.shape[0]), int(self.x.shape[1])
        self.S, self.noise_source = int(mc_samples), noise_source

    def draw(self, *shape):
        """A host draw of the reference."""
        return _draw(self.noise_source, self.device, *shape)

    def fit(self, theta, xc, yc, wc, T, lr, want_loss=False, diagonal=True):
        """T Adam steps on theta (in place), then S samples: (samples, loss)."""
        return _fit(theta, xc, yc, wc, T, lr, self.draw(self.S, self.d), want_loss=want_loss,
                    diagonal=diagonal)

    def run_laplace(self, theta, xc, yc, wc, T, lr, seed=0, diagonal=True):
        """baselines.py:35-70: reseeds every generator first."""
        _reseed(seed)
        return self.fit(theta, xc, yc, wc, T, lr, diagonal=diagonal)[0]

    def predict(self, samples):
        """logreg_forward and the test metrics: (accuracy, mean NLL)."""
        probs = (self.xt @ samples.T).sigmoid().mean(dim=1)
        acc = probs.gt(0.5).float().eq(self.yt).float().mean().item()
        nll = (-torch.distributions.Bernoulli(probs=probs).log_prob(self.yt).mean()).item()
        return acc, nll

    def minibatch(self, B, batch_source):
        idx = batch_source() if batch_source is not None else np.random.randint(self.N, size=B)
        idx = np.asarray(idx, dtype=np.int64)
        return idx, torch.as_tensor(idx, device=self.device)

    def scores(self, samples, xc, yc, wc, sub_t, **want):
        rows = torch.cat((xc, self.x[sub_t])).contiguous()
        labels = torch.cat((yc, self.y[sub_t])).contiguous()
        return laplace_scores(samples, rows, labels, wc, int(xc.shape[0]),
                              self.N / int(sub_t.numel()), **want)


def run_random(x=None, y=None, xt=None, yt=None, mc_samples=4, num_epochs=100, log_every=10,
               N=None, D=None, seed=0, mcmc=False, lr0net=1e-3, noise_source=None,
               choice_source=None, state_out=None, **kwargs):
    """A Laplace fit on a uniformly random subset of the training data that
    grows by one point per epoch (baselines.py:118-203).  Returns the
    reference's results dict {accs, nlls, csizes, times, wt_index}."""
    _refuse(mcmc)
    check_binary(y, "y")
    _reseed(seed)
    L = _Laplace(x, y, xt, yt, mc_samples, noise_source)
    N = L.N
    w = torch.zeros(N, device=L.device)
    nlls, accs, csizes, times, core_idcs = [], [], [], [0], []
    log_core_idcs, log_core_wts = [], []
    theta = None
    t_start = time.time()
    for it in range(num_epochs):
        if it % log_every == 0:
            ci = torch.as_tensor(np.asarray(core_idcs, dtype=np.int64), device=L.device)
            theta = L.draw(L.d)  # drawn before run_laplace reseeds
            smp = L.run_laplace(theta, L.x[ci].contiguous(), L.y[ci].contiguous(),
                                w[ci].contiguous(), 1000, lr0net, seed=seed)
            times.append(times[-1] + time.time() - t_start)
            acc, nll = L.predict(smp)
            nlls.append(nll), accs.append(acc), csizes.append(len(core_idcs))
            log_core_idcs.append(core_idcs.copy())
            log_core_wts.append(w.cpu().numpy().tolist())
        candidates = tuple(set(range(N)).difference(set(core_idcs)))
        pt = choice_source(candidates) if choice_source is not None else random.choice(candidates)
        core_idcs.append(int(pt))
        w[torch.as_tensor(core_idcs, device=L.device)] = N / len(core_idcs)
    if state_out is not None:
        state_out.update(w=w.cpu().numpy(), core_idcs=list(core_idcs),
                         theta=None if theta is None else theta.cpu().numpy())
    return {"accs": accs, "nlls": nlls, "csizes": csizes, "times": times[1:],
            "wt_index": process_wt_index(log_core_idcs, log_core_wts)}


def run_giga(x=None, y=None, xt=None, yt=None, mc_samples=100, data_minibatch=512,
             num_epochs=100, log_every=10, N=None, D=None, seed=0, mcmc=False, subset_size=200,
             lr0net=1e-3, noise_source=None, batch_source=None, state_out=None, **kwargs):
    """GIGA (Campbell & Broderick, 2018; baselines.py:207-423): posterior samples
    from one Laplace fit on a random subset, then on every logging iteration a
    fit on the coreset and one geodesic-ascent step on the minibatch: the point
    whose direction aligns best with the residual's is attached and the weights
    follow the line search.  Returns the reference's results dict {accs, nlls,
    csizes, times}."""
    _refuse(mcmc)
    check_binary(y, "y")
    _reseed(seed)
    L = _Laplace(x, y, xt, yt, max(mc_samples, 50), noise_source)
    N, B = L.N, int(data_minibatch)
    w = torch.zeros(N, device=L.device)
    nlls, accs, csizes, times, core_idcs, pt_idcs = [], [], [], [0], [], []
    t_start = time.time()
    _, sub_t = L.minibatch(int(subset_size), batch_source)
    theta = L.draw(L.d)  # drawn before run_laplace reseeds
    smp = L.run_laplace(theta, L.x[sub_t].contiguous(), L.y[sub_t].contiguous(),
                        torch.full((sub_t.numel(),), N / B, device=L.device), 1000, lr0net,
                        seed=seed)
    lw = torch.zeros(L.S, device=L.device)
    for it in range(num_epochs):
        sub, sub_t = L.minibatch(B, batch_source)
        if it % log_every:
            continue
        ci = torch.as_tensor(np.asarray(core_idcs, dtype=np.int64), device=L.device)
        theta = L.draw(L.d)
        pred = L.run_laplace(theta, L.x[ci].contiguous(), L.y[ci].contiguous(),
                             w[ci].contiguous(), 100, lr0net, seed=seed)
        times.append(times[-1] + time.time() - t_start)
        acc, nll = L.predict(pred)
        nlls.append(nll), accs.append(acc), csizes.append(int((w > 0).sum()))
        step = giga_step(smp, L.x[sub_t].contiguous(), L.y[sub_t].contiguous(), lw)
        res = step["result"].tolist()
        pt, gamma, scale = int(sub[int(res[1])]), res[5], res[6]
        pt_idcs.append(pt)
        if pt not in core_idcs:
            core_idcs.append(pt)
        lw = step["lw"]
        w = (1 - gamma) * w
        w[pt] += gamma
        w = torch.clamp_(w * scale, 0)
    if state_out is not None:
        state_out.update(w=w.cpu().numpy(), core_idcs=list(core_idcs), lw=lw.cpu().numpy(),
                         pt_idcs=pt_idcs)
    return {"accs": accs, "nlls": nlls, "csizes": csizes, "times": times[1:]}


def run_sparsevi(x=None, y=None, xt=None, yt=None, mc_samples=4, data_minibatch=128,
                 num_epochs=100, log_every=10, N=None, D=None, diagonal=True, inner_it=10,
                 outer_it=10, lr0net=1e-3, lr0v=1e-1, seed=0, mcmc=False, noise_source=None,
                 batch_source=None, state_out=None, **kwargs):
    """Sparse VI (Campbell & Beronov, 2019; baselines.py:426-648): per epoch a
    Laplace fit on the coreset, the greedy pick of the minibatch point whose
    centred log-likelihood correlates best with the residual, and ``outer_it``
    projected Adam steps on the weights, each after a fit of its own.  Returns
    the reference's results dict {nlls, accs, csizes, times, wt_index}."""
    _refuse(mcmc, diagonal)
    return _run_sparsevi(x=x, y=y, xt=xt, yt=yt, mc_samples=mc_samples,
                         data_minibatch=data_minibatch, num_epochs=num_epochs,
                         log_every=log_every, diagonal=diagonal, inner_it=inner_it,
                         outer_it=outer_it, lr0net=lr0net, lr0v=lr0v, seed=seed,
                         noise_source=noise_source, batch_source=batch_source,
                         state_out=state_out)


def _run_sparsevi(x, y, xt, yt, mc_samples=4, data_minibatch=128, num_epochs=100, log_every=10,
                  diagonal=True, inner_it=10, outer_it=10, lr0net=1e-3, lr0v=1e-1, seed=0,
                  noise_source=None, batch_source=None, state_out=None):
    """run_sparsevi's body.  ``diagonal=False`` draws every selection-loop
    sample from the full Laplace precision (baselines.py:540-548, 602-610); the
    logging fit stays diagonal, as in the reference (baselines.py:501)."""
    check_binary(y, "y")
    outer_it = min(outer_it, 500)
    _reseed(seed)
    L = _Laplace(x, y, xt, yt, mc_samples, noise_source)
    N, B = L.N, int(data_minibatch)
    w = torch.zeros(N, device=L.device, requires_grad=True)
    nlls, accs, csizes, times, core_idcs = [], [], [], [0], []
    log_core_idcs, log_core_wts = [], []
    theta = None

    def core():
        ci = torch.as_tensor(np.asarray(core_idcs, dtype=np.int64), device=L.device)
        return ci, L.x[ci].contiguous(), L.y[ci].contiguous(), w.detach()[ci].contiguous()

    t_start = time.time()
    for it in range(num_epochs):
        ci, xc, yc, wc = core()
        if it % log_every == 0:
            theta = L.draw(L.d)  # drawn before run_laplace reseeds (with its default, 0)
            smp = L.run_laplace(theta, xc, yc, wc, 1000, lr0net)
            times.append(times[-1] + time.time() - t_start)
            acc, nll = L.predict(smp)
            nlls.append(nll), accs.append(acc), csizes.append(len(core_idcs))
            log_core_idcs.append(core_idcs.copy())
            log_core_wts.append(w.detach().cpu().numpy().tolist())
        # 1. the coreset posterior; 2. log-likelihoods; 3. the point to attach
        sub, sub_t = L.minibatch(B, batch_source)
        theta = L.draw(L.d)
        smp, _ = L.fit(theta, xc, yc, wc, inner_it, lr0net, diagonal=diagonal)
        res = L.scores(smp, xc, yc, wc, sub_t)["result"].tolist()
        if res[3] > 0:
            pt = int(sub[int(res[1])])
            if pt not in core_idcs:
                core_idcs.append(pt)
        # 4. projected Adam steps on the weights, a fit before each
        ci, xc, yc, _ = core()
        optim_w = torch.optim.Adam([w], lr0v)
        theta = L.draw(L.d)
        for _ in range(outer_it):
            wc = w.detach()[ci].contiguous()
            smp, _ = L.fit(theta, xc, yc, wc, inner_it, lr0net, diagonal=diagonal)
            sub, sub_t = L.minibatch(B, batch_source)
            gw = L.scores(smp, xc, yc, wc, sub_t, want_grad_w=True)["grad_w"]
            w.grad = torch.zeros_like(w)
            w.grad[ci] = gw
            optim_w.step()
            with torch.no_grad():
                torch.clamp_(w, 0)
    if state_out is not None:
        state_out.update(w=w.detach().cpu().numpy(), core_idcs=[int(i) for i in core_idcs],
                         theta=None if theta is None else theta.cpu().numpy())
    return {"nlls": nlls, "accs": accs, "csizes": csizes, "times": times[1:],
            "wt_index": process_wt_index(log_core_idcs, log_core_wts)}


def run_opsvi(x=None, y=None, xt=None, yt=None, mc_samples=10, data_minibatch=128,
              num_epochs=100, log_every=10, N=None, D=None, num_pseudo=10, inner_it=10,
              diagonal=True, lr0net=1e-3, lr0u=1e-3, lr0v=1e-3, register_elbos=False,
              init_args="subsample", seed=0, mcmc=False, log_pseudodata=False,
              noise_source=None, batch_source=None, state_out=None, **kwargs):
    """The original PSVI construction (Manousakas et al., 2020;
    baselines.py:652-821): ``num_pseudo`` weighted pseudo-points (u, z), a
    Laplace fit on them every epoch, then one Adam step on the weights and one
    on the pseudo-inputs.  Returns the reference's results dict {accs, nlls,
    csizes, times, elbos} (+ us, zs, vs under log_pseudodata)."""
    _refuse(mcmc, diagonal)
    return _run_opsvi(x=x, y=y, xt=xt, yt=yt, mc_samples=mc_samples,
                      data_minibatch=data_minibatch, num_epochs=num_epochs, log_every=log_every,
                      num_pseudo=num_pseudo, inner_it=inner_it, diagonal=diagonal, lr0net=lr0net,
                      lr0u=lr0u, lr0v=lr0v, register_elbos=register_elbos, init_args=init_args,
                      seed=seed, log_pseudodata=log_pseudodata, noise_source=noise_source,
                      batch_source=batch_source, state_out=state_out)


def _run_opsvi(x, y, xt, yt, mc_samples=10, data_minibatch=128, num_epochs=100, log_every=10,
               num_pseudo=10, inner_it=10, diagonal=True, lr0net=1e-3, lr0u=1e-3, lr0v=1e-3,
               register_elbos=False, init_args="subsample", seed=0, log_pseudodata=False,
               noise_source=None, batch_source=None, state_out=None):
    """run_opsvi's body.  ``diagonal=False`` draws every epoch's samples from
    the full Laplace precision (baselines.py:768-776); the logging fit stays
    diagonal, as in the reference (baselines.py:730)."""
    _reseed(seed)
    L = _Laplace(x, y, xt, yt, mc_samples, noise_source)
    N, B = L.N, int(data_minibatch)
    csizes, elbos, n_logged = [], [], 0
    nlls, accs, times = [], [], [0]
    w = (N / num_pseudo * torch.ones(num_pseudo, device=L.device)).requires_grad_(True)
    theta = L.draw(L.d)
    init = pseudo_rand_init if init_args == "random" else pseudo_subsample_init
    with torch.no_grad():
        u0, z0 = init(x.detach().cpu().float().reshape(N, -1), y.detach().cpu(),
                      num_pseudo=num_pseudo, seed=seed)
    u = torch.cat((u0.detach().float(), torch.ones(num_pseudo, 1)), dim=1).to(
        L.device).contiguous().requires_grad_(True)
    z = z0.float().to(L.device).contiguous()
    optim_u = torch.optim.Adam([u], lr0u)
    optim_w = torch.optim.Adam([w], lr0v * N)
    t_start = time.time()
    for it in range(num_epochs):
        if it % log_every == 0:
            smp = L.run_laplace(theta, u.detach(), z, w.detach(), inner_it, lr0net, seed=seed)
            times.append(times[-1] + time.time() - t_start)
            acc, nll = L.predict(smp)
            csizes.append(num_pseudo), nlls.append(nll), accs.append(acc)
            n_logged += 1
        smp, loss = L.fit(theta, u.detach(), z, w.detach(), inner_it, lr0net,
                          want_loss=register_elbos, diagonal=diagonal)
        if register_elbos:
            elbos.extend((1, -l) for l in loss.tolist()[::log_every])
        sub, sub_t = L.minibatch(B, batch_source)
        sc = L.scores(smp, u.detach(), z, w.detach(), sub_t, want_grad_w=True, want_grad_u=True)
        w.grad, u.grad = sc["grad_w"], sc["grad_u"]
        optim_w.step()
        optim_u.step()
        with torch.no_grad():
            torch.clamp_(w, 0)
    if state_out is not None:
        state_out.update(w=w.detach().cpu().numpy(), core_idcs=list(range(num_pseudo)),
                         theta=theta.cpu().numpy(), u=u.detach().cpu().numpy())
    results = {"accs": accs, "nlls": nlls, "csizes": csizes, "times": times[1:], "elbos": elbos}
    if log_pseudodata:
        # the reference logs u.detach().numpy() / w.detach().numpy(): views of the
        # live tensors, which the in-place optimiser steps keep writing, so every
        # logged entry holds the final values
        results["us"] = [u.detach().cpu().numpy()] * n_logged
        results["zs"] = [z.cpu().numpy()] * n_logged
        results["vs"] = [w.detach().cpu().numpy()] * n_logged
    return results


# ------------------------------------------------------------- MFVI selection
class MfviSelect:
    """MFVI on a subset of the training rows chosen by CoresetSelect
    (baselines.py:1515-1727): ``select_data`` pretrains, scores and picks the
    rows, ``evaluate_coreset`` trains this object's own net on the weighted
    subset and returns the reference's results dict."""

    def __init__(self, x=None, y=None, xt=None, yt=None, dnm=None, train_dataset=None,
                 test_dataset=None, data_minibatch=128, num_pseudo=100, nc=2,
                 architecture="logistic_regression", D=None, n_hidden=100, mc_samples=4,
                 init_sd=None, lr0net=1e-3, num_epochs=100, log_every=10,
                 distr_fn=categorical_fn, seed=0, mul_fact=2, log_pseudodata=False,
                 score_method="kmeans", pretrain_epochs=5, data_folder=None,
                 load_from_saved=False, train_weights=True, distance_fn="euclidean",
                 last_layer_only=False, loaded_from_psvi=True, eps_source=None, clustering=None):
        if log_pseudodata:
            raise NotImplementedError("log_pseudodata (grid predictions) is not on the HIP path")
        if architecture == "lenet":
            raise NotImplementedError('architecture="lenet": psvi_predict_scores runs the affine '
                                      "mean-field stacks only")
        self.x, self.y, self.xt, self.yt, self.dnm = x, y, xt, yt, dnm
        self.train_dataset, self.test_dataset = train_dataset, test_dataset
        self.data_minibatch, self.num_pseudo, self.nc = data_minibatch, num_pseudo, nc
        self.architecture, self.D, self.n_hidden = architecture, D, n_hidden
        self.mc_samples, self.init_sd, self.lr0net = mc_samples, init_sd, lr0net
        self.num_epochs, self.log_every, self.distr_fn = num_epochs, log_every, distr_fn
        self.seed, self.mul_fact, self.log_pseudodata = seed, mul_fact, log_pseudodata
        self.score_method, self.pretrain_epochs = score_method, pretrain_epochs
        self.data_folder, self.load_from_saved = data_folder, load_from_saved
        self.train_weights, self.distance_fn = train_weights, distance_fn
        self.last_layer_only, self.loaded_from_psvi = last_layer_only, loaded_from_psvi
        self.eps_source, self.clustering = eps_source, clustering
        self.wt_vec = len(self.train_dataset) / self.num_pseudo * torch.ones(self.num_pseudo)
        self._setup()

    def select_data(self):
        from .utils import CoresetSelect

        select_method = CoresetSelect(
            train_dataset=self.train_dataset, score_method=self.score_method,
            test_dataset=self.test_dataset, num_pseudo=self.num_pseudo, nc=self.nc,
            architecture=self.architecture, D=self.D, n_hidden=self.n_hidden,
            distr_fn=self.distr_fn, mc_samples=self.mc_samples, init_sd=self.init_sd,
            data_minibatch=self.data_minibatch, pretrain_epochs=self.pretrain_epochs,
            lr0net=self.lr0net, log_every=10, data_folder=self.data_folder,
            load_from_saved=self.load_from_saved, dnm=self.dnm, distance_fn=self.distance_fn,
            last_layer_only=self.last_layer_only, loaded_from_psvi=self.loaded_from_psvi,
            eps_source=self.eps_source, clustering=self.clustering)
        select_method.select_data()
        self.chosen_dataset = select_method.chosen_dataset
        self.wt_index = select_method.wt_index

    def _setup(self):
        self.device = _device()
        random.seed(self.seed), np.random.seed(self.seed), torch.manual_seed(self.seed)
        self.net = set_up_model(architecture=self.architecture, D=self.D, n_hidden=self.n_hidden,
                                nc=self.nc, mc_samples=self.mc_samples,
                                init_sd=self.init_sd).to(self.device)

    def _test(self, stepper):
        """The last test alone is kept: one launch per batch of a newly shuffled loader."""
        test_loader = DataLoader(self.test_dataset, batch_size=self.data_minibatch,
                                 pin_memory=True, shuffle=True)
        total, stats = 0, torch.zeros(2, dtype=torch.float64, device=self.device)
        for xt, yt in test_loader:
            stats += stepper.predict(xt, yt, int(xt.shape[0]), stats=True)["stats"]
            total += yt.size(0)
        corrects, test_nll = stats.tolist()
        return [corrects / float(total)], [test_nll / float(total)]

    def evaluate_coreset(self):
        """baselines.py:1660-1727: per iteration one step per batch of 128 of the
        chosen rows, under ONE zero_grad: the batches' gradients add up across
        the steps of an iteration (visible when num_pseudo > 128)."""
        elbos_mfvi, accs_mfvi, nlls_mfvi = [], None, None
        stepper = _MFVIStepper(self.net, self.device, self.lr0net, self.seed, self.eps_source)
        items = [self.chosen_dataset[i] for i in range(len(self.chosen_dataset))]
        xs = torch.stack([torch.as_tensor(it[1]) for it in items])
        ys = torch.as_tensor([float(it[2]) for it in items])
        ws = torch.as_tensor([float(it[3]) for it in items])
        batches = [(xs[lo:lo + 128], ys[lo:lo + 128], ws[lo:lo + 128])
                   for lo in range(0, len(items), 128)]
        acc = torch.zeros_like(stepper.params) if len(batches) > 1 else None
        for i in range(self.mul_fact * self.num_epochs):
            if acc is not None:
                acc.zero_()
            for xb, yb, wb in batches:
                loss = stepper.step(xb, yb, None, weights=wb, accumulate=acc)
            elbos_mfvi.append(-loss.item())
            if i % self.log_every == 0:
                accs_mfvi, nlls_mfvi = self._test(stepper)
        stepper.sync_model()
        return {"accs": accs_mfvi, "nlls": nlls_mfvi, "times": 0, "elbos": elbos_mfvi,
                "csizes": [self.num_pseudo] * (self.mul_fact * self.num_epochs),
                "wt_index": self.wt_index}


def run_selection_with_mfvi(x=None, y=None, xt=None, yt=None, mc_samples=4, data_minibatch=128,
                            num_epochs=100, log_every=10, D=None, lr0net=1e-3, mul_fact=2,
                            seed=0, distr_fn=categorical_fn, log_pseudodata=False,
                            train_dataset=None, test_dataset=None, num_pseudo=100,
                            init_args="subsample", architecture=None, n_hidden=None, nc=2,
                            dnm=None, init_sd=None, mfvi_selection_method="kmeans",
                            pretrain_epochs=5, data_folder=None, load_from_saved=False,
                            distance_fn="euclidean", last_layer_only=False,
                            loaded_from_psvi=True, eps_source=None, clustering=None, **kwargs):
    """Pretrain by MFVI, score every training row, keep the top rows per class,
    train MFVI on that weighted subset (baselines.py:1855-1952).  Returns
    {accs, nlls, times, elbos, csizes, wt_index}.  clustering="hip" opens the
    k-means methods on psvi_kmeans (CoresetSelect); None refuses them."""
    if mfvi_selection_method == "incremental":
        raise NotImplementedError('mfvi_selection_method "incremental" starts from a k-means '
                                  "selection (sklearn), which is not on the HIP path")
    mfvi_select = MfviSelect(
        x=x, y=y, xt=xt, yt=yt, dnm=dnm, train_dataset=train_dataset, test_dataset=test_dataset,
        data_minibatch=data_minibatch, num_pseudo=num_pseudo, nc=nc, architecture=architecture,
        D=D, n_hidden=n_hidden, mc_samples=mc_samples, init_sd=init_sd, lr0net=lr0net,
        num_epochs=num_epochs, log_every=log_every, distr_fn=categorical_fn, seed=seed,
        mul_fact=mul_fact, log_pseudodata=log_pseudodata, score_method=mfvi_selection_method,
        pretrain_epochs=pretrain_epochs, data_folder=data_folder,
        load_from_saved=load_from_saved, distance_fn=distance_fn,
        last_layer_only=last_layer_only, loaded_from_psvi=loaded_from_psvi,
        eps_source=eps_source, clustering=clustering)
    mfvi_select.select_data()
    return mfvi_select.evaluate_coreset()
