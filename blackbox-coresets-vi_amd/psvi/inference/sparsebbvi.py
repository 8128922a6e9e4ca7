"""Sparse black-box VI on the HIP path: the reference's incremental variational
coreset ``run_sparsevi_with_bb_elbo`` (psvi/inference/sparsebbvi.py:28-198,
with elbo / sparsevi_psvi_elbo / forward_through_coreset /
predict_through_coreset of psvi/inference/utils.py:85-141).

Each epoch (a) fits the mean-field network on the current coreset with
``inner_it`` steps, (b) scores a data minibatch by the correlation of its
scaled log-likelihoods with the residual, (c) attaches one point, and (d)
takes ``outer_it`` projected Adam steps on the weights under the
importance-weighted PSVI ELBO.  The network's forward / backward is the
Bernoulli-likelihood plan of the HIP library (psvi_elbo_grad, psvi_row_loglik),
the sampled KL psvi_sampled_kl_grad, the scores psvi_select_scores and the
weight gradient psvi_select_weight_grad; there is no CPU fallback.

Reference behaviours reproduced ("Sparse-BBVI"):

* The inner objective.  ``elbo`` returns ``(pseudo_nll.sum() - sampled_nkl).sum()``
  with ``sampled_nkl`` of shape (S,): the scalar NLL sum broadcasts against it,
  so the loss is S * sum_{s,m} w_m NLL_sm - sum_s nkl_s -- the weighted NLL
  counts S times.  The plan runs with weights S * w.
* Gradient accumulation.  ``optim_net0.zero_grad()`` runs once per epoch,
  outside the inner loop: inner iteration t feeds Adam the running sum of the
  epoch's gradients.
* Plain Adam state.  ``optim_net0`` is torch.optim.Adam (PSVI_ADAM_TORCH); its
  moments and step count persist across epochs.
* Empty coreset at epoch 0.  The inner loop runs on the sampled-KL term alone;
  no plan with 0 rows is created (the KL term runs on a 1-row plan).
* Point selection.  ``sub_idcs[torch.argmax(torch.max(corrs))]`` is the argmax
  of a 0-dim tensor, i.e. always ``sub_idcs[0]``; a point is attached iff max
  corr > max corecorr or the core is empty.  ``greedy_argmax=True`` takes the
  kernel's true argmax instead.
* Weight optimiser.  torch Adam on the full w (N,), a device tensor; only core
  entries get gradient; ``clamp_(w, 0)`` follows each step.
* Prediction.  ``predict_through_coreset`` forwards the test rows and all N
  training rows; rows with w == 0 add nothing to the weighted sum, so the core
  rows and the test rows are forwarded, under one eps.
  test_probs = clamp(W @ sigmoid(f), max=1).
* Plan reuse.  The coreset grows by at most one row per epoch; plans are
  cached by row count (no padding).

``eps_source(n)`` (optional) supplies the noise of each network forward of the
reference, in the reference's order and the library's eps layout;
``batch_source()`` (optional) the ``np.random.randint`` minibatch indices.
Without them the noise comes from psvi_randn and numpy as seeded.
"""
import time

import numpy as np
import torch
import torch.distributions as dist
import torch.nn as nn

from ..models import VILinear, make_fcnet, model_spec
from ..runtime import (InnerLoopPlan, adam_update_, check_binary, randn_, select_scores,
                       select_weight_grad)

__all__ = ["run_sparsevi_with_bb_elbo"]


class _SparseBBVI:
    """Device state of one run: parameters and torch-Adam moments of the
    network, the weights, and the Bernoulli plans cached by row count."""

    def __init__(self, net, device, lr0, seed, eps_source):
        fam, self.layers, self.prior_sd, self.S = model_spec(net)
        if fam != "meanfield" or self.layers[-1][1] != 1:
            raise ValueError("sparse-BBVI runs a mean-field network with one output")
        self.device, self.lr0 = device, float(lr0)
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

    def plan(self, M):
        if M not in self.plans:
            self.plans[M] = InnerLoopPlan("meanfield", self.layers, self.S, M,
                                          prior_sd=self.prior_sd, likelihood="bernoulli")
        return self.plans[M]

    def draw(self, plan):
        if self.eps_source is not None:
            return self.eps_source(plan.eps_count).to(self.device, torch.float32).contiguous()
        eps = torch.empty(plan.eps_count, device=self.device)
        randn_(eps, self.seed, self.offset)
        self.offset += plan.eps_stride
        return eps

    def elbo_grad(self, xc, yc, wc):
        """utils.elbo and its gradient at one draw: (loss float64 (1,), grad)."""
        Nu = int(xc.shape[0])
        plan = self.plan(max(Nu, 1))
        eps = self.draw(plan)
        if Nu:
            loss, grad = plan.elbo_grad(xc, yc, (self.S * wc).contiguous(), eps, self.params,
                                        include_kl=False)
        else:
            loss = torch.zeros(1, dtype=torch.float64, device=self.device)
            grad = torch.zeros_like(self.params)
        nkl = plan.sampled_kl_grad(eps, self.params, grad=grad)
        return loss - nkl.sum(), grad

    def inner_loop(self, xc, yc, wc, inner_it, on_loss=None):
        gsum = torch.zeros_like(self.params)  # zero_grad() once per epoch
        for in_it in range(inner_it):
            loss, grad = self.elbo_grad(xc, yc, wc)
            if on_loss is not None:
                on_loss(in_it, loss)
            gsum += grad
            self.t += 1
            adam_update_(self.params, gsum, self.m, self.v, step=self.t, lr=self.lr0,
                         kind="torch")

    def loglik(self, xc, yc, xd, yd, logits=False):
        """ll (S, Nu + Nd), f, nkl of cat(core, data) rows under one draw."""
        rows = torch.cat((xc, xd)).contiguous()
        labels = torch.cat((yc, yd)).contiguous()
        plan = self.plan(int(rows.shape[0]))
        return plan.row_loglik(rows, labels, self.draw(plan), self.params, logits=logits)

    def predict(self, xc, yc, wc, xt):
        """predict_through_coreset: (test logits (S, Nt), W (S))."""
        Nu = int(xc.shape[0])
        ll, f, nkl = self.loglik(xc, yc, xt, torch.zeros(xt.shape[0], dtype=torch.int32,
                                                        device=self.device), logits=True)
        lw = nkl.clone()
        if Nu:
            lw += ll[:, :Nu].double() @ wc.double()
        return f[:, Nu:], lw.softmax(-1).float()


def run_sparsevi_with_bb_elbo(n_layers=1, logistic_regression=True, n_hidden=40, log_every=10,
                              lr0=1e-3, register_elbos=False, seed=0, eps_source=None,
                              batch_source=None, greedy_argmax=False, params0=None,
                              state_out=None, **kwargs):
    """Incremental variational coreset with the PSVI objective (module
    docstring: the reference behaviours kept).  Takes the reference's keywords
    (num_epochs, inner_it, outer_it, x, y, xt, yt, mc_samples, data_minibatch,
    scatterplot_coreset) and returns its results dict {accs, nlls, csizes,
    times, elbos}.  ``params0`` (optional) replaces the seeded initialisation of
    the network's parameter vector; ``state_out`` (a dict, optional) receives
    the final w, core_idcs and params."""
    if kwargs.get("scatterplot_coreset", False):
        raise NotImplementedError("scatterplot_coreset (grid plots) is not on the HIP path")
    if not torch.cuda.is_available():
        raise RuntimeError("sparse-BBVI runs on the HIP library: no HIP device")
    device = torch.device("cuda")
    np.random.seed(seed), torch.manual_seed(seed)
    num_epochs, inner_it, outer_it = kwargs["num_epochs"], kwargs["inner_it"], kwargs["outer_it"]
    mc_samples, B = kwargs["mc_samples"], int(kwargs["data_minibatch"])
    x = kwargs["x"].detach().to(device, torch.float32)
    xt = kwargs["xt"].detach().to(device, torch.float32)
    x, xt = x.reshape(x.shape[0], -1).contiguous(), xt.reshape(xt.shape[0], -1).contiguous()
    N, D = x.shape
    y_f, yt_f = kwargs["y"].detach().to(device), kwargs["yt"].detach().to(device)
    check_binary(y_f, "y")
    y, yt = y_f.to(torch.int32).contiguous(), yt_f.float()
    net = (nn.Sequential(VILinear(D, 1, mc_samples=mc_samples)) if logistic_regression
           else make_fcnet(D, n_hidden, 1, n_layers=n_layers, linear_class=VILinear,
                           nonl_class=nn.ReLU, mc_samples=mc_samples))
    if params0 is not None:
        with torch.no_grad():
            nn.utils.vector_to_parameters(torch.as_tensor(params0, dtype=torch.float32),
                                          list(net.parameters()))
    st = _SparseBBVI(net, device, lr0, seed, eps_source)
    w = torch.zeros(N, device=device, requires_grad=True)
    optim_w = torch.optim.Adam([w], lr0)
    core_idcs, elbos = [], []
    nlls, accs, csizes, times = [], [], [], [0]
    t_start = time.time()

    def minibatch():
        idx = batch_source() if batch_source is not None else np.random.randint(N, size=B)
        return np.asarray(idx, dtype=np.int64)

    def core():
        ci = torch.as_tensor(np.asarray(core_idcs, dtype=np.int64), device=device)
        return ci, x[ci].contiguous(), y[ci].contiguous(), w.detach()[ci].contiguous()

    for it in range(num_epochs):
        ci, xc, yc, wc = core()
        if it % log_every == 0:
            f, W = st.predict(xc, yc, wc, xt)
            test_probs = torch.clamp(W @ f.sigmoid(), max=1)
            accs.append(test_probs.gt(0.5).float().eq(yt).float().mean().item())
            nlls.append((-dist.Bernoulli(probs=test_probs).log_prob(yt).mean()).item())
            csizes.append(len(core_idcs))
            times.append(times[-1] + time.time() - t_start)
        sub = minibatch()
        sum_scaling = N / len(sub)
        # 1. the coreset posterior: inner_it ELBO steps on the coreset support
        log1 = (lambda i, l: elbos.append((1, -l.item())) if i % log_every == 0 else None)
        st.inner_loop(xc, yc, wc, inner_it, log1 if register_elbos else None)
        # 2. log-likelihoods of the core and the minibatch; 3. the scores
        sub_t = torch.as_tensor(sub, device=device)
        ll, _, nkl = st.loglik(xc, yc, x[sub_t], y[sub_t])
        sc = select_scores(ll, nkl, wc, len(core_idcs), sum_scaling)
        res = sc["result"].tolist()
        if res[3] > 0:
            pt = int(sub[int(res[1])] if greedy_argmax else sub[0])
            if pt not in core_idcs:
                core_idcs.append(pt)
        # 4. projected Adam steps on the weights under the PSVI ELBO
        ci, xc, yc, _ = core()
        sub = minibatch()
        sub_t = torch.as_tensor(sub, device=device)
        for out_it in range(outer_it):
            wc = w.detach()[ci].contiguous()
            ll, _, nkl = st.loglik(xc, yc, x[sub_t], y[sub_t])
            loss, gw = select_weight_grad(ll, nkl, wc, N)
            if register_elbos and out_it % log_every == 0:
                elbos.append((0, -loss.item()))
            w.grad = torch.zeros_like(w)
            w.grad[ci] = gw
            optim_w.step()
            with torch.no_grad():
                torch.clamp_(w, 0)
    if state_out is not None:
        state_out.update(w=w.detach().cpu().numpy(), core_idcs=[int(i) for i in core_idcs],
                         params=st.params.cpu().numpy())
    return {"accs": accs, "nlls": nlls, "csizes": csizes, "times": times[1:], "elbos": elbos}
