"""Host wrapper around one libpsvi_hip plan.

``InnerLoopPlan`` owns a ``psvi_plan`` (geometry + device work lists) and
launches the fused HIP inner step, the autograd-boundary ELBO/gradient, or the
sharded phases on torch's current HIP stream.  All tensors are caller-owned
torch tensors on the GPU; this module only checks shapes and passes pointers.
"""
import ctypes

import torch
from torch.autograd.graph import increment_version

from . import _lib
from ._lib import AdamHP, Likelihood, NetDesc, check


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need(t, name, numel, dtype=torch.float32):
    if t is None:
        raise ValueError(f"{name} is required")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor (got {t.device})")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name} has {t.numel()} elements, expected {numel}")


def _wrote(*tensors):
    """Bump the version counters of tensors the library wrote in place (no
    torch op saw the write), so that a resident inner-loop state keyed to
    them is not taken up after it (InnerLoopPlan.inner_loop(keep=True)).
    Every method that hands a workspace to the library marks it written (the
    library also drops its resident state in every entry point but the loop's
    own)."""
    for t in tensors:
        if t is not None:
            increment_version(t)


def make_adam(lr, step, kind="higher", betas=(0.9, 0.999), eps=1e-8):
    k = {"higher": _lib.ADAM_HIGHER, "hypergrad": _lib.ADAM_HYPERGRAD,
         "torch": _lib.ADAM_TORCH}[kind]
    return AdamHP(float(lr), float(betas[0]), float(betas[1]), float(eps), int(step), k)


class _Token:
    """What a KEEP inner loop left resident: compared by tensor identity,
    version counters, seed and the continuing Philox offset."""

    __slots__ = ("tensors", "versions", "seed", "offset")

    def __init__(self, tensors, versions, seed, offset):
        self.tensors, self.versions, self.seed, self.offset = tensors, versions, seed, offset

    def __eq__(self, o):
        return (all(a is b for a, b in zip(self.tensors, o.tensors)) and self.versions == o.versions
                and self.seed == o.seed and self.offset == o.offset)


class InnerLoopPlan:
    """family: 'meanfield' (VILinear stack) or 'fullcov' (VILinearMultivariateNormal
    stack); layers: [(in, out), ...]; S: global MC samples; M: pseudopoints.
    likelihood: None (categorical, class ids in an int32 z) or ("gaussian", tau):
    Normal(f, 1 / sqrt(tau)) over the one network output, the regressors'
    observation model -- every z / z_all is then a float32 tensor of targets;
    or "bernoulli" (also ("bernoulli", None)): Bernoulli(logits = f) over the one
    output, int32 class ids in {0, 1} in z -- sparse black-box VI."""

    def __init__(self, family, layers, S, M, prior_sd=1.0, world=1, rank=0, likelihood=None):
        self.lib = _lib.load()
        if likelihood is None:
            self.likelihood, self.tau = "categorical", None
        elif likelihood == "bernoulli" or tuple(likelihood) == ("bernoulli", None):
            self.likelihood, self.tau = "bernoulli", None
        else:
            kind, tau = likelihood
            if kind != "gaussian":
                raise ValueError(f"unknown likelihood {kind!r} (None, 'bernoulli' or "
                                 "('gaussian', tau))")
            self.likelihood, self.tau = "gaussian", float(tau)
        # dtype of every z / z_all argument
        self._zdtype = torch.float32 if self.likelihood == "gaussian" else torch.int32
        self._resident = None  # inner_loop(keep=True)'s token
        self.family = family
        fam = {"meanfield": _lib.FAMILY_MEANFIELD, "fullcov": _lib.FAMILY_FULLCOV,
               "lenet": _lib.FAMILY_LENET}[family]
        layers = [tuple(int(x) for x in l) for l in layers]
        if family == "lenet":
            # fixed make_lenet stack (conv "in" = in_channels * 25); input 1x28x28
            if layers != [(25, 6), (150, 16), (400, 120), (120, 84), (84, 10)]:
                raise ValueError(f"not make_lenet's layer table: {layers}")
            self.in_features = 784
        else:
            for a, b in zip(layers[:-1], layers[1:]):
                if a[1] != b[0]:
                    raise ValueError(f"layer sizes do not chain: {layers}")
            self.in_features = layers[0][0]
        if not 1 <= len(layers) <= _lib.MAX_LAYERS:
            raise ValueError("1..8 layers supported")
        self.layers = layers
        self.S, self.M, self.world, self.rank = int(S), int(M), int(world), int(rank)
        d = NetDesc()
        d.n_layers = len(layers)
        dims = [layers[0][0]] + [o for _, o in layers]
        for i, v in enumerate(dims):
            d.dims[i] = v
        d.S, d.M, d.prior_sd = self.S, self.M, float(prior_sd)
        self.desc = d
        h = ctypes.c_void_p()
        if self.likelihood != "categorical":
            lik = (Likelihood(_lib.LIK_GAUSSIAN, self.tau) if self.likelihood == "gaussian"
                   else Likelihood(_lib.LIK_BERNOULLI, 0.0))
            check(self.lib.psvi_plan_create_lik(fam, ctypes.byref(d), self.world, self.rank,
                                                ctypes.byref(lik), ctypes.byref(h)),
                  "psvi_plan_create_lik")
        else:
            check(self.lib.psvi_plan_create(fam, ctypes.byref(d), self.world, self.rank,
                                            ctypes.byref(h)), "psvi_plan_create")
        self.handle = h
        q = self._query
        self.param_count = q(_lib.Q_PARAM_COUNT)
        self.eps_count = q(_lib.Q_EPS_COUNT)
        self.ws_bytes = q(_lib.Q_WS_BYTES)
        self.s_local = q(_lib.Q_S_LOCAL)
        self.s_offset = q(_lib.Q_S_OFFSET)
        self.acc_count = q(_lib.Q_ACC_COUNT)
        self.rows_local = q(_lib.Q_ROWS_LOCAL)
        self.xshard_count = q(_lib.Q_XSHARD_COUNT)
        self.xrecv_count = q(_lib.Q_XRECV_COUNT)
        self.loop_ws_bytes = q(_lib.Q_LOOP_WS_BYTES)
        self.tiled_floats = q(_lib.Q_TILED_FLOATS)  # 0: no tiled state for this plan
        self.outer_ws_bytes = q(_lib.Q_OUTER_WS_BYTES)
        self.hvp_ws_bytes = q(_lib.Q_HVP_WS_BYTES)
        self.eval_ws_bytes = q(_lib.Q_EVAL_WS_BYTES)
        self.net_part_ok = bool(q(_lib.Q_NET_PART_OK))
        self.net_mchunks = q(_lib.Q_NET_MCHUNKS)   # pseudopoint chunks of the network kernels
        self.eps_stride = (self.eps_count + 3) // 4 * 4   # Philox offset per loop step
        self.n_tot = sum(i * o + o for i, o in layers)

    def _query(self, key):
        v = ctypes.c_int64()
        check(self.lib.psvi_plan_query(self.handle, key, ctypes.byref(v)), "psvi_plan_query")
        return v.value

    def shard_info(self, r):
        """Rank r's samples and rows: s_offset, s_count, rows (x-shard columns),
        row_lo / row_cnt per layer (row_lo -1 when the layer's rows are several
        runs) and runs = [(layer, first row, count, x-shard column)] in column
        order (psvi_plan_shard_runs)."""
        out = (ctypes.c_int64 * (3 + 2 * _lib.MAX_LAYERS))()
        check(self.lib.psvi_plan_shard_info(self.handle, r, out), "psvi_plan_shard_info")
        L = len(self.layers)
        n = ctypes.c_int32()
        check(self.lib.psvi_plan_shard_runs(self.handle, r, None, 0, ctypes.byref(n)),
              "psvi_plan_shard_runs")
        buf = (ctypes.c_int64 * max(4 * n.value, 1))()
        check(self.lib.psvi_plan_shard_runs(self.handle, r, buf, n.value, ctypes.byref(n)),
              "psvi_plan_shard_runs")
        runs = [tuple(int(buf[4 * i + k]) for k in range(4)) for i in range(n.value)]
        return dict(s_offset=out[0], s_count=out[1], rows=out[2],
                    row_lo=[out[3 + l] for l in range(L)],
                    row_cnt=[out[3 + _lib.MAX_LAYERS + l] for l in range(L)], runs=runs)

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                self.lib.psvi_plan_destroy(h)
            except Exception:
                pass
            self.handle = None

    # ----------------------------------------------------------- buffers
    def workspace(self, device="cuda"):
        return torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)

    def _inputs(self, u, z, w, eps):
        _need(u, "u", self.M * self.in_features)
        _need(z, "z", self.M, self._zdtype)
        _need(w, "w", self.M)
        _need(eps, "eps", self.eps_count)

    # ------------------------------------------------- sparse black-box VI
    def sampled_kl_grad(self, eps, params, grad=None, nkl=None):
        """The sampled KL term of every layer (psvi_sampled_kl_grad, mean-field
        plans): returns nkl (S float64, log p(theta_s) - log q(theta_s)); with
        ``grad`` (param_count float32) the gradient of -sum_s nkl_s is ADDED
        into it.  Bitwise reproducible."""
        _need(eps, "eps", self.eps_count)
        _need(params, "params", self.param_count)
        if grad is not None:
            _need(grad, "grad", self.param_count)
        if nkl is None:
            nkl = torch.empty(self.S, dtype=torch.float64, device=params.device)
        _need(nkl, "nkl", self.S, torch.float64)
        check(self.lib.psvi_sampled_kl_grad(self.handle, _ptr(eps), _ptr(params), _ptr(nkl),
                                            _ptr(grad), _stream()), "psvi_sampled_kl_grad")
        if grad is not None:
            _wrote(grad)
        return nkl

    def row_loglik(self, x_all, z_all, eps, params, logits=False, nkl=True):
        """Per-sample, per-row log-likelihoods of a Bernoulli plan's M rows under
        ONE draw eps (psvi_row_loglik).  Returns (ll, f, nkl): ll (S, M) float32
        = -NLL; f (S, M) the raw outputs when ``logits``; nkl (S) float64 when
        ``nkl`` (else None).  The labels must be class ids in {0, 1}: checked by
        the caller (``check_binary``)."""
        if self.likelihood != "bernoulli":
            raise ValueError("row_loglik needs a Bernoulli-likelihood plan")
        _need(x_all, "x_all", self.M * self.in_features)
        _need(z_all, "z_all", self.M, torch.int32)
        _need(eps, "eps", self.eps_count)
        _need(params, "params", self.param_count)
        dev = params.device
        ll = torch.empty(self.S, self.M, dtype=torch.float32, device=dev)
        f = torch.empty(self.S, self.M, dtype=torch.float32, device=dev) if logits else None
        k = torch.empty(self.S, dtype=torch.float64, device=dev) if nkl else None
        check(self.lib.psvi_row_loglik(self.handle, _ptr(x_all), _ptr(z_all), _ptr(eps),
                                       _ptr(params), _ptr(ll), _ptr(f), _ptr(k), _stream()),
              "psvi_row_loglik")
        return ll, f, k

    # --------------------------------------------------------- world == 1
    def inner_step(self, u, z, w, eps, params, adam_m, adam_v, step, lr, kind="higher",
                   elbo_out=None, ws=None):
        """One fused inner step (psvi_inner_step); params/m/v updated in place.
        Returns the (device, float64) negative ELBO at the incoming params."""
        self._inputs(u, z, w, eps)
        for t, n in ((params, "params"), (adam_m, "adam_m"), (adam_v, "adam_v")):
            _need(t, n, self.param_count)
        if elbo_out is None:
            elbo_out = torch.empty(1, dtype=torch.float64, device=params.device)
        _need(elbo_out, "elbo_out", 1, torch.float64)
        if ws is None:
            ws = self.workspace(params.device)
        hp = make_adam(lr, step, kind)
        check(self.lib.psvi_inner_step(self.handle, _ptr(u), _ptr(z), _ptr(w), _ptr(eps),
                                       _ptr(params), _ptr(adam_m), _ptr(adam_v),
                                       ctypes.byref(hp), _ptr(elbo_out), _ptr(ws),
                                       ws.numel(), _stream()), "psvi_inner_step")
        _wrote(params, adam_m, adam_v, ws)
        return elbo_out

    def inner_loop(self, u, z, w, params, adam_m, adam_v, T, lr, kind="higher", step0=1,
                   eps=None, seed=0, offset=0, elbo_out=None, ws=None, keep=False):
        """T chained inner steps (psvi_inner_loop).  eps: (T, eps_count) device
        tensor, or None for in-library Philox draws (seed, offset + t * eps_stride).
        Returns the (T,) float64 device tensor of negative ELBOs before each step.

        keep=True (Philox mode, full-cov plans with a tiled state): the loop's
        state stays in ws -- the tiled corr / m / v, the next step's draw and
        sample -- and the next call that continues this one takes it up
        instead of redoing the first steps' fixed work (psvi_inner_loop_ex
        KEEP / RESUME).  It continues when it passes the same ws, params,
        adam_m, adam_v tensors, unmodified since (version counters; this
        plan's own in-place writers bump them), the same seed and offset +
        T * eps_stride.  The resumed numbers are those of one call over all
        the steps, bit for bit, when the last call of the run has keep=False
        (a keep=True call's last step takes the fused update with the next
        sample, where a plain call's last step takes the packed-out one:
        the same values up to fp32 rounding)."""
        _need(u, "u", self.M * self.in_features)
        _need(z, "z", self.M, self._zdtype)
        _need(w, "w", self.M)
        for t, n in ((params, "params"), (adam_m, "adam_m"), (adam_v, "adam_v")):
            _need(t, n, self.param_count)
        T = int(T)
        if eps is not None:
            _need(eps, "eps", T * self.eps_count)
        if elbo_out is None:
            elbo_out = torch.empty(max(T, 1), dtype=torch.float64, device=params.device)
        _need(elbo_out, "elbo_out", None, torch.float64)
        if elbo_out.numel() < T:
            raise ValueError("elbo_out holds fewer than T doubles")
        if ws is None or ws.numel() < self.loop_ws_bytes:
            ws = torch.empty(self.loop_ws_bytes, dtype=torch.uint8, device=params.device)
        hp = make_adam(lr, step0, kind)
        flags = 0
        tok, self._resident = self._resident, None
        if eps is None:
            if keep:
                flags |= _lib.LOOP_KEEP
            if tok is not None and tok == self._loop_token(ws, params, adam_m, adam_v, seed, offset):
                flags |= _lib.LOOP_RESUME
        else:
            keep = False
        check(self.lib.psvi_inner_loop_ex(self.handle, _ptr(u), _ptr(z), _ptr(w), _ptr(eps),
                                          int(seed) & (2**64 - 1), int(offset), T, _ptr(params),
                                          _ptr(adam_m), _ptr(adam_v), ctypes.byref(hp),
                                          _ptr(elbo_out), _ptr(ws), ws.numel(), flags, _stream()),
              "psvi_inner_loop_ex")
        _wrote(params, adam_m, adam_v, ws)
        if keep and T > 0:
            self._resident = self._loop_token(ws, params, adam_m, adam_v, seed,
                                              int(offset) + T * self.eps_stride)
        return elbo_out[:T]

    @staticmethod
    def _loop_token(ws, params, adam_m, adam_v, seed, offset):
        # the tensors themselves (held, so that no new tensor reuses the
        # addresses) and their version counters: any torch write in between
        # makes the next call start cold
        ts = (ws, params, adam_m, adam_v)
        return _Token(ts, tuple(t._version for t in ts), int(seed) & (2**64 - 1), int(offset))

    def elbo_grad(self, u, z, w, eps, params, include_kl=True, ws=None):
        self._inputs(u, z, w, eps)
        _need(params, "params", self.param_count)
        elbo = torch.empty(1, dtype=torch.float64, device=params.device)
        grad = torch.empty(self.param_count, dtype=torch.float32, device=params.device)
        if ws is None:
            ws = self.workspace(params.device)
        check(self.lib.psvi_elbo_grad(self.handle, _ptr(u), _ptr(z), _ptr(w), _ptr(eps),
                                      _ptr(params), int(bool(include_kl)), _ptr(elbo),
                                      _ptr(grad), _ptr(ws), ws.numel(), _stream()),
              "psvi_elbo_grad")
        _wrote(ws)
        return elbo, grad

    def outer_elbo_grad(self, n_pseudo, x_all, z_all, w_all, eps, params, grad=True,
                        grad_u=True, grad_w=True, sample_stats=False, ws=None, grad_z=False):
        """Outer objective (PSVI.psvi_elbo) over this plan's M rows (pseudopoints
        first, n_pseudo of them) -- psvi_outer_elbo_grad.  Returns a dict of
        device tensors: loss (float64, 1), and as requested grad (P), grad_u
        (n_pseudo, D), grad_w (n_pseudo), samples (S, 4: pseudo, data, nkl,
        weight; float64).  grad_z=True (Gaussian plans; needs grad): also grad_z
        (n_pseudo), the gradient of the pseudo rows' targets
        (psvi_outer_elbo_grad_ex)."""
        D = self.in_features
        n_pseudo = int(n_pseudo)
        if grad_z and self.likelihood != "gaussian":
            raise ValueError("grad_z needs a Gaussian-likelihood plan")
        _need(x_all, "x_all", self.M * D)
        _need(z_all, "z_all", self.M, self._zdtype)
        _need(w_all, "w_all", self.M)
        _need(eps, "eps", self.eps_count)
        _need(params, "params", self.param_count)
        dev = params.device
        out = {"loss": torch.empty(1, dtype=torch.float64, device=dev)}
        if grad:
            out["grad"] = torch.empty(self.param_count, dtype=torch.float32, device=dev)
        if grad and grad_u:
            out["grad_u"] = torch.empty(n_pseudo, D, dtype=torch.float32, device=dev)
        if grad_w:
            out["grad_w"] = torch.empty(n_pseudo, dtype=torch.float32, device=dev)
        if sample_stats:
            out["samples"] = torch.empty(self.S, 4, dtype=torch.float64, device=dev)
        if grad and grad_z:
            out["grad_z"] = torch.empty(n_pseudo, dtype=torch.float32, device=dev)
        if ws is None or ws.numel() < self.outer_ws_bytes:
            ws = torch.empty(self.outer_ws_bytes, dtype=torch.uint8, device=dev)
        if "grad_z" in out:
            check(self.lib.psvi_outer_elbo_grad_ex(
                self.handle, n_pseudo, _ptr(x_all), _ptr(z_all), _ptr(w_all), _ptr(eps),
                _ptr(params), _ptr(out["loss"]), _ptr(out.get("grad")), _ptr(out.get("grad_u")),
                _ptr(out.get("grad_w")), _ptr(out["grad_z"]), _ptr(out.get("samples")), _ptr(ws),
                ws.numel(), _stream()), "psvi_outer_elbo_grad_ex")
        else:
            check(self.lib.psvi_outer_elbo_grad(
                self.handle, n_pseudo, _ptr(x_all), _ptr(z_all), _ptr(w_all), _ptr(eps),
                _ptr(params), _ptr(out["loss"]), _ptr(out.get("grad")), _ptr(out.get("grad_u")),
                _ptr(out.get("grad_w")), _ptr(out.get("samples")), _ptr(ws), ws.numel(),
                _stream()), "psvi_outer_elbo_grad")
        _wrote(ws)
        return out

    def outer_ablated_elbo_grad(self, x_all, z_all, w_all, eps, params, grad=True,
                                sample_stats=False, ws=None):
        """PSVI_Ablated.psvi_elbo over this plan's M data rows (no pseudopoints):
        mean_s data_s - mean_s nkl_s -- psvi_outer_ablated_elbo_grad.  Returns
        a dict: loss (float64, 1), grad (P) when requested, samples (S, 4)."""
        D = self.in_features
        _need(x_all, "x_all", self.M * D)
        _need(z_all, "z_all", self.M, self._zdtype)
        _need(w_all, "w_all", self.M)
        _need(eps, "eps", self.eps_count)
        _need(params, "params", self.param_count)
        dev = params.device
        out = {"loss": torch.empty(1, dtype=torch.float64, device=dev)}
        if grad:
            out["grad"] = torch.empty(self.param_count, dtype=torch.float32, device=dev)
        if sample_stats:
            out["samples"] = torch.empty(self.S, 4, dtype=torch.float64, device=dev)
        if ws is None or ws.numel() < self.outer_ws_bytes:
            ws = torch.empty(self.outer_ws_bytes, dtype=torch.uint8, device=dev)
        check(self.lib.psvi_outer_ablated_elbo_grad(
            self.handle, _ptr(x_all), _ptr(z_all), _ptr(w_all), _ptr(eps), _ptr(params),
            _ptr(out["loss"]), _ptr(out.get("grad")), _ptr(out.get("samples")), _ptr(ws),
            ws.numel(), _stream()), "psvi_outer_ablated_elbo_grad")
        _wrote(ws)
        return out

    def outer_grad_coef(self, n_pseudo, x_all, z_all, w_all, eps, params, coef, grad_u=True,
                        grad_w=True, ws=None, grad_z=False):
        """Backward of the outer objective with caller-given per-sample
        coefficients coef = [rowcoef (S, 2) | ck (S) | sck] (float32, 3S + 1)
        -- psvi_outer_elbo_grad_coef, the second pass of the sample-sharded
        outer objective (sharded.ShardedOuter).  Returns grad (P), grad_u
        (n_pseudo, D) and grad_w (n_pseudo) as requested; grad_z (n_pseudo) on
        Gaussian plans (psvi_outer_elbo_grad_coef_ex)."""
        D = self.in_features
        n_pseudo = int(n_pseudo)
        if grad_z and self.likelihood != "gaussian":
            raise ValueError("grad_z needs a Gaussian-likelihood plan")
        _need(x_all, "x_all", self.M * D)
        _need(z_all, "z_all", self.M, self._zdtype)
        _need(w_all, "w_all", self.M)
        _need(eps, "eps", self.eps_count)
        _need(params, "params", self.param_count)
        _need(coef, "coef", 3 * self.S + 1)
        dev = params.device
        out = {"grad": torch.empty(self.param_count, dtype=torch.float32, device=dev)}
        if grad_u:
            out["grad_u"] = torch.empty(n_pseudo, D, dtype=torch.float32, device=dev)
        if grad_w:
            out["grad_w"] = torch.empty(n_pseudo, dtype=torch.float32, device=dev)
        if ws is None or ws.numel() < self.outer_ws_bytes:
            ws = torch.empty(self.outer_ws_bytes, dtype=torch.uint8, device=dev)
        if grad_z:
            out["grad_z"] = torch.empty(n_pseudo, dtype=torch.float32, device=dev)
            check(self.lib.psvi_outer_elbo_grad_coef_ex(
                self.handle, n_pseudo, _ptr(x_all), _ptr(z_all), _ptr(w_all), _ptr(eps),
                _ptr(params), _ptr(coef), _ptr(out["grad"]), _ptr(out.get("grad_u")),
                _ptr(out.get("grad_w")), _ptr(out["grad_z"]), _ptr(ws), ws.numel(), _stream()),
                "psvi_outer_elbo_grad_coef_ex")
            _wrote(ws)
            return out
        check(self.lib.psvi_outer_elbo_grad_coef(
            self.handle, n_pseudo, _ptr(x_all), _ptr(z_all), _ptr(w_all), _ptr(eps),
            _ptr(params), _ptr(coef), _ptr(out["grad"]), _ptr(out.get("grad_u")),
            _ptr(out.get("grad_w")), _ptr(ws), ws.numel(), _stream()),
            "psvi_outer_elbo_grad_coef")
        _wrote(ws)
        return out

    def evaluate(self, n_pseudo, x_all, z_all, w_all, eps, params, correction=True, probs=False,
                 ws=None):
        """Importance-weighted predictive evaluation of the data rows of this
        plan's M rows (psvi_evaluate).  Returns (stats, probs): stats a float64
        device tensor [entropy of W, normalised ESS, correct, summed NLL];
        probs ([M - n_pseudo, C]) when requested."""
        D, C = self.in_features, self.layers[-1][1]
        _need(x_all, "x_all", self.M * D)
        _need(z_all, "z_all", self.M, self._zdtype)
        _need(w_all, "w_all", self.M)
        _need(eps, "eps", self.eps_count)
        _need(params, "params", self.param_count)
        dev = params.device
        stats = torch.empty(4, dtype=torch.float64, device=dev)
        pr = torch.empty(self.M - int(n_pseudo), C, dtype=torch.float32, device=dev) if probs else None
        if ws is None or ws.numel() < self.eval_ws_bytes:
            ws = torch.empty(self.eval_ws_bytes, dtype=torch.uint8, device=dev)
        check(self.lib.psvi_evaluate(self.handle, int(n_pseudo), _ptr(x_all), _ptr(z_all),
                                     _ptr(w_all), _ptr(eps), _ptr(params), int(bool(correction)),
                                     _ptr(pr), _ptr(stats), _ptr(ws), ws.numel(), _stream()),
              "psvi_evaluate")
        _wrote(ws)
        return stats, pr

    def evaluate_regression(self, n_pseudo, x_all, y_all, w_all, eps, params, y_mean=0.0,
                            y_std=1.0, correction=True, pred=False, ws=None):
        """The regressors' predictive evaluation of the data rows of this plan's
        M rows (psvi_evaluate_regression, Gaussian plans): y_all holds the
        pseudo targets, then the test targets in original units.  Returns
        (stats, pred): stats a float64 device tensor [entropy of W, normalised
        ESS, summed squared error, summed test log-likelihood]; pred
        ([M - n_pseudo], the de-normalised predictive mean) when requested."""
        if self.likelihood != "gaussian":
            raise ValueError("evaluate_regression needs a Gaussian-likelihood plan")
        _need(x_all, "x_all", self.M * self.in_features)
        _need(y_all, "y_all", self.M)
        _need(w_all, "w_all", self.M)
        _need(eps, "eps", self.eps_count)
        _need(params, "params", self.param_count)
        dev = params.device
        stats = torch.empty(4, dtype=torch.float64, device=dev)
        pr = torch.empty(self.M - int(n_pseudo), dtype=torch.float32, device=dev) if pred else None
        if ws is None or ws.numel() < self.eval_ws_bytes:
            ws = torch.empty(self.eval_ws_bytes, dtype=torch.uint8, device=dev)
        check(self.lib.psvi_evaluate_regression(
            self.handle, int(n_pseudo), _ptr(x_all), _ptr(y_all), _ptr(w_all), _ptr(eps),
            _ptr(params), int(bool(correction)), float(y_mean), float(y_std), _ptr(pr),
            _ptr(stats), _ptr(ws), ws.numel(), _stream()), "psvi_evaluate_regression")
        _wrote(ws)
        return stats, pr

    def hvp(self, u, z, w, eps, params, vec, mixed=True, out=None, ws=None, include_kl=True):
        """Hessian-vector product of the negative inner ELBO at fixed eps
        (psvi_hvp).  Returns (hv, d_u, d_w): H vec and, with mixed=True, the
        mixed products d/du and d/dw of vec . grad (else None, None).
        include_kl=False: this plan's samples' share without the KL Hessian
        (psvi_hvp_partial, one rank of a sample-sharded product).  On a Gaussian
        plan mixed=True returns (hv, d_u, d_w, d_z), d_z the mixed product w.r.t.
        the targets (psvi_hvp_ex); mixed=False (hv, None, None, None)."""
        self._inputs(u, z, w, eps)
        _need(params, "params", self.param_count)
        _need(vec, "vec", self.param_count)
        dev = params.device
        hv = torch.empty(self.param_count, dtype=torch.float32, device=dev) if out is None else out
        _need(hv, "hv_out", self.param_count)
        du = torch.empty(self.M, self.in_features, dtype=torch.float32, device=dev) if mixed else None
        dw = torch.empty(self.M, dtype=torch.float32, device=dev) if mixed else None
        if ws is None or ws.numel() < self.hvp_ws_bytes:
            ws = torch.empty(self.hvp_ws_bytes, dtype=torch.uint8, device=dev)
        if self.likelihood == "gaussian":
            dz = torch.empty(self.M, dtype=torch.float32, device=dev) if mixed else None
            check(self.lib.psvi_hvp_ex(self.handle, _ptr(u), _ptr(z), _ptr(w), _ptr(eps),
                                       _ptr(params), _ptr(vec), int(bool(include_kl)), _ptr(hv),
                                       _ptr(du), _ptr(dw), _ptr(dz), _ptr(ws), ws.numel(),
                                       _stream()), "psvi_hvp_ex")
            _wrote(ws)
            return hv, du, dw, dz
        check(self.lib.psvi_hvp_partial(self.handle, _ptr(u), _ptr(z), _ptr(w), _ptr(eps),
                                        _ptr(params), _ptr(vec), int(bool(include_kl)), _ptr(hv),
                                        _ptr(du), _ptr(dw), _ptr(ws), ws.numel(), _stream()),
              "psvi_hvp_partial")
        _wrote(ws)
        return hv, du, dw

    # ------------------------------------------------------------ phases
    def mf_accumulate(self, u, z, w, eps, params, acc, nll_out):
        """acc <- [sum_s dW | sum_s dW*eps] (this rank's samples); nll_out += NLL."""
        self._inputs(u, z, w, eps)
        _need(params, "params", self.param_count)
        _need(acc, "acc", self.acc_count)
        _need(nll_out, "nll_out", 1, torch.float64)
        check(self.lib.psvi_mf_phase_accumulate(self.handle, _ptr(u), _ptr(z), _ptr(w),
                                                _ptr(eps), _ptr(params), _ptr(acc),
                                                _ptr(nll_out), _stream()),
              "psvi_mf_phase_accumulate")

    def mf_update(self, acc, params, adam_m=None, adam_v=None, step=1, lr=1e-3,
                  kind="higher", kl_out=None, grad_out=None, include_kl=True):
        _need(acc, "acc", self.acc_count)
        _need(params, "params", self.param_count)
        if kl_out is not None:
            _need(kl_out, "kl_out", 1, torch.float64)
        hp = make_adam(lr, step, kind)
        check(self.lib.psvi_mf_phase_update(self.handle, _ptr(acc), _ptr(params), _ptr(adam_m),
                                            _ptr(adam_v), ctypes.byref(hp), _ptr(kl_out),
                                            _ptr(grad_out), int(bool(include_kl)), _stream()),
              "psvi_mf_phase_update")
        _wrote(params, adam_m, adam_v)

    def mvn_sample(self, eps, params, x_shard):
        _need(eps, "eps", self.eps_count)
        _need(params, "params", self.param_count)
        _need(x_shard, "x_shard", self.xshard_count)
        check(self.lib.psvi_mvn_phase_sample(self.handle, _ptr(eps), _ptr(params),
                                             _ptr(x_shard), _stream()), "psvi_mvn_phase_sample")

    def tiled_state(self, device="cuda"):
        if not self.tiled_floats:
            raise ValueError("this plan has no tiled state (full-cov, world 1, S <= 128)")
        return torch.empty(self.tiled_floats, dtype=torch.float32, device=device)

    def tiled_convert(self, params, adam_m, adam_v, tstate, to_tiled):
        for t, n in ((params, "params"), (adam_m, "adam_m"), (adam_v, "adam_v")):
            _need(t, n, self.param_count)
        _need(tstate, "tstate", self.tiled_floats)
        check(self.lib.psvi_mvn_tiled_convert(self.handle, _ptr(params), _ptr(adam_m),
                                              _ptr(adam_v), _ptr(tstate), int(bool(to_tiled)),
                                              _stream()), "psvi_mvn_tiled_convert")
        _wrote(params, adam_m, adam_v, tstate)

    def mvn_update_tiled(self, eps, g_shard, params, adam_m, adam_v, tstate, step, lr,
                         kind="higher", kl_out=None, include_kl=True, eps_next=None,
                         x_next=None):
        _need(eps, "eps", self.eps_count)
        _need(g_shard, "g_shard", self.xshard_count)
        for t, n in ((params, "params"), (adam_m, "adam_m"), (adam_v, "adam_v")):
            _need(t, n, self.param_count)
        _need(tstate, "tstate", self.tiled_floats)
        if kl_out is not None:
            _need(kl_out, "kl_out", 1, torch.float64)
        if (eps_next is None) != (x_next is None):
            raise ValueError("eps_next and x_next go together")
        if eps_next is not None:
            _need(eps_next, "eps_next", self.eps_count)
            _need(x_next, "x_next", self.xshard_count)
        hp = make_adam(lr, step, kind)
        check(self.lib.psvi_mvn_phase_update_tiled(
            self.handle, _ptr(eps), _ptr(g_shard), _ptr(params), _ptr(adam_m), _ptr(adam_v),
            _ptr(tstate), ctypes.byref(hp), _ptr(kl_out), int(bool(include_kl)), _ptr(eps_next),
            _ptr(x_next), _stream()), "psvi_mvn_phase_update_tiled")
        _wrote(params, adam_m, adam_v, tstate)

    def mvn_net(self, u, z, w, x_recv, g_send, nll_out, draw=None, samples=None, draw_part=(0, 1)):
        """draw = (eps_out, seed, offset): the next step's global eps drawn in the
        same launch (psvi_mvn_phase_net_draw; psvi_randn's values).  samples =
        (s_begin, s_count): only those local samples (psvi_mvn_phase_net_part),
        with part draw_part[0] of draw_part[1] of the draw."""
        _need(u, "u", self.M * self.in_features)
        _need(z, "z", self.M, self._zdtype)
        _need(w, "w", self.M)
        _need(x_recv, "x_recv", self.xrecv_count)
        _need(g_send, "g_send", self.xrecv_count)
        _need(nll_out, "nll_out", 1, torch.float64)
        if samples is not None:
            out, seed, offset = draw if draw is not None else (None, 0, 0)
            n = 0 if out is None else out.numel()
            check(self.lib.psvi_mvn_phase_net_part(
                self.handle, _ptr(u), _ptr(z), _ptr(w), _ptr(x_recv), _ptr(g_send), _ptr(nll_out),
                int(samples[0]), int(samples[1]), _ptr(out), n, int(seed), int(offset),
                int(draw_part[0]), int(draw_part[1]), _stream()), "psvi_mvn_phase_net_part")
            return
        if draw is None:
            check(self.lib.psvi_mvn_phase_net(self.handle, _ptr(u), _ptr(z), _ptr(w), _ptr(x_recv),
                                              _ptr(g_send), _ptr(nll_out), _stream()),
                  "psvi_mvn_phase_net")
            return
        out, seed, offset = draw
        _need(out, "eps_out", out.numel())
        check(self.lib.psvi_mvn_phase_net_draw(self.handle, _ptr(u), _ptr(z), _ptr(w), _ptr(x_recv),
                                               _ptr(g_send), _ptr(nll_out), _ptr(out), out.numel(),
                                               int(seed), int(offset), _stream()),
              "psvi_mvn_phase_net_draw")

    def mvn_update(self, eps, g_shard, params, adam_m=None, adam_v=None, step=1, lr=1e-3,
                   kind="higher", kl_out=None, grad_out=None, include_kl=True, eps_next=None,
                   x_next=None):
        """Full-cov update phase; with eps_next / x_next also the next step's
        sample from the updated parameters (psvi_mvn_phase_update_sample)."""
        _need(eps, "eps", self.eps_count)
        _need(g_shard, "g_shard", self.xshard_count)
        _need(params, "params", self.param_count)
        if kl_out is not None:
            _need(kl_out, "kl_out", 1, torch.float64)
        hp = make_adam(lr, step, kind)
        if eps_next is not None or x_next is not None:
            if grad_out is not None:
                raise ValueError("the fused next-step sample runs with the Adam update only")
            _need(eps_next, "eps_next", self.eps_count)
            _need(x_next, "x_next", self.xshard_count)
            check(self.lib.psvi_mvn_phase_update_sample(
                self.handle, _ptr(eps), _ptr(g_shard), _ptr(params), _ptr(adam_m), _ptr(adam_v),
                ctypes.byref(hp), _ptr(kl_out), int(bool(include_kl)), _ptr(eps_next),
                _ptr(x_next), _stream()), "psvi_mvn_phase_update_sample")
            _wrote(params, adam_m, adam_v)
            return
        check(self.lib.psvi_mvn_phase_update(self.handle, _ptr(eps), _ptr(g_shard),
                                             _ptr(params), _ptr(adam_m), _ptr(adam_v),
                                             ctypes.byref(hp), _ptr(kl_out), _ptr(grad_out),
                                             int(bool(include_kl)), _stream()),
              "psvi_mvn_phase_update")
        _wrote(params, adam_m, adam_v)


def check_binary(z, name="z"):
    """The host's range check of a Bernoulli plan's labels: class ids in {0, 1}."""
    if z.is_floating_point() and not torch.equal(z, z.round()):
        raise ValueError(f"{name} must hold class ids")
    if z.numel() and not bool(((z == 0) | (z == 1)).all()):
        raise ValueError(f"{name} must hold class ids in {{0, 1}} (Bernoulli likelihood)")


def _ll_shape(ll, nkl, n_core, n_data):
    if ll is None or ll.dim() != 2:
        raise ValueError("ll must be the (S, n_core + n_data) tensor of row_loglik")
    S = int(ll.shape[0])
    _need(ll, "ll", S * (int(n_core) + int(n_data)))
    _need(nkl, "nkl", S, torch.float64)
    return S


def select_scores(ll, nkl, w_core, n_core, sum_scaling):
    """Greedy selection scores of sparse black-box VI (psvi_select_scores) from
    row_loglik's ll (S, n_core + n_data; core columns first) and nkl.  Returns a
    dict of device tensors: W (S), corr (n_data), corecorr (n_core, None at 0)
    and result (4 float64: max corr, its first arg, max corecorr, attach)."""
    n_core = int(n_core)
    n_data = int(ll.shape[1]) - n_core
    S = _ll_shape(ll, nkl, n_core, n_data)
    if n_core:
        _need(w_core, "w_core", n_core)
    dev = ll.device
    out = {"W": torch.empty(S, dtype=torch.float32, device=dev),
           "corr": torch.empty(n_data, dtype=torch.float32, device=dev),
           "corecorr": torch.empty(n_core, dtype=torch.float32, device=dev) if n_core else None,
           "result": torch.empty(4, dtype=torch.float64, device=dev)}
    check(_lib.load().psvi_select_scores(S, n_core, n_data, _ptr(ll), _ptr(nkl),
                                         _ptr(w_core) if n_core else None, float(sum_scaling),
                                         _ptr(out["W"]), _ptr(out["corr"]), _ptr(out["corecorr"]),
                                         _ptr(out["result"]), _stream()), "psvi_select_scores")
    return out


def select_weight_grad(ll, nkl, w_core, N):
    """sparsevi_psvi_elbo and its gradient w.r.t. the core weights
    (psvi_select_weight_grad): returns (loss (1,) float64, grad_w (n_core,))."""
    n_core = int(w_core.numel())
    n_data = int(ll.shape[1]) - n_core
    S = _ll_shape(ll, nkl, n_core, n_data)
    _need(w_core, "w_core", n_core)
    loss = torch.empty(1, dtype=torch.float64, device=ll.device)
    gw = torch.empty(n_core, dtype=torch.float32, device=ll.device)
    check(_lib.load().psvi_select_weight_grad(S, n_core, n_data, _ptr(ll), _ptr(nkl),
                                              _ptr(w_core), float(N), _ptr(loss), _ptr(gw),
                                              _stream()), "psvi_select_weight_grad")
    return loss, gw


def laplace_fit(x_core, y_core, w_core, theta, T, lr, eps=None, prior_mean=0.0, prior_sd=1.0,
                betas=(0.9, 0.999), adam_eps=1e-8, want_loss=False):
    """The Laplace fit of the coreset baselines (psvi_laplace_fit): T torch-Adam
    steps from fresh moments on theta (d,), updated in place, for the weighted
    logistic log-joint of x_core (n_core, d; the ones column included), float
    labels y_core and weights w_core >= 0 (all None for an empty core).
    Returns a dict of device tensors: prec (d), samples (S, d; None without
    eps (S, d)) and loss (T float64: the negative log-joint before each step;
    None unless want_loss)."""
    d = int(theta.numel())
    _need(theta, "theta", d)
    n_core = 0 if x_core is None else int(x_core.shape[0])
    if n_core:
        _need(x_core, "x_core", n_core * d)
        _need(y_core, "y_core", n_core)
        _need(w_core, "w_core", n_core)
    S = 0
    dev = theta.device
    if eps is not None:
        if eps.dim() != 2:
            raise ValueError("eps must be the (S, d) tensor of draws")
        S = int(eps.shape[0])
        _need(eps, "eps", S * d)
    out = {"prec": torch.empty(d, dtype=torch.float32, device=dev),
           "samples": torch.empty(S, d, dtype=torch.float32, device=dev) if S else None,
           "loss": torch.empty(int(T), dtype=torch.float64, device=dev) if want_loss else None}
    on = bool(n_core)
    req = _lib.LaplaceFitReq(
        n_core, d, S, int(T), _ptr(x_core if on else None), _ptr(y_core if on else None),
        _ptr(w_core if on else None), float(prior_mean), float(prior_sd), _ptr(theta), float(lr),
        float(betas[0]), float(betas[1]), float(adam_eps), _ptr(eps), _ptr(out["loss"]),
        _ptr(out["prec"]), _ptr(out["samples"]))
    check(_lib.load().psvi_laplace_fit(ctypes.byref(req), _stream()), "psvi_laplace_fit")
    _wrote(theta)
    return out


def _mfvi_desc(layers, S, B, prior_sd):
    layers = [tuple(int(x) for x in l) for l in layers]
    if not 1 <= len(layers) <= _lib.MAX_LAYERS:
        raise ValueError("1..8 layers supported")
    for a, b in zip(layers[:-1], layers[1:]):
        if a[1] != b[0]:
            raise ValueError(f"layer sizes do not chain: {layers}")
    d = NetDesc()
    d.n_layers = len(layers)
    for i, v in enumerate([layers[0][0]] + [o for _, o in layers]):
        d.dims[i] = v
    d.S, d.M, d.prior_sd = int(S), int(B), float(prior_sd)
    return d


def mfvi_fit_query(layers, S, B, prior_sd=1.0):
    """What psvi_mfvi_fit does with a network (psvi_mfvi_fit_query; no device
    needed): a dict with placement ("lds": params / adam_m / adam_v, the
    gradient accumulators and the batch stay in LDS; "global": they are read
    and written in global memory), ws_bytes (per member), param_count and
    eps_count."""
    d = _mfvi_desc(layers, S, B, prior_sd)
    out = (ctypes.c_int64 * 4)()
    check(_lib.load().psvi_mfvi_fit_query(ctypes.byref(d), out), "psvi_mfvi_fit_query")
    return {"placement": "lds" if out[0] else "global", "ws_bytes": int(out[1]),
            "param_count": int(out[2]), "eps_count": int(out[3])}


def mfvi_fit(layers, S, x, y, scale, taus, params, T, lr, adam_m=None, adam_v=None, step0=0,
             eps=None, seed=0, offsets=None, prior_sd=1.0, betas=(0.9, 0.999), adam_eps=1e-8,
             want_loss=True):
    """The fit of the MFVI regression baselines (psvi_mfvi_fit): T chained steps
    of a mean-field Gaussian-likelihood MLP (layers [(in, out), ...], one
    output, S samples) on the fixed batch x (B, D) / y (B), loss = scale *
    sum_{s,b} NLL(tau_g) + KL, each followed by one torch.optim.Adam step, for
    G = len(taus) independent members in one launch.  params (G, P) is updated
    in place; adam_m / adam_v (G, P; zeros when None: a new fit) too, with
    step0 the Adam steps already taken.  eps: (G, T, eps_count) device tensor
    in the library's eps layout, or None for the Philox stream: member g's step
    t takes what randn_(seed, offsets[g] + t * round_up(eps_count, 4)) writes
    (offsets: G multiples of 4; default 0).  Returns a dict of device tensors:
    params, adam_m, adam_v (the tensors updated in place) and loss (G, T
    float64: the loss before each step; None unless want_loss)."""
    taus = [float(v) for v in taus]
    G, T = len(taus), int(T)
    if x is None or x.dim() != 2:
        raise ValueError("x must be the (B, D) batch")
    B = int(x.shape[0])
    q = mfvi_fit_query(layers, S, B, prior_sd)
    P, E = q["param_count"], q["eps_count"]
    _need(x, "x", B * int(layers[0][0]))
    _need(y, "y", B)
    _need(params, "params", G * P)
    dev = params.device
    if adam_m is None:
        adam_m = torch.zeros(G, P, dtype=torch.float32, device=dev)
    if adam_v is None:
        adam_v = torch.zeros(G, P, dtype=torch.float32, device=dev)
    _need(adam_m, "adam_m", G * P)
    _need(adam_v, "adam_v", G * P)
    if eps is not None:
        _need(eps, "eps", G * T * E)
    if offsets is None:
        offsets = [0] * G
    if len(offsets) != G:
        raise ValueError("offsets must hold one Philox offset per member")
    tau_h = (ctypes.c_float * G)(*taus)
    off_h = (ctypes.c_uint64 * G)(*[int(o) for o in offsets])
    loss = torch.empty(G, T, dtype=torch.float64, device=dev) if want_loss else None
    ws = torch.empty(max(G * q["ws_bytes"], 1), dtype=torch.uint8, device=dev)
    d = _mfvi_desc(layers, S, B, prior_sd)
    req = _lib.MfviFitReq(
        ctypes.pointer(d), G, T, int(step0), _ptr(x), _ptr(y), float(scale),
        ctypes.cast(tau_h, ctypes.c_void_p), _ptr(params), _ptr(adam_m), _ptr(adam_v), float(lr),
        float(betas[0]), float(betas[1]), float(adam_eps), _ptr(eps), int(seed) & (2**64 - 1),
        ctypes.cast(off_h, ctypes.c_void_p), _ptr(loss), _ptr(ws), ws.numel())
    check(_lib.load().psvi_mfvi_fit(ctypes.byref(req), _stream()), "psvi_mfvi_fit")
    _wrote(params, adam_m, adam_v)
    return {"params": params, "adam_m": adam_m, "adam_v": adam_v, "loss": loss}


def laplace_sample_full(x_core, w_core, theta, eps=None, want_prec=False, want_factor=False,
                        want_logdet=False):
    """Samples from the full-precision Laplace posterior at the fitted mode
    theta (d,) (psvi_laplace_sample_full): P = I + x^T diag(w p (1 - p)) x for
    x_core (n_core, d; the ones column included) and w_core >= 0 (both None for
    an empty core), A lower-triangular with A^T A = P, and theta + A^-1 eps_s
    for eps (S, d) -- what MultivariateNormal(theta, precision_matrix=P) draws
    from the same noise.  Returns a dict of device tensors: samples (S, d; None
    without eps) and, on request (None otherwise), prec (d, d), factor (d, d:
    A) and logdet (1 float64: log det P)."""
    d = int(theta.numel())
    _need(theta, "theta", d)
    n_core = 0 if x_core is None else int(x_core.shape[0])
    if n_core:
        _need(x_core, "x_core", n_core * d)
        _need(w_core, "w_core", n_core)
    S = 0
    dev = theta.device
    if eps is not None:
        if eps.dim() != 2:
            raise ValueError("eps must be the (S, d) tensor of draws")
        S = int(eps.shape[0])
        _need(eps, "eps", S * d)

    def new(*shape, on=True, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=dev) if on else None

    out = {"samples": new(S, d, on=S > 0), "prec": new(d, d, on=want_prec),
           "factor": new(d, d, on=want_factor),
           "logdet": new(1, on=want_logdet, dtype=torch.float64)}
    on = bool(n_core)
    req = _lib.LaplaceSampleFullReq(
        n_core, d, S, _ptr(x_core if on else None), _ptr(w_core if on else None), _ptr(theta),
        _ptr(eps if S else None), _ptr(out["prec"]), _ptr(out["factor"]), _ptr(out["samples"]),
        _ptr(out["logdet"]))
    check(_lib.load().psvi_laplace_sample_full(ctypes.byref(req), _stream()),
          "psvi_laplace_sample_full")
    return out


def laplace_scores(samples, rows, labels, w_core, n_core, sum_scaling, want_grad_w=False,
                   want_ll=False, want_grad_u=False):
    """Selection scores and gradients of the Laplace baselines
    (psvi_laplace_scores) from samples (S, d), rows (n_core + n_data, d; core
    rows first), their float labels and w_core.  Returns a dict of device
    tensors: corr (n_data), corecorr (n_core, None at 0), result (4 float64:
    max corr, its first arg, max corecorr, attach) and, on request, grad_w
    (n_core), ll (S, n_core + n_data) and grad_u (n_core, d)."""
    if samples is None or samples.dim() != 2 or rows is None or rows.dim() != 2:
        raise ValueError("samples must be (S, d) and rows (n_core + n_data, d)")
    S, d = int(samples.shape[0]), int(samples.shape[1])
    n_core = int(n_core)
    M = int(rows.shape[0])
    n_data = M - n_core
    _need(samples, "samples", S * d)
    _need(rows, "rows", M * d)
    _need(labels, "labels", M)
    if n_core:
        _need(w_core, "w_core", n_core)
    dev = samples.device

    def new(*shape, on=True, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=dev) if on else None

    out = {"corr": new(max(n_data, 0)), "corecorr": new(n_core, on=n_core > 0),
           "result": new(4, dtype=torch.float64),
           "grad_w": new(n_core, on=want_grad_w and n_core > 0),
           "ll": new(S, M, on=want_ll), "grad_u": new(n_core, d, on=want_grad_u and n_core > 0)}
    req = _lib.LaplaceScoresReq(
        S, d, n_core, n_data, _ptr(samples), _ptr(rows), _ptr(labels),
        _ptr(w_core if n_core else None), float(sum_scaling), _ptr(out["corr"]),
        _ptr(out["corecorr"]), _ptr(out["result"]), _ptr(out["grad_w"]), _ptr(out["ll"]),
        _ptr(out["grad_u"]))
    check(_lib.load().psvi_laplace_scores(ctypes.byref(req), _stream()), "psvi_laplace_scores")
    return out


def giga_step(samples, rows, labels, lw, want_ll=False):
    """One geodesic-ascent step of GIGA (psvi_giga_step) from samples (S, d),
    the minibatch rows (n_data, d; the ones column included), their float
    labels and lw (S: the coreset's unit vector, zeros before the first step).
    Returns a dict of device tensors: score (n_data), lw (S: the new vector),
    result (8 float64: max score, its first arg, zeta0, zeta1, zeta2, gamma,
    scale, L) and, on request, ll (S, n_data)."""
    if samples is None or samples.dim() != 2 or rows is None or rows.dim() != 2:
        raise ValueError("samples must be (S, d) and rows (n_data, d)")
    S, d = int(samples.shape[0]), int(samples.shape[1])
    n_data = int(rows.shape[0])
    _need(samples, "samples", S * d)
    _need(rows, "rows", n_data * d)
    _need(labels, "labels", n_data)
    _need(lw, "lw", S)
    dev = samples.device
    out = {"score": torch.empty(n_data, dtype=torch.float32, device=dev),
           "lw": torch.empty(S, dtype=torch.float32, device=dev),
           "result": torch.empty(8, dtype=torch.float64, device=dev),
           "ll": torch.empty(S, n_data, dtype=torch.float32, device=dev) if want_ll else None}
    req = _lib.GigaStepReq(S, d, n_data, _ptr(samples), _ptr(rows), _ptr(labels), _ptr(lw),
                           _ptr(out["score"]), _ptr(out["lw"]), _ptr(out["ll"]),
                           _ptr(out["result"]))
    check(_lib.load().psvi_giga_step(ctypes.byref(req), _stream()), "psvi_giga_step")
    return out


PREDICT_OUTPUTS = ("mean_logits", "least_conf", "entropy", "el2n", "correct")
_PREDICT_NEED_Z = ("el2n", "correct")


def predict_scores(plan, x, z, eps, params, rows_per_draw, want=PREDICT_OUTPUTS, state=None,
                   stats=False):
    """The scoring pass of the MFVI selection baselines (psvi_predict_scores):
    the mean-logit forward of a mean-field categorical plan over the rows x
    (n_rows, D) in one launch, rows [k rpd, (k + 1) rpd) on eps block k of eps
    (ceil(n_rows / rpd) blocks of plan.eps_count floats).  ``want`` names the
    per-row outputs (PREDICT_OUTPUTS); ``state`` = (last_acc, forgetting,
    never_learnt), three float32 (n_rows,) device tensors, is updated in place
    as MeanFieldVI.after_epoch does; ``stats=True`` adds ``stats`` (2 float64:
    the number of correct rows, sum_j -log p_j[z_j]).  z (int32 class ids) may
    be None when nothing asked for reads labels; a label outside [0, C) is
    refused here (PSVI_EINVAL), the one check the library leaves to its caller.
    Returns a dict of device tensors."""
    if not isinstance(plan, InnerLoopPlan):
        raise ValueError("plan must be an InnerLoopPlan")
    want = tuple(want)
    bad = [k for k in want if k not in PREDICT_OUTPUTS]
    if bad:
        raise ValueError(f"unknown outputs {bad}: choose from {PREDICT_OUTPUTS}")
    rpd = int(rows_per_draw)
    if x is None or x.dim() != 2 or int(x.shape[0]) < 1:
        raise ValueError("x must be (n_rows, D) with n_rows >= 1")
    if rpd < 1:
        raise ValueError("rows_per_draw must be >= 1")
    n_rows, C = int(x.shape[0]), plan.layers[-1][1]
    _need(x, "x", n_rows * plan.in_features)
    _need(eps, "eps", -(-n_rows // rpd) * plan.eps_count)
    _need(params, "params", plan.param_count)
    if state is not None:
        if len(state) != 3:
            raise ValueError("state is (last_acc, forgetting, never_learnt)")
        for t, nm in zip(state, ("last_acc", "forgetting", "never_learnt")):
            _need(t, nm, n_rows)
    need_z = stats or state is not None or any(k in _PREDICT_NEED_Z for k in want)
    if z is not None:
        _need(z, "z", n_rows, torch.int32)
        if need_z and (int(z.min()) < 0 or int(z.max()) >= C):
            raise _lib.PsviError(f"psvi_predict_scores failed (PSVI_EINVAL): a label lies outside "
                                 f"[0, {C})")
    dev = x.device
    out = {k: torch.empty((n_rows, C) if k == "mean_logits" else (n_rows,), dtype=torch.float32,
                          device=dev) for k in want}
    if stats:
        out["stats"] = torch.empty(2, dtype=torch.float64, device=dev)
    st = state if state is not None else (None, None, None)
    req = _lib.PredictScoresReq(plan.handle, n_rows, rpd, _ptr(x), _ptr(z), _ptr(eps), _ptr(params),
                                *(_ptr(out.get(k)) for k in PREDICT_OUTPUTS),
                                *(_ptr(t) for t in st), _ptr(out.get("stats")))
    check(plan.lib.psvi_predict_scores(ctypes.byref(req), _stream()), "psvi_predict_scores")
    _wrote(*st)
    return out


def predict_query(plan, rows_per_draw):
    """How psvi_predict_scores cuts a plan's work at rows_per_draw
    (psvi_predict_query; no device needed): a dict with rows_per_group,
    tile_floats (the W tile in LDS) and units_per_tile (per layer; less than
    the layer's width where the layer runs in several tiles)."""
    if not isinstance(plan, InnerLoopPlan):
        raise ValueError("plan must be an InnerLoopPlan")
    out = (ctypes.c_int64 * (2 + _lib.MAX_LAYERS))()
    check(plan.lib.psvi_predict_query(plan.handle, int(rows_per_draw), out), "psvi_predict_query")
    return {"rows_per_group": int(out[0]), "tile_floats": int(out[1]),
            "units_per_tile": [int(out[2 + l]) for l in range(len(plan.layers))]}


DRAW_STATUS = {1:"a weight is negative or not finite", 2: "the weights sum to zero",
               3: "fewer positive weights than rows to draw without replacement"}


def coreset_draw(w, n, replacement, seed, offset, rows=None, targets=None):
    """n coreset indices drawn in proportion to the weights w (M floats) on the
    Philox stream (seed, offset) (psvi_coreset_draw): independently
    (replacement=True, inverse CDF) or n distinct ones in the order they are
    drawn (replacement=False, Efraimidis-Spirakis keys).  rows (M, D float32) /
    targets (M, int32 or float32) are gathered by the indices on the device.
    Returns (idx int32 (n), rows_out or None, targets_out or None, consumed):
    consumed is the length of the stream the draw used, 4 ceil(n / 4) with and
    4 ceil(M / 4) without replacement -- add it to offset for the next draw.
    Reads the status word once on the host; raises ValueError naming the
    condition when the weights admit no such draw."""
    if w is None or w.dim() != 1:
        raise ValueError("w must be a vector of M weights")
    M, n = int(w.numel()), int(n)
    _need(w, "w", M)
    if M < 1 or n < 1 or n > _lib.DRAW_MAX_N:
        raise ValueError(f"coreset_draw: M >= 1 and 1 <= n <= 2^24 (got M = {M}, n = {n})")
    if not replacement and n > M:
        raise ValueError(f"cannot draw {n} distinct rows out of {M}")
    dev = w.device
    D, rows_out, targets_out = 0, None, None
    if rows is not None:
        if rows.dim() != 2 or int(rows.shape[0]) != M:
            raise ValueError(f"rows must be ({M}, D)")
        D = int(rows.shape[1])
        _need(rows, "rows", M * D)
        rows_out = torch.empty(n, D, dtype=torch.float32, device=dev)
    if targets is not None:
        if targets.dtype not in (torch.int32, torch.float32):
            raise ValueError("targets must be int32 or float32 (4-byte slots)")
        _need(targets, "targets", M, targets.dtype)
        targets_out = torch.empty(n, dtype=targets.dtype, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    req = _lib.CoresetDrawReq(
        _ptr(w), M, n, _lib.DRAW_REPLACE if replacement else _lib.DRAW_NOREPLACE,
        int(seed) & (2**64 - 1), int(offset), _ptr(rows) if D > 0 else None, D, _ptr(targets),
        _ptr(idx), _ptr(rows_out) if D > 0 else None, _ptr(targets_out), _ptr(status))
    check(_lib.load().psvi_coreset_draw(ctypes.byref(req), _stream()), "psvi_coreset_draw")
    st = int(status.item())
    if st:
        raise ValueError(f"coreset_draw: {DRAW_STATUS.get(st, f'status {st}')}")
    return idx, rows_out, targets_out, 4 * (((n if replacement else M) + 3) // 4)


KMEANS_STATUS = {1: "a row or a given centre is not finite",
                 2: "fewer than K distinct rows: every remaining distance to the chosen centres "
                    "is zero"}
KMEANS_WS_CAP = 256 << 20    # the wrapper's workspace: the one-pass sums up to this many bytes


def kmeans_query(N, D, K):
    """(one-pass ws bytes, least ws bytes, columns of an LDS tile, assignment
    workgroups) of psvi_kmeans at a shape; needs no device."""
    out = (ctypes.c_int64 * 4)()
    check(_lib.load().psvi_kmeans_query(int(N), int(D), int(K), out), "psvi_kmeans_query")
    return tuple(int(v) for v in out)


def kmeans(x, K, seed=0, offset=0, centres=None, max_iter=300, tol=0.0, ws_bytes=None):
    """K-means of the rows x (N, D float32 on the device) in fp64 (psvi_kmeans):
    k-means++ seeding with one candidate per centre on the Philox stream
    (seed, offset) -- or the given initial ``centres`` (K, D float64) -- then
    Lloyd iterations until no label changes, the summed squared centre shift
    is <= tol, or max_iter updates.  An empty cluster keeps its centre.
    ``ws_bytes`` picks the workspace (default: the one-pass sums when they
    take at most KMEANS_WS_CAP bytes, else that many bytes of partials).
    Returns a dict of device tensors ``centres`` (K, D float64), ``labels``
    (N int32), ``counts`` (K int32), ``seeds`` (K int32: the rows the seeding
    chose, -1 with given centres), and host numbers ``inertia``, ``n_iter``,
    ``consumed`` (the words of the stream used: 4 K, 0 with given centres --
    add it to offset for the next call).  Reads the status once on the host;
    raises ValueError naming the condition when the rows admit no clustering."""
    if x is None or x.dim() != 2:
        raise ValueError("x must be (N, D)")
    N, D, K = int(x.shape[0]), int(x.shape[1]), int(K)
    _need(x, "x", N * D)
    full, least, _, _ = kmeans_query(N, D, K)
    if ws_bytes is None:
        ws_bytes = min(full, max(least, KMEANS_WS_CAP))
    dev = x.device
    if centres is not None:
        _need(centres, "centres", K * D, torch.float64)
    out = dict(centres=torch.empty(K, D, dtype=torch.float64, device=dev),
               labels=torch.empty(N, dtype=torch.int32, device=dev),
               counts=torch.empty(K, dtype=torch.int32, device=dev),
               seeds=torch.empty(K, dtype=torch.int32, device=dev))
    inertia = torch.empty(1, dtype=torch.float64, device=dev)
    small = torch.empty(2, dtype=torch.int32, device=dev)     # n_iter, status
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
    req = _lib.KmeansReq(
        _ptr(x), N, D, K, _ptr(centres), int(seed) & (2**64 - 1), int(offset), int(max_iter),
        float(tol), _ptr(out["centres"]), _ptr(out["labels"]), _ptr(out["counts"]),
        _ptr(out["seeds"]), _ptr(inertia), _ptr(small), _ptr(small[1:]), _ptr(ws), int(ws_bytes))
    check(_lib.load().psvi_kmeans(ctypes.byref(req), _stream()), "psvi_kmeans")
    n_iter, st = small.tolist()
    if st:
        raise ValueError(f"kmeans: {KMEANS_STATUS.get(st, f'status {st}')}")
    out.update(inertia=float(inertia.item()), n_iter=int(n_iter),
               consumed=0 if centres is not None else 4 * K)
    return out


def randn_(out, seed, offset=0):
    """Fill a float32 device tensor with N(0,1) (Philox4x32-10 + Box-Muller)."""
    _need(out, "out", None)
    lib = _lib.load()
    check(lib.psvi_randn(_ptr(out), out.numel(), int(seed) & (2**64 - 1),
                         int(offset), _stream()), "psvi_randn")
    return out


def nonfinite_(flag, *tensors):
    """flag (device int32, 1 element) |= 1 if any value of the float32 /
    float64 device tensors is NaN or +-inf (psvi_nonfinite; no host sync)."""
    _need(flag, "flag", 1, torch.int32)
    lib = _lib.load()
    for t in tensors:
        if t is None:
            continue
        if t.dtype not in (torch.float32, torch.float64) or not t.is_cuda or not t.is_contiguous():
            raise ValueError("nonfinite_: contiguous float32 / float64 device tensors")
        check(lib.psvi_nonfinite(_ptr(t), t.numel(), int(t.dtype == torch.float64), _ptr(flag),
                                 _stream()), "psvi_nonfinite")
    return flag


def adam_adjoint_(lt, lm, lv, adam_m, adam_v, grad, step, lr, lg_out, kind="higher",
                  betas=(0.9, 0.999), eps=1e-8):
    """Reverse of one Adam step (psvi_adam_adjoint): lm, lv updated in place,
    lg_out <- adjoint of the step's gradient."""
    n = lt.numel()
    for t, nm in ((lt, "lt"), (lm, "lm"), (lv, "lv"), (adam_m, "adam_m"), (adam_v, "adam_v"),
                  (grad, "grad"), (lg_out, "lg_out")):
        _need(t, nm, n)
    hp = make_adam(lr, step, kind, betas, eps)
    lib = _lib.load()
    check(lib.psvi_adam_adjoint(n, _ptr(lt), _ptr(lm), _ptr(lv), _ptr(adam_m), _ptr(adam_v),
                                _ptr(grad), _ptr(lg_out), ctypes.byref(hp), _stream()),
          "psvi_adam_adjoint")
    return lg_out


def adam_update_(params, grad, adam_m, adam_v, step, lr, kind="higher", betas=(0.9, 0.999),
                 eps=1e-8):
    n = params.numel()
    for t, nm in ((params, "params"), (grad, "grad"), (adam_m, "adam_m"), (adam_v, "adam_v")):
        _need(t, nm, n)
    hp = make_adam(lr, step, kind, betas, eps)
    lib = _lib.load()
    check(lib.psvi_adam_update(n, _ptr(params), _ptr(grad), _ptr(adam_m), _ptr(adam_v),
                               ctypes.byref(hp), _stream()), "psvi_adam_update")
