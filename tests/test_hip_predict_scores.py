"""psvi_predict_scores on the device against the float64 restatement
(tests/mfvi_select_util.py).  Tolerances: mean logits within the project's
parity bound, 1e-4 relative (to the largest logit); each score within 1e-4
relative plus 1e-4 of its largest possible value (1, log C, sqrt 2); the
statistics 1e-4 relative.  ``correct`` is compared exactly on the rows whose
top-two mean-logit gap in float64 is at least 1e-3 (every row of the seeded
cases: asserted)."""
import itertools

import numpy as np
import pytest
import torch

import mfvi_select_util as R
from golden_util import rel

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALL = ("mean_logits", "least_conf", "entropy", "el2n", "correct")
CASES = {
    "logreg_one_row": dict(layers=[(5, 3)], S=3, n=1, rpd=1),
    "fn_131_rows": dict(layers=[(7, 9), (9, 3)], S=3, n=131, rpd=32),
    "two_hidden": dict(layers=[(7, 33), (33, 33), (33, 10)], S=5, n=70, rpd=70),
    "c2_s1": dict(layers=[(6, 5), (5, 2)], S=1, n=67, rpd=16),
}
# Past the first trip of the capped loops.  The item loop runs on at most
# kPredMaxGrid = 2048 workgroups and the statistics kernel's kPredThreads = 256
# threads stride over their partials: 2050 items, and 6151 rows in blocks of 3
# (2051 items, the last one ragged).  The sigma kernel covers 64 x 256 = 16,384
# elements of a layer per pass: 130 x 127 + 127 = 16,637.  A layer runs in
# several weight tiles when ut < dout: at 64 rows of 350 inputs a group's
# inputs leave the tile 28 of the 50 units (asserted from psvi_predict_query).
# "safe": the rows whose float64 top-two gap is >= 1e-3 at seed 0, counted with
# the restatement alone.
CAPPED = {
    "items_2050": dict(layers=[(5, 3)], S=2, n=2050, rpd=1, safe=2048),
    "items_6151_ragged": dict(layers=[(5, 3)], S=2, n=6151, rpd=3, safe=6148),
    "sigma_16637": dict(layers=[(130, 127), (127, 3)], S=1, n=5, rpd=5, safe=5),
    "two_tiles": dict(layers=[(350, 50), (50, 3)], S=2, n=70, rpd=64, safe=70),
}
CASES.update(CAPPED)


def _t(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _case(name, seed=0):
    c = CASES[name]
    rng = np.random.default_rng(seed)
    layers, S, n = c["layers"], c["S"], c["n"]
    params = []
    for din, dout in layers:
        k = din * dout + dout
        params += [rng.normal(size=k) * 0.8, rng.uniform(-3.0, -1.0, size=k)]
    nblk = -(-n // c["rpd"])
    return dict(c, params=np.concatenate(params).astype(np.float32),
                eps=rng.normal(size=nblk * R.eps_count(layers, S)).astype(np.float32),
                x=rng.normal(size=(n, layers[0][0])).astype(np.float32),
                z=rng.integers(0, layers[-1][1], size=n).astype(np.int32))


def _run(c, want=ALL, state=None, stats=True, z=True, params=None):
    from psvi.runtime import InnerLoopPlan, predict_scores

    plan = InnerLoopPlan("meanfield", c["layers"], c["S"], 3)  # M is not read
    out = predict_scores(plan, _t(c["x"]), _t(c["z"], torch.int32) if z else None, _t(c["eps"]),
                         _t(c["params"] if params is None else params), c["rpd"], want=want,
                         state=state, stats=stats)
    torch.cuda.synchronize()
    return out


def _check(out, ref, C, safe_rows=None):
    """safe_rows=None: every row's float64 top-two gap is at least 1e-3 and
    ``correct`` is compared on all of them.  safe_rows=k: exactly k rows have
    such a gap (counted on the CPU from the restatement for the case's seed),
    ``correct`` is compared on those and the correct count within the others."""
    caps = dict(least_conf=1.0, entropy=np.log(C), el2n=np.sqrt(2.0))
    assert rel(out["mean_logits"].cpu().numpy(), ref["mean_logits"]) < 1e-4
    for k, cap in caps.items():
        got = out[k].cpu().numpy().astype(np.float64)
        err = np.abs(got - ref[k])
        print(k, "max err", err.max())
        assert (err <= 1e-4 * np.abs(ref[k]) + 1e-4 * cap).all(), k
    safe = R.top2_gap(ref["mean_logits"]) >= 1e-3
    assert safe.all() if safe_rows is None else int(safe.sum()) == safe_rows
    correct = out["correct"].cpu().numpy()
    assert np.array_equal(correct[safe], ref["correct"][safe])
    st = out["stats"].cpu().numpy()
    assert st[0] == correct.sum() and abs(st[0] - ref["stats"][0]) <= (~safe).sum()
    assert abs(st[1] - ref["stats"][1]) <= 1e-4 * abs(ref["stats"][1])


@pytest.mark.parametrize("name", sorted(set(CASES) - set(CAPPED)))
def test_against_restatement(name):
    c = _case(name)
    ref = R.scores(R.mean_logits(c["layers"], c["S"], c["params"], c["eps"], c["x"], c["rpd"]),
                   c["z"])
    _check(_run(c), ref, c["layers"][-1][1])


@pytest.mark.parametrize("name", sorted(CAPPED))
def test_past_one_trip_against_restatement(name):
    """Every output on every row within _check's tolerances; ``correct`` on the
    rows with a top-two gap (at least 99 % of them: 2048 of 2050, 6148 of
    6151, all of the others).  Then the same launch without the statistics --
    no barrier then separates an item's scoring from the next item's staging
    -- gives the same bits on every row."""
    from psvi.runtime import InnerLoopPlan, predict_query

    c = _case(name)
    assert c["safe"] >= 0.99 * c["n"]
    q = predict_query(InnerLoopPlan("meanfield", c["layers"], c["S"], 3), c["rpd"])
    if name == "two_tiles":
        assert q["units_per_tile"][0] < c["layers"][0][1], q       # ut < dout: the tile loop
    if name == "sigma_16637":
        assert c["layers"][0][0] * c["layers"][0][1] + c["layers"][0][1] > 64 * 256
    if name.startswith("items"):
        items = -(-c["n"] // c["rpd"]) * -(-c["rpd"] // q["rows_per_group"])
        assert items > 2048
    ref = R.scores(R.mean_logits(c["layers"], c["S"], c["params"], c["eps"], c["x"], c["rpd"]),
                   c["z"])
    out = _run(c)
    _check(out, ref, c["layers"][-1][1], safe_rows=c["safe"])
    quiet = _run(c, stats=False)
    assert sorted(quiet) == sorted(ALL)
    for k in ALL:
        assert torch.equal(quiet[k], out[k]), k


def test_zero_row_under_zero_mean_net():
    """Equal logits: argmax 0, entropy log C, least confidence 1 - 1/C."""
    c = _case("fn_131_rows")
    k = sum(i * o + o for i, o in c["layers"])
    params = c["params"].copy()
    po = 0
    for din, dout in c["layers"]:
        n = din * dout + dout
        params[po:po + n] = 0.0        # means
        params[po + n - dout:po + n] = 0.0
        po += 2 * n
    assert po == 2 * k
    c["x"][5] = 0.0
    c["eps"][:] = 0.0  # the weights are their (zero) means: every logit is exactly 0
    c["z"][5] = 0
    out = _run(c, params=params)
    assert out["mean_logits"][5].abs().max().item() == 0.0
    assert out["correct"][5].item() == 1.0  # the first of equal maxima
    assert abs(out["entropy"][5].item() - np.log(3)) < 1e-6
    assert abs(out["least_conf"][5].item() - (1 - 1 / 3)) < 1e-6
    assert abs(out["el2n"][5].item() - np.sqrt(4 / 9 + 2 / 9)) < 1e-6


def test_saturated_softmax_has_zero_entropy():
    """Last bias means (0, 200, -200): p is exactly (0, 1, 0); entropy 0, not NaN."""
    c = _case("fn_131_rows")
    params = c["params"].copy()
    (d0, h), (_, C) = c["layers"]
    po = 2 * (d0 * h + h)
    n = h * C + C
    params[po:po + h * C] = 0.0
    params[po + h * C:po + n] = [0.0, 200.0, -200.0]
    params[po + n:po + 2 * n] = -30.0  # softplus(rho) ~ 1e-13
    c["z"][:] = 1
    out = _run(c, params=params)
    for k, v in (("entropy", 0.0), ("least_conf", 0.0), ("el2n", 0.0), ("correct", 1.0)):
        assert (out[k] == v).all(), k
    assert out["stats"].tolist() == [131.0, 0.0]
    c["z"][:] = 2
    out = _run(c, params=params)
    assert torch.isfinite(out["stats"]).all() and (out["correct"] == 0).all()
    assert abs(out["el2n"][0].item() - np.sqrt(2.0)) < 1e-6


def _state(n, seed=3):
    rng = np.random.default_rng(seed)
    return tuple(_t(a) for a in (rng.integers(0, 2, n), rng.integers(0, 3, n),
                                 rng.integers(0, 2, n)))


def test_output_subsets_agree_with_all_together():
    """Every non-empty subset of the five per-row outputs alone, the statistics
    alone, the state alone, and the state and the statistics next to every
    subset: the same bits as everything in one launch."""
    c = _case("fn_131_rows")
    full_state = _state(c["n"])
    full = _run(c, state=full_state)
    subsets = [w for r in range(1, 6) for w in itertools.combinations(ALL, r)]
    assert len(subsets) == 31
    for want in subsets:
        need_z = any(k in ("el2n", "correct") for k in want)
        out = _run(c, want=want, stats=False, z=need_z)
        assert sorted(out) == sorted(want)
        for k in want:
            assert torch.equal(out[k], full[k]), (want, k)
    only = _run(c, want=(), stats=True)
    assert sorted(only) == ["stats"] and torch.equal(only["stats"], full["stats"])
    st = _state(c["n"])
    assert _run(c, want=(), state=st, stats=False) == {}
    for a, b in zip(st, full_state):
        assert torch.equal(a, b)
    for want in [()] + subsets:
        for stats in (False, True):
            st = _state(c["n"])
            out = _run(c, want=want, state=st, stats=stats)
            for k in want:
                assert torch.equal(out[k], full[k]), (want, stats, k)
            assert not stats or torch.equal(out["stats"], full["stats"])
            for a, b in zip(st, full_state):
                assert torch.equal(a, b), (want, stats)


def test_two_runs_bitwise_equal():
    c = _case("two_hidden")
    a, b = _run(c), _run(c)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    big = dict(CASES["fn_131_rows"], n=5000, rpd=2)  # more items than workgroups: the stride loop
    CASES["_big"] = big
    try:
        c = _case("_big")
    finally:
        del CASES["_big"]
    a, b = _run(c), _run(c)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    ref = R.scores(R.mean_logits(c["layers"], c["S"], c["params"], c["eps"], c["x"], c["rpd"]),
                   c["z"])
    assert rel(a["mean_logits"].cpu().numpy(), ref["mean_logits"]) < 1e-4
    safe = R.top2_gap(ref["mean_logits"]) >= 1e-3
    assert np.array_equal(a["correct"].cpu().numpy()[safe], ref["correct"][safe])
    assert abs(a["stats"][1].item() - ref["stats"][1]) <= 1e-4 * ref["stats"][1]


def test_forgetting_update_over_three_launches():
    c = _case("fn_131_rows")
    n = c["n"]
    state = (torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.ones(n, device=DEV))
    la, fg, nl = np.zeros(n), np.zeros(n), np.ones(n)
    rng = np.random.default_rng(7)
    for it in range(3):
        params = c["params"].copy()
        params[:40] += rng.normal(size=40) * 2.0 * it
        ref = R.scores(R.mean_logits(c["layers"], c["S"], params, c["eps"], c["x"], c["rpd"]),
                       c["z"])
        assert R.top2_gap(ref["mean_logits"]).min() >= 1e-3
        la, fg, nl = R.forgetting_update(la, fg, nl, ref["correct"])
        out = _run(c, want=("correct",), state=state, stats=False, params=params)
        assert np.array_equal(out["correct"].cpu().numpy(), ref["correct"])
        for got, want in zip(state, (la, fg, nl)):
            assert np.array_equal(got.cpu().numpy(), want)
    assert fg.sum() > 0 and 0 < nl.sum() < n


def test_refusals_on_the_device():
    from psvi.runtime import InnerLoopPlan, PsviError, predict_scores

    c = _case("fn_131_rows")
    x, z, eps, params = _t(c["x"]), _t(c["z"], torch.int32), _t(c["eps"]), _t(c["params"])
    plan = InnerLoopPlan("meanfield", c["layers"], c["S"], 3)
    with pytest.raises(PsviError, match="PSVI_EINVAL"):  # nothing asked for
        predict_scores(plan, x, z, eps, params, c["rpd"], want=())
    with pytest.raises(PsviError, match="PSVI_EINVAL"):  # labels needed, none given
        predict_scores(plan, x, None, eps, params, c["rpd"], want=("el2n",))
    zbad = z.clone()
    zbad[17] = 3
    with pytest.raises(PsviError, match="PSVI_EINVAL"):  # a label outside [0, C)
        predict_scores(plan, x, zbad, eps, params, c["rpd"], want=("correct",))
    out = predict_scores(plan, x, zbad, eps, params, c["rpd"], want=("entropy",))  # labels unread
    assert torch.isfinite(out["entropy"]).all()
    for fam, layers, kw in (("fullcov", [(7, 3)], {}),
                            ("meanfield", [(7, 9), (9, 1)], dict(likelihood="bernoulli")),
                            ("meanfield", [(7, 9), (9, 1)], dict(likelihood=("gaussian", 1.0)))):
        p = InnerLoopPlan(fam, layers, c["S"], 3, **kw)
        e = torch.zeros(-(-c["n"] // c["rpd"]) * p.eps_count, device=DEV)
        with pytest.raises(PsviError, match="PSVI_ESTATE"):
            predict_scores(p, x, None, e, torch.zeros(p.param_count, device=DEV), c["rpd"],
                           want=("entropy",))
    with pytest.raises(ValueError):  # eps one block short
        predict_scores(plan, x, z, eps[:-plan.eps_count].contiguous(), params, c["rpd"])
