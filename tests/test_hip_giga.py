"""GIGA on the GPU: psvi_giga_step against the reference-generated fixtures k1
and, at the shape edges, against the fp64 restatement (giga_util, itself pinned
to the fixtures on the CPU); run_giga against the reference's whole runs k2,
replayed through the hooks.

Tolerances: ll within 1e-4 relative + 1e-6; score, gamma, lw and w within 4x
the reference's own fp32-against-fp64 gap recorded in the fixture; the picked
indices, csizes and accs exactly (the fixtures' margins make that a fair
demand).  The kernel's sums are fp64 with float outputs, so against the
restatement applied to the GPU's own ll it agrees to float rounding (1e-6
relative)."""
import ctypes

import numpy as np
import pytest
import torch

from golden_util import load_fixture, rel
import giga_util as G
import laplace_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _step(samples, rows, labels, lw):
    from psvi.runtime import giga_step

    out = giga_step(dev(samples), dev(rows), dev(labels), dev(lw), want_ll=True)
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("name", ["k1_step_first", "k1_step_mid"])
def test_step_matches_reference(name):
    f = load_fixture(name)
    c = f["cfg"]
    assert c["top2"] > 100 * 4 * c["tol_score"] and c["den"] > 100 * 4 * c["tol_score"]
    out = _step(f["samples"], f["rows"], f["labels"], f["lw_in"])
    res = out["result"].tolist()
    err = np.abs(out["ll"].numpy() - f["ll64"])
    es = np.abs(out["score"].numpy() - f["score64"]).max()
    el = np.abs(out["lw"].numpy() - f["lw64"]).max()
    print(name, "ll max err", err.max(), "score err", es, "4 x gap", 4 * c["tol_score"],
          "gamma err", abs(res[5] - float(f["gamma64"])), "4 x gap", 4 * c["tol_gamma"],
          "lw err", el, "4 x gap", 4 * c["tol_lw"], "scale err", abs(res[6] - float(f["scale64"])))
    assert (err <= 1e-4 * np.abs(f["ll64"]) + 1e-6).all()
    assert es <= 4 * c["tol_score"]
    assert abs(res[5] - float(f["gamma64"])) <= 4 * c["tol_gamma"]
    assert el <= 4 * c["tol_lw"]
    assert int(res[1]) == c["argmax"] and int(f["sub"][int(res[1])]) == int(f["pt_idx64"])
    assert abs(res[0] - f["score64"].max()) <= 4 * c["tol_score"]


# ---- shape edges: twice, bit for bit, and against the restatement
def _problem(S, n, d, seed, lw="unit"):
    g = torch.Generator().manual_seed(seed)
    rows = torch.cat((torch.randn(n, d - 1, generator=g), torch.ones(n, 1)), dim=1)
    labels = (torch.rand(n, generator=g) > 0.5).float()
    samples = (torch.randn(d, generator=g) + 0.5 * torch.randn(S, d, generator=g)) / d ** 0.5
    v = torch.randn(S, generator=g)
    return samples, rows, labels, (v / v.norm() if lw == "unit" else torch.zeros(S))


def _check(out, samples, rows, labels, lw):
    ll64 = U.ll_matrix(samples.double(), rows.double(), labels.double())
    assert ((out["ll"].double() - ll64).abs() <= 1e-6 * ll64.abs() + 1e-7).all()
    res = out["result"].tolist()
    n = int(res[1])
    assert res[1] == n and 0 <= n < rows.shape[0]
    r = G.step(out["ll"].double(), lw.double(), pick=n)
    assert rel(out["score"], r["score"]) < 1e-6
    # the pick is the maximum up to rounding (at S = 2 every |score| is 1) and
    # holds the largest of the kernel's own scores
    assert r["score"][n] >= r["score"].max() - 1e-6
    assert out["score"][n] == out["score"].max()
    assert res[0] == pytest.approx(float(r["score"][n]), rel=1e-6, abs=1e-9)
    for i, k in ((2, "zeta0"), (3, "zeta1"), (4, "zeta2"), (5, "gamma"), (6, "scale"), (7, "L")):
        assert res[i] == pytest.approx(float(r[k]), rel=1e-6, abs=1e-9), k
    assert rel(out["lw"], r["lw"]) < 1e-6
    assert float(out["lw"].double().norm()) == pytest.approx(1.0, abs=1e-6)


def _twice(prob, check=True):
    a, b = _step(*prob), _step(*prob)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert all(torch.isfinite(v).all() for v in a.values())
    if check:
        _check(a, *prob)
    return a


# S: 65 crosses a wave, 2048 is the range edge; n_data: 513 crosses the
# workgroup's 512 column owners, 2048 is the range edge; d: both range edges
EDGES = [(2, 1, 2), (2, 2048, 2), (3, 1, 2), (3, 2, 256), (50, 513, 3), (65, 513, 2),
         (65, 32, 256), (2048, 2, 3), (2048, 1, 2), (50, 2048, 2)]


@pytest.mark.parametrize("lw", ["zero", "unit"])
@pytest.mark.parametrize("S,n,d", EDGES)
def test_edge_shapes_and_bitwise_repeat(S, n, d, lw):
    _twice(_problem(S, n, d, 1000 * S + 10 * n + d, lw))


@pytest.mark.parametrize("lw", ["zero", "unit"])
def test_duplicated_rows_return_the_first_index(lw):
    """Every row twice, the copy 600 places on (another owner, another stride):
    the winner ties with its copy bit for bit and the first index is returned."""
    samples, rows, labels, v = _problem(50, 600, 3, 11, lw)
    out = _twice((samples, torch.cat((rows, rows)), torch.cat((labels, labels)), v))
    n = int(out["result"][1])
    assert n < 600
    assert torch.equal(out["score"][:600], out["score"][600:])
    assert out["score"][n] == out["score"].max()
    assert n == int((out["score"] == out["score"].max()).nonzero()[0, 0])


def test_zero_centred_row_takes_the_clamp():
    """A row of zeros (ones column included) has the same ll under every sample:
    cll is identically zero, its direction is 0 / 1e-12 = 0 and so is its score."""
    samples, rows, labels, v = _problem(50, 40, 3, 12)
    rows[7] = 0.0
    out = _twice((samples, rows, labels, v))
    assert torch.equal(out["ll"][:, 7], out["ll"][0, 7].expand(50))
    assert out["score"][7] == 0.0 and int(out["result"][1]) != 7


def test_out_of_range_arguments_return_einval():
    from psvi.runtime import PsviError, _lib, giga_step
    from psvi.runtime.engine import _ptr, _stream

    def step(S=3, n=2, d=3):
        samples, rows, labels, lw = _problem(S, max(n, 1), d, 3)
        return giga_step(dev(samples), dev(rows[:n]), dev(labels[:n]), dev(lw))

    step()
    for kw in (dict(S=1), dict(S=2049), dict(d=1), dict(d=257), dict(n=0), dict(n=2049)):
        with pytest.raises(PsviError, match="PSVI_EINVAL"):
            step(**kw)
            pytest.fail(f"{kw} was accepted")
    # lw_out must not alias lw_in
    samples, rows, labels, lw = (dev(t) for t in _problem(3, 2, 3, 3))
    score, result = torch.empty(2, device=DEV), torch.empty(8, dtype=torch.float64, device=DEV)
    req = _lib.GigaStepReq(3, 3, 2, _ptr(samples), _ptr(rows), _ptr(labels), _ptr(lw), _ptr(score),
                           _ptr(lw), None, _ptr(result))
    assert _lib.load().psvi_giga_step(ctypes.byref(req), _stream()) == -1


# ---- whole runs of the reference, replayed through the hooks
def _replay(name):
    import psvi.inference as I

    f = load_fixture(name)
    c = f["cfg"]
    flat, o = torch.tensor(f["draws"]), [0]

    def take(n):
        out = flat[o[0]:o[0] + n]
        assert out.numel() == n, "draw stream exhausted"
        o[0] += n
        return out

    batches, state = iter([f["subset"]] + list(f["batches"])), {}
    res = I.run_giga(x=torch.tensor(f["x"]), y=torch.tensor(f["y"]), xt=torch.tensor(f["xt"]),
                     yt=torch.tensor(f["yt"]), mc_samples=c["S"], data_minibatch=c["B"],
                     num_epochs=c["epochs"], log_every=c["log_every"], N=c["N"], D=c["D"],
                     seed=c["seed"], subset_size=c["subset_size"], lr0net=c["lr0net"],
                     noise_source=take, batch_source=lambda: next(batches), state_out=state)
    assert o[0] == flat.numel() and next(batches, None) is None
    return f, c, res, state


@pytest.mark.parametrize("name", ["k2_run_log1", "k2_run_log2"])
def test_whole_run_replays_reference(name):
    f, c, res, state = _replay(name)
    assert c["top2"] > 100 * 4 * c["tol_score"] and c["den"] > 100 * 4 * c["tol_score"]
    assert (np.abs(f["probs64"] - 0.5) > 100 * 4 * np.abs(f["probs32"] - f["probs64"])).all()
    ew, el = np.abs(state["w"] - f["w"][-1]).max(), np.abs(state["lw"] - f["lw"][-1]).max()
    print(name, "pts", state["pt_idcs"], "max|dw|", ew, "4 x gap", 4 * c["tol_w"], "max|dlw|", el,
          "4 x gap", 4 * c["tol_lw"], "nlls", res["nlls"], f["nlls"])
    assert state["pt_idcs"] == f["pt_idx"].tolist()
    assert state["core_idcs"] == f["core_idcs"].tolist()
    assert res["csizes"] == f["csizes"].tolist()
    nt = len(f["yt"])
    assert np.array_equal(np.round(np.array(res["accs"]) * nt), np.round(f["accs"] * nt))
    assert np.allclose(res["nlls"], f["nlls"], rtol=1e-4, atol=0)
    assert ew <= 4 * c["tol_w"] and el <= 4 * c["tol_lw"]
    assert set(res) == {"accs", "nlls", "csizes", "times"}
    assert len(res["times"]) == len(res["accs"]) == len(f["pt_idx"])


def test_coreset_grows_on_logging_iterations_only():
    """log_every = 2 over the same six epochs: half the steps, half the points."""
    a, b = load_fixture("k2_run_log1"), _replay("k2_run_log2")[3]
    assert len(b["pt_idcs"]) == 3 and 2 * len(b["core_idcs"]) == len(a["core_idcs"])
