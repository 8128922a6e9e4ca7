"""psvi_randn against an independent statement of its stream.

Every draw of the library in throughput mode -- psvi_randn, the network
launch's fused draw, the loops' draws and their bf16 planes -- goes through one
device function, and the other tests hold those paths to each other, bitwise.
Here the stand-alone kernel is held to tests/philox_util.py: Philox4x32-10
(pinned to the published known-answer vectors by test_philox_cpu.py) and
Box-Muller in float64, as include/psvi_hip.h documents the stream.

  * values: every seed / offset pair that reaches another word of the key or
    of the counter (the seed's high half, the carry of the counter's low word
    into the high one, bit 63 of the offset), elementwise within TOL;
  * the edges of u1 = ((w >> 8) + 1) / 2^24: the largest radius (the only
    place a half-step error of the mapping, or a missing + 1, shows) and
    radius 0;
  * the stream's identities (an offset moves along one stream, a shorter draw
    is a prefix), bitwise;
  * tails and alignment: sentinels around the draw survive, the 4-byte-aligned
    path writes the same bits as the vector-store path, n = 0 writes nothing;
  * the grid-stride loop: more quads than the launch has threads.

TOL, absolute: the same formula in fp32 with a correctly rounded libm is
within 1.1e-6 of the float64 reference; the kernel takes log2, sqrt, sin and
cos from the native instructions, whose extra error is allowed for by about
20x that figure.  A swapped sine / cosine or u1 / u2 moves nearly every element
by more than 1e-4 (median 0.9), so the bound separates the two cleanly.  Each
test prints the largest deviation it saw (pytest -s); DESIGN.md records it."""
import ctypes

import numpy as np
import pytest
import torch

from philox_util import normals

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-5
SEEDS = [0, 1234, 2**32 + 1234, 2**64 - 1]
OFFSETS = [0, 4, 2**34 - 8, 2**63]
N = 4099
EDGE_SEED = 0x5EED  # test_philox_cpu.py::test_edge_words asserts the words of these quads
EDGE_MAX = [(2569854, 0), (8233467, 1)]  # (counter, pair): w[2 pair] >> 8 == 0, u1 = 2^-24
EDGE_ZERO = 489735  # w[0] >> 8 == 0xffffff: u1 = 1
RMAX = float(np.sqrt(48.0 * np.log(2.0)))  # sqrt(-2 ln 2^-24) = 5.76810...
SENT = 0x7FC00000  # a NaN's bits: no draw produces them
PAD = 8


def _draw(n, seed, offset=0):
    from psvi.runtime import randn_

    return randn_(torch.empty(n, device=DEV), seed, offset)


def _dev(got, seed, offset, what):
    """max |got - reference| over a draw of (seed, offset), printed."""
    ref = normals(seed, offset, got.numel())
    x = got.cpu().double().numpy()
    assert np.isfinite(x).all(), what
    d = float(np.abs(x - ref).max())
    print(f"randn {what}: max |kernel - float64 reference| = {d:.3e}")
    return d


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("seed", SEEDS)
def test_values_match_reference(seed, offset):
    got = _draw(N, seed, offset)
    assert _dev(got, seed, offset, f"seed {seed:#x} offset {offset:#x}") < TOL


def test_key_and_counter_high_words_are_used():
    """The seed's high half and the counter's high word change the stream."""
    base = _draw(N, 1234, 0)
    for seed, offset in ((2**32 + 1234, 0), (1234, 2**34)):
        other = _draw(N, seed, offset)
        assert (other != base).float().mean().item() > 0.99, (seed, offset)


@pytest.mark.parametrize("ctr,pair", EDGE_MAX)
def test_largest_radius(ctr, pair):
    """u1 = 2^-24: finite, the reference's values, radius sqrt(48 ln 2)."""
    offset = 4 * ctr - 8
    got = _draw(16, EDGE_SEED, offset)
    assert torch.isfinite(got).all()
    assert _dev(got, EDGE_SEED, offset, f"largest radius, counter {ctr}") < TOL
    a, b = (float(v) for v in got[8 + 2 * pair:10 + 2 * pair].cpu().double())
    ref = normals(EDGE_SEED, offset, 16)[8 + 2 * pair:10 + 2 * pair]
    assert abs(a - ref[0]) < TOL and abs(b - ref[1]) < TOL
    rad = float(np.hypot(a, b))
    print(f"randn largest radius, counter {ctr}: {rad:.7f} (exact {RMAX:.7f})")
    assert abs(rad - 5.76815) < 1e-4
    assert abs(rad - RMAX) < 2 * TOL  # each of a, b within TOL of the reference's


def test_zero_radius():
    """u1 = 1: rad = 0, both outputs of the pair are zeros."""
    offset = 4 * EDGE_ZERO - 8
    got = _draw(16, EDGE_SEED, offset)
    assert _dev(got, EDGE_SEED, offset, f"zero radius, counter {EDGE_ZERO}") < TOL
    assert got[8].abs().item() == 0.0 and got[9].abs().item() == 0.0


@pytest.mark.parametrize("offset", [8, 2**34 - 8])
def test_offset_moves_along_the_stream(offset):
    full = _draw(8192, 1234, offset)
    for k in (1, 1025):
        part = _draw(8192 - 4 * k, 1234, offset + 4 * k)
        assert torch.equal(part, full[4 * k:]), k


def test_shorter_draws_are_prefixes():
    full = _draw(8192, 1234, 4)
    for n in (1, 2, 3, 5, 4099):
        assert torch.equal(_draw(n, 1234, 4), full[:n]), n


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4099])
def test_tails_and_alignment(n):
    """A draw into the middle of a sentinel-filled buffer, 16-byte aligned
    (float4 stores and a scalar tail) and one float further (4-byte aligned:
    scalar stores throughout): the same bits, nothing written outside."""
    from psvi.runtime import randn_

    ref = _draw(n, 77, 12).view(torch.int32)
    assert _dev(ref.view(torch.float32), 77, 12, f"n = {n}") < TOL
    for shift in (0, 1):
        buf = torch.full((n + 2 * PAD + 1,), SENT, dtype=torch.int32, device=DEV)
        out = buf[PAD + shift:PAD + shift + n].view(torch.float32)
        assert out.data_ptr() % 16 == 4 * shift
        randn_(out, 77, 12)
        assert torch.equal(buf[PAD + shift:PAD + shift + n], ref), shift
        assert (buf[:PAD + shift] == SENT).all() and (buf[PAD + shift + n:] == SENT).all(), shift


def test_empty_draw_writes_nothing():
    from psvi.runtime import _lib

    lib = _lib.load()
    buf = torch.full((2 * PAD,), SENT, dtype=torch.int32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.psvi_randn(ctypes.c_void_p(buf[PAD:].data_ptr()), 0, 1234, 0, stream) == 0
    torch.cuda.synchronize()
    assert (buf == SENT).all()


def test_grid_stride_loop():
    """The launch caps at 4096 blocks of 256 threads, one quad per thread and
    pass: 4 * 4096 * 256 + 23 values take a second pass and end in a cut quad."""
    n = 4 * 4096 * 256 + 23
    seed, offset = 2**32 + 1234, 2**34 - 8
    buf = torch.full((n + PAD,), SENT, dtype=torch.int32, device=DEV)
    from psvi.runtime import randn_

    got = randn_(buf[:n].view(torch.float32), seed, offset)
    assert _dev(got, seed, offset, f"n = {n}") < TOL
    assert (buf[n:] == SENT).all()


def test_rejects_bad_arguments():
    """offset % 4 != 0 and n < 0: PSVI_EINVAL, nothing written."""
    from psvi.runtime import PsviError, _lib, randn_

    lib = _lib.load()
    buf = torch.full((16,), SENT, dtype=torch.int32, device=DEV)
    for offset in (1, 2, 3, 2**63 + 2):
        with pytest.raises(PsviError, match="PSVI_EINVAL.*multiple of 4"):
            randn_(buf.view(torch.float32), 1, offset)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.psvi_randn(ctypes.c_void_p(buf.data_ptr()), -1, 1, 0, stream) == -1  # PSVI_EINVAL
    assert lib.psvi_randn(None, 4, 1, 0, stream) == -1
    torch.cuda.synchronize()
    assert (buf == SENT).all()
