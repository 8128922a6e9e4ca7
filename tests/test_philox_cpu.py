"""Pins tests/philox_util.py, the numpy restatement of psvi_randn's stream that
test_hip_randn.py holds the kernel to: the published Random123 known-answer
vectors of philox4x32 with 10 rounds, the counter / key mapping, the three
quads of seed 0x5EED whose words sit on the edges of the u1 mapping (the GPU
test's premise), and the moments of the normals.  No GPU."""
import numpy as np
import pytest

from philox_util import normals, philox4x32_10, words

# counter, key -> output (Random123's kat_vectors, philox4x32 10)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]
EDGE_SEED = 0x5EED
# (counter, pair) of the largest radius (w[2 pair] >> 8 == 0), and the counter
# whose first pair has radius 0 (w[0] >> 8 == 0xffffff)
EDGE_MAX = [(2569854, 0), (8233467, 1)]
EDGE_ZERO = 489735


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_known_answer_vectors(ctr, key, out):
    got = philox4x32_10(*ctr, *key)
    assert tuple(int(g[0]) for g in got) == out


def test_known_answer_vectors_as_one_batch():
    """The same three vectors through the array path the streams use."""
    cols = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    keys = [np.array([k[1][i] for k in KAT], dtype=np.uint64) for i in range(2)]
    got = np.stack(philox4x32_10(*cols, *keys), axis=1)
    assert got.tolist() == [list(k[2]) for k in KAT]


def test_words_map_counter_and_key():
    """words(): counter = offset / 4 + q in words 0 and 1 (low, high), zeros in
    words 2 and 3, the seed's halves as the key -- across the carry of the
    counter's low word and past 2^63."""
    seed = (0x299F31D0 << 32) | 0xA4093822
    for offset, nq in ((0, 3), (4 * 0xFFFFFFFE, 4), (2**34 - 8, 16), (2**63, 2), (2**64 - 8, 3)):
        w = words(seed, offset, nq)
        assert w.shape == (nq, 4) and w.dtype == np.uint64
        for q in range(nq):
            c = (offset // 4 + q) % 2**64
            ref = philox4x32_10(c & 0xFFFFFFFF, c >> 32, 0, 0, 0xA4093822, 0x299F31D0)
            assert w[q].tolist() == [int(r[0]) for r in ref], (offset, q)
    # the first vector: seed 0, offset 0
    assert words(0, 0, 1)[0].tolist() == list(KAT[0][2])
    # each half of the seed and of the counter reaches the generator
    base = words(1234, 0, 4)
    assert not (words(2**32 + 1234, 0, 4) == base).any()
    assert not (words(1234, 2**34, 4) == base).any()
    assert (words(1234, 8, 2) == base[2:]).all()


def test_edge_words():
    """The quads test_hip_randn.py draws for the edges of u1."""
    w = words(EDGE_SEED, 4 * 2569854, 1)[0]
    assert (int(w[0]), int(w[1])) == (0x000000D3, 0x20B884D3)
    w = words(EDGE_SEED, 4 * 8233467, 1)[0]
    assert (int(w[2]), int(w[3])) == (0x0000008B, 0xCD2489E3)
    w = words(EDGE_SEED, 4 * EDGE_ZERO, 1)[0]
    assert int(w[0]) == 0xFFFFFF70
    # what they mean for the normals: the largest radius, sqrt(-2 ln 2^-24), and 0
    rmax = np.sqrt(48.0 * np.log(2.0))
    assert abs(rmax - 5.7681075) < 1e-7
    for ctr, pair in EDGE_MAX:
        x = normals(EDGE_SEED, 4 * ctr, 4)
        assert np.isfinite(x).all()
        assert abs(np.hypot(x[2 * pair], x[2 * pair + 1]) - rmax) < 1e-12
    x = normals(EDGE_SEED, 4 * EDGE_ZERO, 4)
    assert x[0] == 0.0 and x[1] == 0.0 and np.hypot(x[2], x[3]) > 0.0


def test_normals_shape_and_moments():
    x = normals(1234, 0, 1 << 16)
    assert x.dtype == np.float64 and x.shape == (1 << 16,) and np.isfinite(x).all()
    assert abs(x.mean()) < 0.02 and abs(x.std() - 1.0) < 0.02
    # n cuts the last quad; an offset moves along the same stream
    assert (normals(1234, 0, 5) == x[:5]).all()
    assert (normals(1234, 4100, 7) == x[4100:4107]).all()
    assert normals(1234, 0, 0).shape == (0,)
