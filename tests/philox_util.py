"""psvi_randn's stream restated in numpy (no torch, no GPU), from the
description in include/psvi_hip.h and csrc/psvi_internal.hpp -- not from the
kernel's arithmetic: Philox4x32-10 on uint64 arrays masked to 32 bits, and
Box-Muller in float64.

Normal i of the stream (seed, offset), offset a multiple of 4, is element
i % 4 of the quad of Philox counter offset / 4 + i / 4:

    counter words (ctr & 0xffffffff, ctr >> 32, 0, 0), key (seed & 0xffffffff, seed >> 32)
    pair j in {0, 1}:  u1 = ((w[2j] >> 8) + 1) / 2^24   in (0, 1]
                       u2 = (w[2j+1] >> 8) / 2^24       in [0, 1)
                       rad = sqrt(-2 ln u1)
                       out[2j], out[2j+1] = rad cos(2 pi u2), rad sin(2 pi u2)
"""
import numpy as np

M0 = 0xD2511F53  # multiplies c0
M1 = 0xCD9E8D57  # multiplies c2
W0 = 0x9E3779B9  # key bumps per round (Weyl sequence)
W1 = 0xBB67AE85
MASK32 = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64)) & np.uint64(MASK32)


def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox4x32 on 32-bit words held in uint64 arrays (broadcast against each
    other); returns the four output words as uint64 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(x) for x in (c0, c1, c2, c3, k0, k1)))
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0  # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(W0)) & m32
        k1 = (k1 + np.uint64(W1)) & m32
    return c0, c1, c2, c3


def words(seed, offset, nquads):
    """The Philox output words of quads [0, nquads) of the stream (seed,
    offset): a (nquads, 4) uint64 array."""
    seed, offset = int(seed) & MASK64, int(offset) & MASK64
    assert offset % 4 == 0
    # counter = offset / 4 + q in two 32-bit halves, the low half's carry added
    # to the high one (q < 2^32 here, so no sum leaves uint64)
    base = offset // 4
    low = np.uint64(base & MASK32) + np.arange(int(nquads), dtype=np.uint64)
    lo = low & np.uint64(MASK32)
    hi = (np.uint64(base >> 32) + (low >> np.uint64(32))) & np.uint64(MASK32)
    return np.stack(philox4x32_10(lo, hi, 0, 0, seed & MASK32, seed >> 32), axis=1).reshape(-1, 4)


def normals(seed, offset, n):
    """Normals [0, n) of the stream (seed, offset), float64."""
    w = words(seed, offset, (int(n) + 3) // 4)
    out = np.empty((w.shape[0], 4), dtype=np.float64)
    for j in range(2):
        u1 = ((w[:, 2 * j] >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
        u2 = (w[:, 2 * j + 1] >> np.uint64(8)).astype(np.float64) / 16777216.0
        rad = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * j] = rad * np.cos(2.0 * np.pi * u2)
        out[:, 2 * j + 1] = rad * np.sin(2.0 * np.pi * u2)
    return out.reshape(-1)[:int(n)]
