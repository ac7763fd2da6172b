"""Host side of stochastic depth (ConvNextDropPath): who is kept, known before anything is launched.

The keep bits are the hidden-dropout bits (include/mmpt.h K16, csrc/philox.h): sample b of a
block is element b of a dropout site and is kept iff word b % 4 of
philox4x32_10(counter = (b / 4, site), key = seed) >= floor(p * 2^32).  The rule is a pure
function of (p, seed, site), so the host restates it in numpy and never asks the device;
mmpt_dropout_mask(n = B, p, seed, site) gives the same bits.
"""

from __future__ import annotations

import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _philox4x32_10(c, k):
    """Philox4x32-10 on uint64 arrays holding 32-bit words: four counter words, two key words."""
    c = [np.asarray(x, dtype=np.uint64) & _U32 for x in c]
    k = [np.uint64(x) & _U32 for x in k]
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _U32, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _U32]
        k = [(k[0] + np.uint64(_W0)) & _U32, (k[1] + np.uint64(_W1)) & _U32]
    return c


def keep_masks(n: int, ps, seed: int, sites) -> np.ndarray:
    """bool [len(ps), n]: row i holds the keep bits of elements 0 .. n-1 of dropout site sites[i]
    under `seed` at drop probability ps[i] (0 <= p < 1; a threshold of 0 keeps everything).  One
    vectorised Philox evaluation for all sites: a micro-step's blocks cost one call."""
    for p in ps:
        if not 0.0 <= p < 1.0:
            raise ValueError(f"keep_masks: p must lie in [0, 1), got {p!r}")
    t = np.array([int(float(p) * 4294967296.0) for p in ps], dtype=np.uint64)[:, None]
    q = np.arange((n + 3) // 4, dtype=np.uint64)[None, :]
    lo = np.array([s & 0xFFFFFFFF for s in sites], dtype=np.uint64)[:, None]
    hi = np.array([(s >> 32) & 0xFFFFFFFF for s in sites], dtype=np.uint64)[:, None]
    zero = np.zeros((len(ps), q.shape[1]), dtype=np.uint64)
    w = _philox4x32_10((q & _U32 | zero, q >> _S32 | zero, lo | zero, hi | zero),
                       (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    words = np.stack(w, axis=2).reshape(len(ps), -1)[:, :n]
    return (words >= t) | (t == 0)


def keep_mask(n: int, p: float, seed: int, site: int) -> np.ndarray:
    """bool [n]: the keep bits of one site (mmpt_dropout_mask(n, p, seed, site) on the host)."""
    return keep_masks(n, (p,), seed, (site,))[0]


def kept_indices(B: int, p: float, seed: int, site: int) -> tuple:
    """The kept samples of a block, increasing: the planes its compact tensors hold."""
    return tuple(int(i) for i in np.flatnonzero(keep_mask(B, p, seed, site)))


def kept_indices_of(B: int, ps, seed: int, sites) -> list:
    """kept_indices for several blocks (one probability and one site each) in one evaluation."""
    return [tuple(int(i) for i in np.flatnonzero(m)) for m in keep_masks(B, ps, seed, sites)]
