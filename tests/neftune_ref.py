"""numpy float32 restatement of the NEFTune noise rule (csrc/philox.h, include/mmpt.h K8) and the
hook that feeds a given noise tensor to an oracle's input embedding.

The rule: logical element e = row*h + col of noise site `site` takes word e % 4 of
dropout_words(e / 4, site, seed) (the hidden-dropout addressing, test_dropout_cpu.philox4x32_10);
  k = word >> 9,  s = float32(2k + 1) * 2^-23 - 1,  noise = s * mag,  out = value + noise
with every operation a separately rounded float32 one (numpy float32 arrays never fuse), and
mag = float32(alpha / sqrt(S_in * hidden)) computed in double.
"""

import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

from test_dropout_cpu import U32, philox4x32_10

TWO_M23 = np.float32(2.0 ** -23)


def words(e, site: int, seed: int) -> np.ndarray:
    """uint32: the Philox word of every logical element in `e` (any shape, uint64 values)."""
    e = np.asarray(e, dtype=np.uint64)
    q = e >> np.uint64(2)
    w = philox4x32_10((q & U32, q >> np.uint64(32), site & 0xFFFFFFFF, (site >> 32) & 0xFFFFFFFF),
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    w = np.stack(np.broadcast_arrays(*w), axis=-1)
    return np.take_along_axis(w, (e & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]


def unit(word) -> np.ndarray:
    """float32 s in (-1, 1), an odd multiple of 2^-23: exact at every step."""
    k = np.asarray(word, dtype=np.uint32) >> np.uint32(9)
    odd = (k.astype(np.int64) * 2 + 1).astype(np.float32)  # < 2^24: exact
    return odd * TWO_M23 - np.float32(1.0)


def mag_of(alpha: float, seq_in: int, hidden: int) -> np.float32:
    return np.float32(float(alpha) / math.sqrt(float(seq_in) * float(hidden)))


def noise_at(e, site: int, seed: int, mag) -> np.ndarray:
    """float32 noise of the logical elements `e`: one rounded multiply."""
    return unit(words(e, site, seed)) * np.float32(mag)


def noise(rows: int, h: int, site: int, seed: int, mag, row0: int = 0) -> np.ndarray:
    """float32 [rows, h]: the noise of rows row0 .. row0 + rows - 1 of an h-wide site."""
    e = np.arange(row0 * h, (row0 + rows) * h, dtype=np.uint64).reshape(rows, h)
    return noise_at(e, site, seed, mag)


def add(value: np.ndarray, nz: np.ndarray) -> np.ndarray:
    """out = value + noise: one rounded float32 add."""
    return np.asarray(value, dtype=np.float32) + np.asarray(nz, dtype=np.float32)


@contextlib.contextmanager
def embedding_hook(table: torch.Tensor, nz):
    """The forward hook HF's Trainer registers on the input embedding, for the functional
    oracles: while active, F.embedding over `table` (that very tensor object — the word table the
    oracle reads) returns its output + nz (a float32 tensor or array of the output's shape, the
    leading dimensions flattened or not).  Other tables (positions) pass through.  Yields a
    one-element list counting the hooked calls."""
    nz = torch.as_tensor(np.asarray(nz)) if not torch.is_tensor(nz) else nz
    orig = F.embedding
    calls = [0]

    def hooked(input, weight, *a, **kw):
        out = orig(input, weight, *a, **kw)
        if weight is table:
            calls[0] += 1
            out = out + nz.reshape(out.shape).to(out.dtype)
        return out

    F.embedding = hooked
    try:
        yield calls
    finally:
        F.embedding = orig
