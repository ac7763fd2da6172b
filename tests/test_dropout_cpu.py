"""CPU-only tests of the hidden-dropout host side.

* csrc/philox.h, compiled into a small stand-alone g++ program, against the Random123 known
  answers of Philox4x32-10, and the header's dropout addressing (counter / key / threshold /
  scale) against the numpy restatement below — which tests/test_dropout_gpu.py reuses as the
  reference of the kernels' masks.
* engine.dropout_site: injective over steps, ranks, units and sites; raises out of range.
* config: the fields, with_dropout, the tiny-mm-drop preset, ValueError on Llama / CLIP.
* include/mmpt.h and _lib.py agree on ABI 16 and on the four dropout signatures.
"""

import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHILOX_H = os.path.join(ROOT, "multimodal_llm_pretraining_amd", "csrc", "philox.h")

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)

# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, expected)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


# ------------------------------------------------------------------ numpy restatement
def philox4x32_10(c, k):
    """c: four uint32 arrays (or ints) of one shape, k: two; returns the four output words as
    uint32 arrays.  Arithmetic in uint64 with explicit 32-bit masks."""
    c = [np.asarray(x, dtype=np.uint64) & U32 for x in c]
    k = [np.asarray(x, dtype=np.uint64) & U32 for x in k]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1],
             p0 & U32]
        k = [(k[0] + np.uint64(W0)) & U32, (k[1] + np.uint64(W1)) & U32]
    return [x.astype(np.uint32) for x in c]


def threshold(p: float) -> int:
    return int(np.floor(np.float64(p) * 4294967296.0))


def scale(p: float) -> np.float32:
    return np.float32(1.0 / (1.0 - np.float64(p)))


def keep_mask(n: int, p: float, seed: int, site: int) -> np.ndarray:
    """bool [n]: element e is kept iff word e % 4 of philox(counter = (e/4, site), key = seed)
    >= floor(p * 2^32)."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((q & U32, q >> np.uint64(32), site & 0xFFFFFFFF, (site >> 32) & 0xFFFFFFFF),
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    words = np.stack(np.broadcast_arrays(*w), axis=1).reshape(-1)[:n]
    return words >= np.uint32(threshold(p)) if threshold(p) else np.ones(n, dtype=bool)


# ------------------------------------------------------------------ the header itself
PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include "philox.h"
// argv: "kat" c0 c1 c2 c3 k0 k1 (hex) -> the four words; "words" q site seed (hex) -> the four
// words of dropout_words; "rule" p -> threshold (hex) and the scale's bits (hex)
int main(int argc, char** argv) {
  if (argc == 8) {
    uint32_t v[6];
    for (int i = 0; i < 6; ++i) v[i] = (uint32_t)strtoul(argv[2 + i], nullptr, 16);
    const mmpt::philox4 r = mmpt::philox4x32_10(v[0], v[1], v[2], v[3], v[4], v[5]);
    printf("%08x %08x %08x %08x\n", r.w[0], r.w[1], r.w[2], r.w[3]);
  } else if (argc == 5) {
    const mmpt::philox4 r = mmpt::dropout_words(strtoull(argv[2], nullptr, 16),
                                                strtoull(argv[3], nullptr, 16),
                                                strtoull(argv[4], nullptr, 16));
    printf("%08x %08x %08x %08x\n", r.w[0], r.w[1], r.w[2], r.w[3]);
  } else {
    const double p = strtod(argv[2], nullptr);
    const float s = mmpt::dropout_scale(p);
    uint32_t bits;
    __builtin_memcpy(&bits, &s, 4);
    printf("%08x %08x\n", mmpt::dropout_threshold(p), bits);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def philox_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("philox")
    src, exe = str(d / "philox_check.cpp"), str(d / "philox_check")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.dirname(PHILOX_H), src, "-o", exe],
                   check=True)

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return [int(x, 16) for x in r.stdout.split()]

    return run


def test_known_answers_header(philox_exe):
    for c, k, want in KAT:
        got = philox_exe("kat", *(f"{x:x}" for x in c + k))
        assert tuple(got) == want, (c, k, [f"{x:08x}" for x in got])


def test_known_answers_numpy():
    for c, k, want in KAT:
        assert tuple(int(x) for x in philox4x32_10(c, k)) == want
    # vectorised: the three vectors at once
    c = [np.array([v[0][i] for v in KAT]) for i in range(4)]
    k = [np.array([v[1][i] for v in KAT]) for i in range(2)]
    got = np.stack(philox4x32_10(c, k), axis=1)
    assert (got == np.array([v[2] for v in KAT], dtype=np.uint32)).all()


def test_header_addressing_matches_numpy(philox_exe):
    """dropout_words(q, site, seed): counter = (lo q, hi q, lo site, hi site), key = (lo seed,
    hi seed); threshold floor(p 2^32) and scale float(1 / (1 - p))."""
    for q, site, seed in [(0, 0, 0), (5, 7, 1234), (1 << 33 | 3, 0xABCDEF0123456789, 1 << 63 | 17),
                          (0xFFFFFFFF, 1 << 32, 0xFFFFFFFF00000000)]:
        want = philox4x32_10((q & 0xFFFFFFFF, q >> 32, site & 0xFFFFFFFF, site >> 32),
                             (seed & 0xFFFFFFFF, seed >> 32))
        got = philox_exe("words", f"{q:x}", f"{site:x}", f"{seed:x}")
        assert got == [int(x) for x in want], (q, site, seed)
        # keep_mask reads the same words
        thr = threshold(0.5)
        if q < 1 << 20:
            km = keep_mask(4 * q + 4, 0.5, seed, site)[4 * q:]
            assert list(km) == [w >= thr for w in got]
    for p in (0.0, 0.1, 0.5, 0.25, 0.999999):
        thr, bits = philox_exe("rule", repr(p))
        assert thr == threshold(p)
        assert bits == int(np.array(scale(p)).view(np.uint32))
    assert threshold(0.0) == 0 and threshold(0.5) == 1 << 31
    assert threshold(0.1) == 429496729  # floor(0.1 * 2^32) with 0.1 the nearest double


def test_mask_statistics_numpy():
    """The figure the GPU statistics test quotes: n = 2^20, seed 1234, site 7, p = 0.1."""
    n, p = 1 << 20, 0.1
    dropped = 1.0 - keep_mask(n, p, 1234, 7).mean()
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(dropped - p) < 5 * sigma, (dropped, sigma)
    assert abs(dropped - 0.100126) < 1e-6, dropped


# ------------------------------------------------------------------ dropout_site
def test_dropout_site_injective_and_ranged():
    from multimodal_llm_pretraining_amd.engine import (SITE_KS, SITE_RANKS, SITE_STEPS,
                                                       SITE_UNITS, VISION_UNIT, dropout_site)

    steps = [0, 1, 2, 1000, SITE_STEPS - 1]
    ranks = [0, 1, 7, 255, SITE_RANKS - 1]
    units = [0, 1, 2, 40, VISION_UNIT - 1, VISION_UNIT, VISION_UNIT + 1, SITE_UNITS - 1]
    ks = [0, 1, 2, SITE_KS - 1]
    seen = {}
    for key in itertools.product(steps, ranks, units, ks):
        s = dropout_site(*key)
        assert 0 <= s < 1 << 64
        assert seen.setdefault(s, key) == key, (key, seen[s])
    assert len(seen) == len(steps) * len(ranks) * len(units) * len(ks)
    # the fields: the step is the high word (two steps differ only there)
    assert dropout_site(3, 0, 0, 0) == 3 << 32
    assert dropout_site(5, 2, 9, 1) ^ dropout_site(6, 2, 9, 1) == (5 ^ 6) << 32
    for bad in [(-1, 0, 0, 0), (SITE_STEPS, 0, 0, 0), (0, -1, 0, 0), (0, SITE_RANKS, 0, 0),
                (0, 0, -1, 0), (0, 0, SITE_UNITS, 0), (0, 0, 0, -1), (0, 0, 0, SITE_KS)]:
        with pytest.raises(ValueError, match="dropout_site"):
            dropout_site(*bad)


# ------------------------------------------------------------------ configuration
def test_config_fields_and_helper():
    from multimodal_llm_pretraining_amd import config as C

    for name in ("tiny-mm", "tiny-lm", "vit-b16-pythia-1b", "pythia-1b", "llava-pretrain"):
        cfg = C.get_config(name)
        assert cfg.text.hidden_dropout == 0.0
        assert cfg.vision is None or cfg.vision.hidden_dropout == 0.0
    base = C.get_config("tiny-mm")
    d = C.with_dropout(base, text=0.1, vision=0.2)
    assert (d.text.hidden_dropout, d.vision.hidden_dropout) == (0.1, 0.2)
    assert C.with_dropout(d) == base  # the defaults switch it off again
    assert C.param_shapes(d) == C.param_shapes(base)
    assert C.get_config("tiny-mm-drop") == C.with_dropout(base, text=0.1, vision=0.1)
    assert C.with_dropout(C.get_config("tiny-lm"), text=0.1).text.hidden_dropout == 0.1
    assert not hasattr(d.text, "attention_dropout")  # attention-probability dropout: out of scope


@pytest.mark.parametrize("name,kw", [("tiny-llama", {"text": 0.1}), ("tiny-llava", {"text": 0.1}),
                                     ("tiny-llava", {"vision": 0.1}),
                                     ("tiny-clip-d80", {"vision": 0.1}),
                                     ("llava-pretrain", {"text": 0.1, "vision": 0.1}),
                                     ("tiny-lm", {"vision": 0.1}), ("tiny-lm", {"text": 1.0}),
                                     ("tiny-lm", {"text": -0.1})])
def test_with_dropout_raises(name, kw):
    from multimodal_llm_pretraining_amd import config as C

    with pytest.raises(ValueError, match="hidden_dropout"):
        C.with_dropout(C.get_config(name), **kw)


def test_config_constructor_raises():
    from multimodal_llm_pretraining_amd import config as C

    with pytest.raises(ValueError, match="Llama"):
        C.TextConfig(arch="llama", hidden_dropout=0.1)
    with pytest.raises(ValueError, match="CLIP"):
        C.VisionConfig(pre_ln=True, hidden_dropout=0.1)
    C.with_dropout(C.get_config("tiny-clip-d80"), text=0.1)  # GPTNeoX beside a CLIP tower: fine


# ------------------------------------------------------------------ header / binding
C_TYPES = {"int64_t": "I64", "double": "F64", "uint64_t": "U64", "void*": "P", "constvoid*": "P",
           "constfloat*": "P", "float*": "P", "uint8_t*": "P"}
WANT = {
    "mmpt_dropout_bf16": "rows h src ld_src dst ld_dst p seed site stream",
    "mmpt_dropout_f32": "rows h src dst p seed site stream",
    "mmpt_dropout_add_f32": "rows h y ld_y site_y y2 ld_y2 site_y2 resid out p seed stream",
    "mmpt_dropout_mask": "n p seed site keep stream",
}


def test_header_and_binding_agree_on_dropout():
    from multimodal_llm_pretraining_amd import _lib

    src = open(os.path.join(ROOT, "include", "mmpt.h")).read()
    assert re.search(r"#define MMPT_ABI_VERSION (\d+)", src).group(1) == "16"
    assert _lib.ABI_VERSION == 16
    for name, params in WANT.items():
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
        names = [re.split(r"[ *]", a)[-1] for a in args]
        assert names == params.split(), (name, names)
        types = [C_TYPES["".join(a.rsplit(n, 1)[0].split())] for a, n in zip(args, names)]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is _lib.I32
        assert argtypes == [getattr(_lib, t) for t in types], (name, types)
