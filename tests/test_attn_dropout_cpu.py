"""CPU-only tests of attention-probability dropout (include/mmpt.h "K19").

* csrc/philox.h's attention helpers, compiled into a stand-alone g++ program, against the numpy
  restatement of the mask addressing (tests/attn_dropout_ref.keep_mask), and t8 / p_eff / scale.
* Statistics of the numpy mask: keep fraction within 5 sigma of 1 - p_eff, neighbour correlation
  along q and along k below 5 / sqrt(n).
* scripts/diag/attn_plan_check.cpp with the dropout invariants; the plan argument itself.
* config: TextConfig.attn_dropout / VisionConfig.attention_dropout, their validation, with_dropout's keywords, the presets.
* The rounding-model pin: the two torch models of tests/attn_dropout_ref.py against the masked
  fp64 reference in row scales; their worst ratio fixes FACTOR.
* include/mmpt.h and _lib.py agree on the new signatures, with MMPT_ABI_VERSION still 16.
"""

import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_dropout_ref as DR  # noqa: E402
import attn_rowwise as AR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodal_llm_pretraining_amd", "csrc")

SEED, SITE = 0x9E3779B97F4A7C15, (0x12345 << 32) | (3 << 16) | (7 << 4) | 2  # high words set

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include "philox.h"
// "mask" b h heads seq_q seq_k p seed site -> seq_q lines of seq_k keep bits
// "rule" p -> t8, p_eff (%.17g), the scale's bits (hex)
int main(int argc, char** argv) {
  if (argc == 10) {
    const uint32_t b = atoi(argv[2]), h = atoi(argv[3]), heads = atoi(argv[4]);
    const int sq = atoi(argv[5]), sk = atoi(argv[6]);
    const uint32_t t8 = mmpt::attn_dropout_t8(strtod(argv[7], nullptr));
    const uint64_t seed = strtoull(argv[8], nullptr, 16), site = strtoull(argv[9], nullptr, 16);
    for (int q = 0; q < sq; ++q) {
      for (int k = 0; k < sk; ++k)
        putchar(mmpt::attn_dropout_keep_at(q, k, b * heads + h, site, seed, t8) ? '1' : '0');
      putchar('\n');
    }
  } else {
    const double p = strtod(argv[2], nullptr);
    const float s = mmpt::attn_dropout_scale(p);
    uint32_t bits;
    __builtin_memcpy(&bits, &s, 4);
    printf("%u %.17g %08x\n", mmpt::attn_dropout_t8(p), mmpt::attn_dropout_p_eff(p), bits);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("attn_philox")
    src, out = str(d / "attn_mask_check.cpp"), str(d / "attn_mask_check")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out], check=True)

    def run(*args):
        r = subprocess.run([out, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    return run


# ------------------------------------------------------------------ the mask
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("sq,sk", [(1, 1), (5, 7), (66, 130)])
@pytest.mark.parametrize("b,h", [(0, 0), (2, 5)])
def test_header_mask_matches_numpy(exe, b, h, sq, sk, p):
    heads = 7
    lines = exe("mask", b, h, heads, sq, sk, repr(p), f"{SEED:x}", f"{SITE:x}").split()
    got = np.array([[c == "1" for c in ln] for ln in lines])
    want = DR.keep_mask(b + 1, heads, sq, sk, p, SEED, SITE)[b, h]
    assert got.shape == (sq, sk) and (got == want).all()
    # the batch index enters through b * heads + h alone
    assert (DR.keep_mask(1, heads, sq, sk, p, SEED, SITE, b0=b)[0, h] == want).all()


def test_rule(exe):
    for p, t8 in [(0.0, 0), (0.001, 0), (0.1, 25), (0.5, 128), (0.999, 255)]:
        got_t8, got_pe, bits = exe("rule", repr(p)).split()
        assert int(got_t8) == t8 == DR.t8_of(p)
        assert float(got_pe) == t8 / 256.0 == DR.p_eff(p)
        assert int(bits, 16) == int(np.array(DR.scale_of(p)).view(np.uint32))
        assert DR.scale_of(p) == np.float32(1.0 / (1.0 - t8 / 256.0))
    assert DR.scale_of(0.001) == 1.0  # t8 == 0: the p = 0 path


def test_mask_statistics():
    for p in (0.1, 0.5):
        m = DR.keep_mask(2, 4, 256, 256, p, SEED, SITE)
        n, pe = m.size, DR.p_eff(p)
        sigma = (pe * (1 - pe) / n) ** 0.5
        assert abs(m.mean() - (1 - pe)) < 5 * sigma, (p, m.mean(), sigma)
        x = m.astype(np.float64) - m.mean()
        var = (x * x).mean()
        cq = (x[:, :, 1:] * x[:, :, :-1]).mean() / var
        ck = (x[..., 1:] * x[..., :-1]).mean() / var
        assert abs(cq) < 5 / n ** 0.5 and abs(ck) < 5 / n ** 0.5, (p, cq, ck)
    # another seed, a site differing in the high word only, another batch index: other masks
    base = DR.keep_mask(1, 2, 64, 64, 0.5, SEED, SITE)
    for other in (DR.keep_mask(1, 2, 64, 64, 0.5, SEED ^ 1, SITE),
                  DR.keep_mask(1, 2, 64, 64, 0.5, SEED, SITE ^ (1 << 40)),
                  DR.keep_mask(1, 2, 64, 64, 0.5, SEED, SITE, b0=1)):
        assert 0.4 < (other != base).mean() < 0.6
    assert DR.keep_mask(1, 1, 9, 9, 0.001, SEED, SITE).all()


# ------------------------------------------------------------------ plan
def test_plan_invariants_with_dropout(tmp_path):
    src = os.path.join(ROOT, "scripts", "diag", "attn_plan_check.cpp")
    assert "dropout" in open(src).read()
    out = str(tmp_path / "attn_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]


PLAN_PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "attn_plan.h"
int main() {
  using namespace mmpt;
  const AttnSwitches sw;
  for (long d : {64, 80, 128, 256})
    for (int varlen = 0; varlen < 2; ++varlen) {
      const AttnPlan a = attn_plan(2, 130, 3, d, varlen, 64, true, sw);
      const AttnPlan b = attn_plan(2, 130, 3, d, varlen, 64, true, sw, true);
      std::printf("%ld %d %d %d %d %d %lld %d\n", d, varlen, (int)a.family, (int)b.family,
                  (int)b.fused_rope, (int)b.dropout, (long long)b.workspace_bytes, b.D * 1000 + b.DR);
    }
}
"""


def test_plan_argument(tmp_path):
    src, out = str(tmp_path / "p.cpp"), str(tmp_path / "p")
    with open(src, "w") as f:
        f.write(PLAN_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-I", CSRC, src, "-o", out], check=True)
    rows = [[int(x) for x in ln.split()] for ln in
            subprocess.run([out], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert len(rows) == 8
    for d, varlen, fam_off, fam_on, fused, drop, ws, dd in rows:
        assert fam_on == 0 and fused == 0 and drop == 1  # RING_RECOMPUTE, no fused rope
        assert ws == 2 * 130 * 3 * 4  # delta only
        assert dd == {64: 64064, 80: 128080, 128: 128128, 256: 256256}[d]
        assert fam_off == (2 if d == 256 and not varlen else 0)  # PAIR_DS without dropout


# ------------------------------------------------------------------ config
def test_config_fields_and_presets():
    from multimodal_llm_pretraining_amd import config as C

    for name in ("tiny-mm", "tiny-lm", "tiny-llama", "tiny-vit-cls", "llava-pretrain", "pythia-1b",
                 "tiny-mm-drop", "vit-l16-cls"):
        cfg = C.get_config(name)
        assert cfg.text is None or cfg.text.attn_dropout == 0.0
        assert cfg.vision is None or cfg.vision.attention_dropout == 0.0
    mm = C.get_config("tiny-mm-adrop")
    assert (mm.text.hidden_dropout, mm.text.attn_dropout, mm.vision.hidden_dropout,
            mm.vision.attention_dropout) == (0.1, 0.1, 0.1, 0.1)
    assert mm == C.with_dropout(C.get_config("tiny-mm"), 0.1, 0.1, text_attention=0.1,
                                vision_attention=0.1)
    assert C.get_config("tiny-lm-adrop") == C.with_dropout(C.get_config("tiny-lm"), text_attention=0.1)
    assert C.get_config("tiny-lm-adrop").text.hidden_dropout == 0.0
    # the text side's field is attn_dropout: tests/test_dropout_cpu.py pins that a TextConfig has
    # no attribute named attention_dropout
    assert not hasattr(mm.text, "attention_dropout") and hasattr(mm.vision, "attention_dropout")
    ll = C.get_config("tiny-llama-adrop")  # Llama has attention dropout but no hidden dropout
    assert ll.text.llama and ll.text.attn_dropout == 0.1
    vc = C.get_config("tiny-vit-cls-adrop")
    assert vc.classifier and vc.vision.attention_dropout == 0.1 and vc.vision.hidden_dropout == 0.0
    for a, b in (("tiny-lm-adrop", "tiny-lm"), ("tiny-mm-adrop", "tiny-mm"),
                 ("tiny-llama-adrop", "tiny-llama"), ("tiny-vit-cls-adrop", "tiny-vit-cls")):
        assert C.param_shapes(C.get_config(a)) == C.param_shapes(C.get_config(b))
        assert C.with_dropout(C.get_config(a)) == C.get_config(b)  # the defaults switch it off
    # a CLIP tower takes attention dropout (CLIPVisionConfig.attention_dropout)
    assert C.with_dropout(C.get_config("tiny-clip-d80"), vision_attention=0.2).vision.attention_dropout == 0.2
    # existing calls are unchanged
    assert C.with_dropout(C.get_config("tiny-mm"), text=0.1, vision=0.1) == C.get_config("tiny-mm-drop")


def test_config_validation():
    from multimodal_llm_pretraining_amd import config as C

    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="attention_dropout"):
            C.TextConfig(attn_dropout=bad)
        with pytest.raises(ValueError, match="attention_dropout"):
            C.VisionConfig(attention_dropout=bad)
        with pytest.raises(ValueError, match="attention_dropout"):
            C.with_dropout(C.get_config("tiny-mm"), text_attention=bad)
    with pytest.raises(ValueError, match="attention_dropout"):
        C.with_dropout(C.get_config("tiny-lm"), vision_attention=0.1)
    with pytest.raises(ValueError, match="attention_dropout"):
        C.with_dropout(C.get_config("tiny-vit-cls"), text_attention=0.1)
    with pytest.raises(TypeError):
        C.with_dropout(C.get_config("tiny-mm"), 0.1, 0.1, 0.1)  # keyword-only


def test_engine_site_is_k2():
    from multimodal_llm_pretraining_amd.engine import VISION_UNIT, dropout_site

    hidden = {dropout_site(5, 1, u, k) for u in (0, 1, 2, VISION_UNIT, VISION_UNIT + 1) for k in (0, 1)}
    attn = {dropout_site(5, 1, u, 2) for u in (1, 2, VISION_UNIT + 1)}
    assert not hidden & attn and len(attn) == 3


# ------------------------------------------------------------------ header / binding
def test_header_and_binding_agree():
    from multimodal_llm_pretraining_amd import _lib

    src = open(os.path.join(ROOT, "include", "mmpt.h")).read()
    assert re.search(r"#define MMPT_ABI_VERSION (\d+)", src).group(1) == "16"
    ctypes_of = {"int64_t": "I64", "double": "F64", "uint64_t": "U64", "int": "I32", "float": "F32"}
    for name in ("mmpt_attention_drop_fwd", "mmpt_attention_drop_bwd_workspace_bytes",
                 "mmpt_attention_drop_bwd", "mmpt_attn_dropout_mask", "mmpt_attn_dropout_p_eff"):
        m = re.search(r"\b(int|int64_t|double) " + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(2).split(",")]
        types = ["P" if "*" in a else ctypes_of[a.rsplit(" ", 1)[0]] for a in args]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is getattr(_lib, ctypes_of[m.group(1)]), name
        assert argtypes == [getattr(_lib, t) for t in types], (name, types)
    lib = _lib.load()
    for p in (0.0, 0.001, 0.1, 0.5, 0.999):
        assert lib.mmpt_attn_dropout_p_eff(p) == DR.p_eff(p)


def test_workspace_query():
    from multimodal_llm_pretraining_amd import _lib

    delta = 2 * 130 * 3 * 4
    for d in (64, 80, 128, 256):
        for varlen in (0, 1):
            assert _lib.query("mmpt_attention_drop_bwd_workspace_bytes", 2, 130, 3, d, varlen, 0.1) == delta
            plain = _lib.query("mmpt_attention_varlen_bwd_workspace_bytes" if varlen else
                               "mmpt_attention_bwd_workspace_bytes", 2, 130, 3, d)
            for p in (0.0, 0.001):  # t8 == 0: the plain entry's
                assert _lib.query("mmpt_attention_drop_bwd_workspace_bytes", 2, 130, 3, d, varlen, p) == plain


# ------------------------------------------------------------------ rounding-model pin
def _case(S, causal, p, seed, D=64, B=2, H=3):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).to(AR.BF16)  # noqa: E731
    q, k, v, do = rnd(B, H, S, D), rnd(B, H, S, D), rnd(B, H, S, D), rnd(B, H, S, D)
    keep = torch.from_numpy(DR.keep_mask(B, H, S, S, p, SEED, SITE))
    s = DR.scale_of(p)
    scale = D ** -0.5
    ref = DR.reference(q, k, v, do, causal, scale, keep, s)
    rs = DR.row_scales(ref, q, k, v, do, scale)
    models = [DR.model_plain(q, k, v, do, causal, scale, keep, s),
              DR.model_blocked(q, k, v, do, causal, scale, keep, s)]
    return ref, rs, models


PIN = [(S, causal, p) for S in (5, 65, 130) for causal in (True, False) for p in (0.1, 0.5)]
WORST = {}


@pytest.mark.parametrize("S,causal,p", PIN)
def test_rounding_models_pin(S, causal, p):
    ref, rs, models = _case(S, causal, p, seed=S + 7)
    worst = 0.0
    for m in models:
        for what in ("O", "dQ", "dK", "dV"):
            worst = max(worst, float(AR.row_ratios(getattr(m, what), getattr(ref, what),
                                                   getattr(rs, what)).max()))
        assert float((m.lse.double() - ref.lse).abs().max()) < 1e-5  # the undropped logsumexp
    WORST[(S, causal, p)] = worst
    print(f"S={S} causal={causal} p={p}: worst ratio {worst:.3f}")
    # FACTOR stays 2.5 while the torch models stay within 1.25 (attn_dropout_ref's docstring)
    assert worst <= 1.25, worst
    assert DR.FACTOR == 2.5


def test_unmasked_reference_is_told_apart():
    """The bars are not vacuous: a masked model against the reference WITHOUT the mask fails them."""
    S, causal, p = 65, True, 0.1
    _, _, models = _case(S, causal, p, seed=S + 7)
    g = torch.Generator().manual_seed(S + 7)
    rnd = lambda *s: torch.randn(*s, generator=g).to(AR.BF16)  # noqa: E731
    q, k, v, do = rnd(2, 3, S, 64), rnd(2, 3, S, 64), rnd(2, 3, S, 64), rnd(2, 3, S, 64)
    plain = AR.reference(q, k, v, do, causal, 64 ** -0.5)
    prs = AR.row_scales(plain, q, k, v, do, 64 ** -0.5)
    for what in ("O", "dQ", "dK", "dV"):
        assert float(AR.row_ratios(getattr(models[0], what), getattr(plain, what),
                                   getattr(prs, what)).max()) > 4 * DR.FACTOR, what
