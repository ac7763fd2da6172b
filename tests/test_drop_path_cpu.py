"""ConvNeXt stochastic depth without a GPU: the per-block rates against HF, the host keep rule
against the numpy restatement of tests/test_dropout_cpu.py, the config surface, the site numbering,
and tests/drop_path_ref.py against the live HF module in training mode (torch.rand inside
ConvNextDropPath.forward patched to give the wanted masks)."""

import itertools
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_oracle as CO  # noqa: E402
import drop_path_ref as DR  # noqa: E402
from test_dropout_cpu import keep_mask  # noqa: E402

from multimodal_llm_pretraining_amd import config as C  # noqa: E402
from multimodal_llm_pretraining_amd import droppath  # noqa: E402


# ------------------------------------------------------------------ rates
@pytest.mark.parametrize("depths", [(3, 3, 27, 3), (1, 1, 3, 1)])
@pytest.mark.parametrize("rate", [0.0, 0.1, 0.2, 0.5, 0.8])
def test_rates_are_hfs(depths, rate):
    from transformers import ConvNextConfig
    from transformers.models.convnext.modeling_convnext import ConvNextEncoder, ConvNextLayer

    cn = C.ConvNextConfig(hidden_sizes=(8, 8, 8, 8), depths=depths, image=32, drop_path_rate=rate)
    enc = ConvNextEncoder(ConvNextConfig(hidden_sizes=[8, 8, 8, 8], depths=list(depths),
                                         drop_path_rate=rate))
    # (a layer built with rate 0 holds nn.Identity, which has no drop_prob)
    hf = [getattr(m.drop_path, "drop_prob", 0.0) for m in enc.modules()
          if isinstance(m, ConvNextLayer)]
    got = cn.drop_path_rates()
    assert len(got) == sum(depths) and list(got) == hf
    assert got[0] == 0.0  # block 0 is never dropped
    assert all(isinstance(p, float) and float(np.float32(p)) == p for p in got)  # fp32 values
    assert list(got) == [float(torch.linspace(0, rate, sum(depths))[j]) for j in range(sum(depths))]


# ------------------------------------------------------------------ keep rule
def test_host_keep_rule_is_the_dropout_rule():
    from multimodal_llm_pretraining_amd.engine import VISION_UNIT, dropout_site

    sites = [0, 3, dropout_site(0, 0, VISION_UNIT + 1, 3), dropout_site(7, 2, VISION_UNIT + 36, 3),
             (1 << 64) - 1]
    for n, p, seed, site in itertools.product((1, 2, 5, 8, 64, 257), (0.0, 1e-10, 0.1, 0.5,
                                                                     0.800000011920929, 0.999),
                                              (0, 5, (1 << 63) + 12345), sites):
        got = droppath.keep_mask(n, p, seed, site)
        assert got.dtype == bool and got.shape == (n,)
        assert np.array_equal(got, keep_mask(n, p, seed, site)), (n, p, seed, site)
        assert droppath.kept_indices(n, p, seed, site) == tuple(np.flatnonzero(got))
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            droppath.keep_mask(4, bad, 0, 0)


def test_kept_counts_of_the_gpu_tests():
    """The masks the GPU tests run with (seed as given, step 0, rank 0): what they cover."""
    from multimodal_llm_pretraining_amd.engine import VISION_UNIT, dropout_site

    def counts(name, B, seed):
        pr = C.get_config(name).convnext.drop_path_rates()
        return [int(droppath.keep_mask(B, p, seed, dropout_site(0, 0, VISION_UNIT + 1 + j, 3)).sum())
                for j, p in enumerate(pr)]

    assert counts("tiny-convnext-dp", 8, 0) == [8, 6, 5, 3, 3, 4]
    assert counts("tiny-convnext-dp8", 2, 5) == [2, 1, 2, 2, 1, 0]
    assert counts("tiny-convnext-dp8", 2, 6) == [2, 1, 2, 0, 0, 0]


# ------------------------------------------------------------------ config surface
def test_config_field_presets_and_errors():
    base = C.get_config("tiny-convnext")
    assert base.convnext.drop_path_rate == 0.0 and C.ConvNextConfig().drop_path_rate == 0.0
    for name in ("convnext-large-1k", "convnext-large-22k", "convnext-xlarge-22k"):
        assert C.get_config(name).convnext.drop_path_rate == 0.0  # as the reference builds them
    dp, dp8 = C.get_config("tiny-convnext-dp"), C.get_config("tiny-convnext-dp8")
    assert dp == C.with_drop_path(base, 0.5) and dp8 == C.with_drop_path(base, 0.8)
    assert dp.convnext.drop_path_rate == 0.5 and dp8.convnext.drop_path_rate == 0.8
    assert C.with_drop_path(dp, 0.0) == base
    assert C.preset_name(dp) == "tiny-convnext-dp"
    assert C.param_shapes(dp) == C.param_shapes(base)
    # HF executes the whole block for every sample: the reference-convention count is unchanged
    assert C.flops_per_sample(dp, 0) == C.flops_per_sample(base, 0)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="drop_path_rate"):
            C.with_drop_path(base, bad)
        with pytest.raises(ValueError, match="drop_path_rate"):
            C.ConvNextConfig(drop_path_rate=bad)
    for name in ("tiny-lm", "tiny-mm", "tiny-vit-cls", "tiny-llama", "tiny-roberta", "tiny-mamba",
                 "tiny-clip-d80"):
        with pytest.raises(ValueError, match="drop path"):
            C.with_drop_path(C.get_config(name), 0.1)


def test_hf_model_gets_the_rate():
    from multimodal_llm_pretraining_amd.models import build_hf_model

    assert build_hf_model(C.get_config("tiny-convnext-dp")).config.drop_path_rate == 0.5
    assert build_hf_model(C.get_config("tiny-convnext")).config.drop_path_rate == 0.0


# ------------------------------------------------------------------ sites
def test_site_k3_is_injective_beside_the_others():
    from multimodal_llm_pretraining_amd.engine import VISION_UNIT, dropout_site

    seen = {}
    for step, rank, unit, k in itertools.product((0, 1, (1 << 32) - 1), (0, 1, 65535),
                                                 (0, 1, VISION_UNIT, VISION_UNIT + 1,
                                                  VISION_UNIT + 36, 4095), (0, 1, 2, 3)):
        s = dropout_site(step, rank, unit, k)
        assert 0 <= s < 1 << 64 and s not in seen, (step, rank, unit, k, seen.get(s))
        seen[s] = (step, rank, unit, k)
    blocks = {dropout_site(0, 0, VISION_UNIT + 1 + j, 3) for j in range(36)}
    assert len(blocks) == 36


# ------------------------------------------------------------------ the reference vs HF
def _rand_giving(masks):
    """A torch.rand stand-in: call i returns values whose floor(rand + keep_prob) is masks[i]."""
    it = iter(masks)

    def rand(shape, dtype=None, device=None):
        m = torch.tensor(next(it), dtype=torch.bool)
        assert tuple(shape) == (m.numel(), 1, 1, 1)
        return torch.where(m, 0.999, 0.0).to(dtype).view(shape)

    return rand


@pytest.mark.parametrize("name", ["tiny-convnext-dp", "tiny-convnext-dp8"])
def test_reference_matches_hf_in_training_mode(name):
    from multimodal_llm_pretraining_amd.models import build_hf_model

    cfg = C.get_config(name)
    P = CO.init_params(cfg, seed=0)
    B = 3
    batch = CO.make_batch(cfg, B, seed=1)
    pr = DR.rates(cfg)
    assert pr == list(cfg.convnext.drop_path_rates())
    # block 0 everybody (p = 0: HF draws nothing), then mixed, one block nobody, one everybody
    keep = [[True] * B, [True, False, True], [False, True, True], [False] * B, [True] * B,
            [False, False, True]]
    drawn = [k for k, p in zip(keep, pr) if p != 0.0]
    m = build_hf_model(cfg).train()
    m.load_state_dict(CO.to_hf(P, cfg, m.state_dict()))

    def hf_loss(autocast):
        with mock.patch("torch.rand", _rand_giving(drawn)):
            if autocast:
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    return m(**batch).loss
            return m(**batch).loss

    with torch.no_grad():
        hf32, hf16 = hf_loss(False).item(), hf_loss(True).item()
        o32 = DR.forward_loss(P, cfg, batch, keep, "fp32").item()
        o16 = DR.forward_loss(P, cfg, batch, keep, "bf16", ln_policy="cpu").item()
        dense = CO.forward_loss(P, cfg, batch, "fp32").item()
    print(f"{name}: fp32 {o32:.7f} / HF {hf32:.7f}; bf16 cpu-policy {o16:.7f} / HF {hf16:.7f}; "
          f"no drop path {dense:.7f}")
    assert abs(o32 - hf32) < 2e-6, (o32, hf32)
    assert abs(o16 - hf16) < 2e-6, (o16, hf16)
    assert abs(o32 - dense) > 1e-3  # the masks reach the loss
    _, G = DR.loss_and_grads(P, cfg, batch, keep, "fp32")
    m.zero_grad()
    hf_loss(False).backward()
    hf_g = CO.from_hf({n: (p.grad if p.grad is not None else torch.zeros_like(p))
                       for n, p in m.named_parameters()}, cfg)
    for n, ref in hf_g.items():
        err = ((G[n] - ref).norm() / (ref.norm() + 1e-6)).item()
        assert err < 1e-5, (n, err)
    # the block that kept nobody has exactly zero gradients, in HF and in the reference
    for n in G:
        if n.startswith("convnext.stages.2.layers.1."):
            assert torch.count_nonzero(G[n]) == 0 and torch.count_nonzero(hf_g[n]) == 0, n
    # all kept and rate 0: the plain oracle
    all_keep = [[True] * B] * len(pr)
    base = C.get_config("tiny-convnext")
    with torch.no_grad():
        assert DR.forward_loss(P, base, batch, all_keep, "bf16").item() == \
            CO.forward_loss(P, base, batch, "bf16").item()


# ------------------------------------------------------------------ C-ABI surface
ENTRIES = (("mmpt_dwconv7_idx_fwd", 11), ("mmpt_dwconv7_idx_bwd_input", 11),
           ("mmpt_dwconv7_idx_bwd_weight", 12), ("mmpt_droppath_add_fwd", 12),
           ("mmpt_droppath_bwd_workspace_bytes", 3), ("mmpt_droppath_bwd", 15))


def test_entry_points_are_declared_and_bound():
    import re

    from multimodal_llm_pretraining_amd import _lib
    from multimodal_llm_pretraining_amd import kernels as K

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "mmpt.h")).read()
    for name, nargs in ENTRIES:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    # new entries only: the ABI version stands, as for K20 and K21
    assert re.search(r"#define\s+MMPT_ABI_VERSION\s+16\b", src) and _lib.ABI_VERSION == 16
    for fn in ("dwconv7_idx_fwd", "dwconv7_idx_bwd_input", "dwconv7_idx_bwd_weight",
               "droppath_add_fwd", "droppath_bwd", "KeptSamples", "kept_samples_of"):
        assert callable(getattr(K, fn)), fn
    # the wrappers check the host copy of the map before anything is launched (no device needed)
    for idx in ((2, 0), (1, 1), (0, 3), (-1, 2)):
        with pytest.raises(ValueError, match="strictly increasing"):
            K._kept(K.KeptSamples(3, idx, "cpu"), 3, "t")
    K._kept(K.KeptSamples(3, (0, 2), "cpu"), 3, "t")
    ks = K.kept_samples_of(4, [(0, 3), (), (1, 2, 3)], "cpu")
    assert [k.idx_dev.tolist() for k in ks] == [[0, 3], [], [1, 2, 3]]
    assert [k.slot_dev.tolist() for k in ks] == [[0, -1, -1, 1], [-1] * 4, [-1, 0, 1, 2]]
