"""The vision-only classifier off the GPU: the `vit` / `vit-bf16` recipes against the
reference's constants (src/models/vit.py:9-69), the parameter layout against HF's parameter
count, the CPU oracle of tests/vit_cls_oracle.py against live `ViTForImageClassification`,
the FLOP formulas, the dummy dataset, the image batch's errors, the sharding refusals and the
sweep CLI."""

import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vit_cls_oracle as VO  # noqa: E402

from multimodal_llm_pretraining_amd import config as C  # noqa: E402


# ------------------------------------------------------------------ recipe
def test_vit_recipe_is_the_reference():
    from multimodal_llm_pretraining_amd import models as M

    mc = M.get_model_class("vit")
    assert mc.batch_size == 4096 and mc.training_steps == 311948
    assert mc.mixed_precision is None
    assert mc.optimizer is torch.optim.Adam
    assert mc.optimizer_kwargs == {"lr": 1e-3, "betas": (0.9, 0.999), "weight_decay": 0.03}
    assert mc.scheduler_type == "linear" and mc.scheduler_kwargs == {"num_warmup_steps": 10000}
    assert mc.max_grad_norm == 1.0 and mc.hf_training_args == {}
    assert mc.fsdp_layers_to_wrap == ["ViTLayer"]
    assert mc.image_size == 224 and mc.num_classes == 21841
    cfg = mc.model_config
    v = cfg.vision
    assert cfg.text is None and cfg.classifier and cfg.num_classes == 21841
    assert (v.hidden, v.layers, v.heads, v.ffn, v.image, v.patch) == (1024, 24, 16, 4096, 224, 16)
    assert v.eps == 1e-12 and v.hidden_dropout == 0.1 and v.used_layers == 24
    bf = M.get_model_class("vit-bf16")
    assert bf.mixed_precision == "bf16" and bf.model_config == cfg
    for prop in ("batch_size", "training_steps", "optimizer", "optimizer_kwargs", "scheduler_type",
                 "scheduler_kwargs", "max_grad_norm", "fsdp_layers_to_wrap", "image_size",
                 "num_classes", "hf_training_args"):
        assert getattr(bf, prop) == getattr(mc, prop), prop
    assert "vit" not in M.OUT_OF_SCOPE and "vit-bf16" not in M.OUT_OF_SCOPE
    ds = mc.load_dummy_dataset()
    assert len(ds) == 20_000 and ds.image_size == 224 and ds.num_classes == 21841


def test_fp32_recipe_is_refused():
    from multimodal_llm_pretraining_amd.experiments import TrainingConfig

    with pytest.raises(NotImplementedError, match="bf16"):
        TrainingConfig(1, 8, "mi355x", "vit").training_class().build_trainer(None, None)
    tc = TrainingConfig(1, 8, "mi355x", "vit-bf16").training_class()
    assert tc.bf16 and not tc.fp16 and tc.max_grad_norm == 1.0


# ------------------------------------------------------------------ layout
def test_config_combinations():
    v = C.get_config("tiny-vit-cls").vision
    for kw in (dict(), dict(vision=v), dict(num_classes=5), dict(text=C.TextConfig(), num_classes=5),
               dict(text=C.TextConfig(), vision=v, num_classes=5)):
        with pytest.raises(ValueError):
            C.ModelConfig(**kw)
    cfg = C.ModelConfig(vision=v, num_classes=5)
    assert cfg.classifier and cfg.multimodal and cfg.classes_padded == 8
    assert C.with_dropout(C.get_config("tiny-vit-cls"), vision=0.1) == C.get_config("tiny-vit-cls-drop")
    with pytest.raises(ValueError):
        C.with_dropout(C.get_config("tiny-vit-cls"), text=0.1)


def test_param_shapes_and_count():
    from transformers import ViTConfig, ViTForImageClassification

    s = C.param_shapes(C.get_config("tiny-vit-cls"))
    assert list(s)[-4:] == ["vision.ln_post.weight", "vision.ln_post.bias", "cls_head.weight",
                            "cls_head.bias"]
    assert s["cls_head.weight"] == (1008, 128) and s["cls_head.bias"] == (1008,)
    assert s["vision.pos"] == (17, 128)
    assert not any(n.startswith(("proj.", "text.")) for n in s)
    cfg = C.get_config("vit-l16-cls")
    s = C.param_shapes(cfg)
    assert s["cls_head.weight"] == (21848, 1024) and s["cls_head.bias"] == (21848,)
    with torch.device("meta"):
        m = ViTForImageClassification(ViTConfig(
            hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
            image_size=224, patch_size=16, num_labels=21841))
    hf = sum(p.numel() for p in m.parameters())
    assert C.num_params(cfg) - 7 * 1024 - 7 == hf


# ------------------------------------------------------------------ oracle vs HF
def test_oracle_matches_hf():
    from multimodal_llm_pretraining_amd.models import build_hf_model

    torch.manual_seed(0)
    cfg = C.get_config("tiny-vit-cls")
    P = VO.init_params(cfg, seed=0)
    assert torch.all(P["cls_head.weight"][1001:] == 0) and torch.all(P["cls_head.bias"][1001:] == 0)
    m = build_hf_model(cfg).eval()
    m.config._attn_implementation = "sdpa"
    m.load_state_dict(VO.to_hf(P, cfg, m.state_dict()))
    batch = VO.make_batch(cfg, 3, seed=1)
    with torch.no_grad():
        hf32 = m(**batch).loss.item()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            hf16 = m(**batch).loss.item()
        o32 = VO.forward_loss(P, cfg, batch, "fp32").item()
        o16 = VO.forward_loss(P, cfg, batch, "bf16").item()
    assert abs(o32 - hf32) < 2e-6, (o32, hf32)
    assert abs(o16 - hf16) < 2e-6, (o16, hf16)
    _, G = VO.loss_and_grads(P, cfg, batch, "fp32")
    assert torch.count_nonzero(G["cls_head.weight"][1001:]) == 0
    assert torch.count_nonzero(G["cls_head.bias"][1001:]) == 0
    m.zero_grad()
    m(**batch).loss.backward()
    assert all(p.grad is not None for p in m.parameters())
    # compared tensor by tensor of the oracle's own layout, where q|k|v are one stacked tensor:
    # the key bias alone has an analytically zero gradient (softmax is invariant to it), so on
    # its own both sides hold nothing but rounding noise of ~1e-9 and a relative error of it
    # says nothing; inside qkv.bias it is held to the same absolute scale as its neighbours
    hf_g = VO.from_hf({n: p.grad for n, p in m.named_parameters()}, cfg)
    assert set(hf_g) == set(G)
    for n, ref in hf_g.items():
        err = ((G[n] - ref).norm() / (ref.norm() + 1e-6)).item()
        assert err < 1e-5, (n, err)
    # and the mapping round-trips
    back = VO.from_hf(VO.to_hf(P, cfg, m.state_dict()), cfg)
    assert all(torch.equal(back[n], P[n]) for n in P)


def test_linear_schedule_helper_is_the_trainers():
    from multimodal_llm_pretraining_amd.optim import lr_lambda

    for warm, total in ((0, 4), (2, 10), (10000, 311948)):
        want = [1e-3 * lr_lambda("linear", i, warm, total) for i in range(5)]
        assert VO.linear_lrs(1e-3, warm, total, 5) == pytest.approx(want, rel=1e-12, abs=0)


# ------------------------------------------------------------------ flops
def test_flops():
    from multimodal_llm_pretraining_amd.benchmarking import count_flops_per_example
    from multimodal_llm_pretraining_amd.models import get_model_class

    cfg = C.get_config("tiny-vit-cls")
    # 16 patches of 3·16·16 -> 128; 3 layers over 17 tokens: qkv + o (4·128²), MLP (2·128·256),
    # scores + PV (4·17²·128); head 128 -> 1001
    patch = 2 * 16 * 128 * 768
    layer = 2 * 17 * 128 * (4 * 128 + 2 * 256) + 4 * 17 * 17 * 128
    want = 3.0 * (patch + 3 * layer + 2 * 128 * 1001)
    assert C.flops_per_sample(cfg, 0) == want
    assert C.executed_flops_per_sample(cfg, 0) == want
    big = C.get_config("vit-l16-cls")
    assert C.flops_per_sample(big, 0) == C.executed_flops_per_sample(big, 0)
    assert count_flops_per_example(get_model_class("vit-bf16")) == C.flops_per_sample(big, 0)


# ------------------------------------------------------------------ dataset
def test_dummy_dataset():
    from multimodal_llm_pretraining_amd.data import DummyImageClassificationDataset

    ds = DummyImageClassificationDataset(32, 7, num_samples=50, seed=3)
    assert len(ds) == 50
    a, b = ds[4], ds[4]
    assert set(a) == {"pixel_values", "labels"}
    assert a["pixel_values"].shape == (3, 32, 32) and a["pixel_values"].dtype == torch.float32
    assert a["labels"].shape == () and a["labels"].dtype == torch.int64
    assert torch.equal(a["pixel_values"], b["pixel_values"]) and torch.equal(a["labels"], b["labels"])
    assert 0 <= float(a["pixel_values"].min()) and float(a["pixel_values"].max()) < 1
    labels = torch.stack([ds[i]["labels"] for i in range(50)])
    assert int(labels.min()) >= 0 and int(labels.max()) < 7 and labels.unique().numel() > 1
    assert not torch.equal(ds[4]["pixel_values"], ds[5]["pixel_values"])
    other = DummyImageClassificationDataset(32, 7, num_samples=50, seed=4)
    assert not torch.equal(other[4]["pixel_values"], a["pixel_values"])
    with pytest.raises(IndexError):
        ds[50]
    stacked = {k: torch.stack([ds[i][k] for i in range(4)]) for k in a}
    assert stacked["pixel_values"].shape == (4, 3, 32, 32) and stacked["labels"].shape == (4,)


# ------------------------------------------------------------------ batch errors
def test_image_batch_on_the_host():
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg = C.get_config("tiny-vit-cls")
    bd = VO.make_batch(cfg, 4, seed=1)
    b = Batch(cfg, None, bd["labels"], bd["pixel_values"], "cpu")
    assert (b.B, b.S, b.T, b.num_items, b.tokens) == (4, 17, 68, 4, 68)
    assert b.cu_seqlens is None and b.ids is None and b.segments == ()
    assert torch.equal(b.loss_labels, bd["labels"]) and b.pixels.dtype == torch.float32
    bad = bd["labels"].clone()
    bad[2] = 1001  # == num_classes: a pad row of the head
    with pytest.raises(ValueError, match=r"\[0, 1001\)"):
        Batch(cfg, None, bad, bd["pixel_values"], "cpu")
    bad[2] = -100
    with pytest.raises(ValueError, match=r"\[0, 1001\)"):
        Batch(cfg, None, bad, bd["pixel_values"], "cpu")
    with pytest.raises(ValueError, match="pixel_values shape"):
        Batch(cfg, None, bd["labels"], torch.rand(4, 3, 48, 48), "cpu")
    with pytest.raises(ValueError, match="input_ids"):
        Batch(cfg, torch.zeros(4, 8, dtype=torch.int64), bd["labels"], bd["pixel_values"], "cpu")
    with pytest.raises(ValueError, match="needs pixel_values"):
        Batch(cfg, None, bd["labels"], None, "cpu")
    with pytest.raises(ValueError, match="labels shape"):
        Batch(cfg, None, bd["labels"][:3], bd["pixel_values"], "cpu")
    with pytest.raises(ValueError, match="input_ids"):  # and a language model still needs them
        Batch(C.get_config("tiny-lm"), None, bd["labels"], None, "cpu")


# ------------------------------------------------------------------ sharding refusal
@pytest.mark.parametrize("sharding", ["zero_2", "zero_3", "fsdp_shard_grad_op", "fsdp_full_shard"])
def test_unit_sharding_is_refused(sharding):
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    with pytest.raises(NotImplementedError, match="tiny-vit-cls") as e:
        # device "meta": the refusal comes before any buffer is built
        ManualTrainer(StepConfig(model="tiny-vit-cls", sharding=sharding), AdamConfig(), "meta")
    assert sharding in str(e.value)


# ------------------------------------------------------------------ CLI
def test_cli_lists_and_counts(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import benchmark

    names = benchmark.model_types()
    assert "vit" in names and "vit-bf16" in names
    benchmark.main(["--num-nodes", "1", "--gpus-per-node", "8", "--gpu-type", "mi355x",
                    "--model", "vit-bf16", "--methods", "all", "--cmd", "count"])
    assert "cached experiments: 0 /" in capsys.readouterr().out


def test_k18_entry_points_are_declared_and_bound():
    import re

    from multimodal_llm_pretraining_amd import _lib

    src = open(os.path.join(ROOT, "include", "mmpt.h")).read()
    for name, nargs in (("mmpt_cls_ln_fwd", 12), ("mmpt_cls_ln_bwd_workspace_bytes", 2),
                        ("mmpt_cls_ln_bwd", 16)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
