"""ConvNeXt off the GPU: the `convnext-*` recipes against the reference's constants
(src/models/convnext.py:18-115), the parameter layout against HF's parameter count, the FLOP
formula against FlopCounterMode (the reference's own counter), the CPU oracle of
tests/convnext_oracle.py against live `ConvNextForImageClassification`, the K21 declarations, the
sharding refusals and the sweep CLI."""

import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_oracle as CO  # noqa: E402

from multimodal_llm_pretraining_amd import config as C  # noqa: E402

REFERENCE = ("convnext-large-1k", "convnext-large-22k", "convnext-xlarge-22k")
RECIPES = {  # name: (hidden_sizes, classes, training steps, warmup steps)
    "convnext-large-1k": ((192, 384, 768, 1536), 1000, 93600, 312 * 20),
    "convnext-large-22k": ((192, 384, 768, 1536), 21841, 311940, 3466 * 5),
    "convnext-xlarge-22k": ((256, 512, 1024, 2048), 21841, 311940, 3466 * 5),
}


# ------------------------------------------------------------------ recipe
@pytest.mark.parametrize("name", REFERENCE)
def test_recipe_is_the_reference(name):
    from multimodal_llm_pretraining_amd import models as M

    hs, classes, steps, warm = RECIPES[name]
    mc = M.get_model_class(name)
    assert mc.batch_size == 4096 and mc.training_steps == steps
    assert mc.mixed_precision is None
    assert mc.optimizer is torch.optim.AdamW
    assert mc.optimizer_kwargs == {"lr": 4e-3, "betas": (0.9, 0.999), "weight_decay": 0.05}
    assert mc.scheduler_type == "cosine" and mc.scheduler_kwargs == {"num_warmup_steps": warm}
    assert mc.max_grad_norm == 0.0 and mc.hf_training_args == {}
    assert mc.fsdp_layers_to_wrap == ["ConvNextStage"]
    assert mc.image_size == 224 and mc.num_classes == classes
    assert mc.supports_activation_checkpointing is True
    cfg = mc.model_config
    cn = cfg.convnext
    assert cfg.text is None and cfg.vision is None and cfg.classifier and not cfg.multimodal
    assert cfg.num_classes == classes
    assert cn.hidden_sizes == hs and cn.depths == (3, 3, 27, 3)
    assert (cn.image, cn.patch, cn.channels) == (224, 4, 3)
    assert (cn.eps, cn.head_eps, cn.layer_scale_init) == (1e-6, 1e-12, 1e-6)
    bf = M.get_model_class(name + "-bf16")
    assert bf.mixed_precision == "bf16" and bf.model_config == cfg
    for prop in ("batch_size", "training_steps", "optimizer", "optimizer_kwargs", "scheduler_type",
                 "scheduler_kwargs", "max_grad_norm", "fsdp_layers_to_wrap", "image_size",
                 "num_classes", "hf_training_args", "supports_activation_checkpointing"):
        assert getattr(bf, prop) == getattr(mc, prop), prop
    assert name not in M.OUT_OF_SCOPE and name + "-bf16" not in M.OUT_OF_SCOPE
    ds = mc.load_dummy_dataset()
    assert len(ds) == 20_000 and ds.image_size == 224 and ds.num_classes == classes


def test_out_of_scope_keeps_the_rest():
    from multimodal_llm_pretraining_amd import models as M

    assert set(M.OUT_OF_SCOPE) == {"mamba", "llava-finetune", "vilt-pretrain", "vilt-finetune",
                                   "vilt-original-pretrain", "vilt-original-finetune"}
    for name in M.OUT_OF_SCOPE:
        with pytest.raises(NotImplementedError):
            M.get_model_class(name)
    with pytest.raises(ValueError):
        M.get_model_class("convnext-huge")


@pytest.mark.parametrize("name", REFERENCE)
def test_fp32_recipe_is_refused(name):
    from multimodal_llm_pretraining_amd.experiments import TrainingConfig

    with pytest.raises(NotImplementedError, match="bf16"):
        TrainingConfig(1, 8, "mi355x", name).training_class().build_trainer(None, None)
    tc = TrainingConfig(1, 8, "mi355x", name + "-bf16").training_class()
    assert tc.bf16 and not tc.fp16 and not tc.max_grad_norm


# ------------------------------------------------------------------ config
def test_config_combinations():
    cn = C.get_config("tiny-convnext").convnext
    assert (cn.hidden_sizes, cn.depths, cn.image) == ((24, 48, 96, 192), (1, 1, 3, 1), 64)
    assert [cn.side(s) for s in range(4)] == [16, 8, 4, 2] and cn.patch_k == 48
    cfg = C.ModelConfig(convnext=cn, num_classes=5)
    assert cfg.classifier and not cfg.multimodal and cfg.classes_padded == 8
    v = C.get_config("tiny-vit-cls").vision
    for kw in (dict(convnext=cn), dict(convnext=cn, num_classes=0),
               dict(convnext=cn, vision=v, num_classes=5),
               dict(convnext=cn, text=C.TextConfig(), num_classes=5),
               dict(convnext=cn, num_classes=5, freeze_tower_and_llm=True),
               # every existing error still raises
               dict(), dict(vision=v), dict(num_classes=5), dict(text=C.TextConfig(), num_classes=5),
               dict(text=C.TextConfig(), vision=v, num_classes=5)):
        with pytest.raises(ValueError):
            C.ModelConfig(**kw)
    for kw in (dict(hidden_sizes=(24, 48, 96)), dict(hidden_sizes=(24, 48, 96, 100)),
               dict(depths=(1, 1, 0, 1)), dict(image=60)):
        with pytest.raises(ValueError):
            C.ConvNextConfig(**kw)
    with pytest.raises(ValueError):
        C.with_dropout(C.get_config("tiny-vit-cls"), text=0.1)
    assert C.get_config("tiny-vit-cls").convnext is None and C.get_config("tiny-lm").convnext is None


def test_param_names_and_fp32_region():
    from multimodal_llm_pretraining_amd.params import ParamStore, is_fp32_read
    from multimodal_llm_pretraining_amd.zero3 import unit_of

    cfg = C.get_config("tiny-convnext")
    s = C.param_shapes(cfg)
    assert s["convnext.stem.weight"] == (24, 48) and s["convnext.stem_ln.bias"] == (24,)
    assert "convnext.stages.0.down.weight" not in s
    assert s["convnext.stages.1.down.weight"] == (48, 96) and s["convnext.stages.1.down_ln.weight"] == (24,)
    assert s["convnext.stages.2.layers.2.dw.weight"] == (49, 96)
    assert s["convnext.stages.2.layers.2.fc1.weight"] == (384, 96)
    assert s["convnext.stages.2.layers.2.fc2.weight"] == (96, 384)
    assert s["convnext.stages.3.layers.0.gamma"] == (192,)
    assert s["cls_head.weight"] == (1008, 192) and s["cls_head.bias"] == (1008,)
    assert not any(n.startswith(("vision.", "proj.", "text.")) for n in s)
    f32 = {n for n in s if is_fp32_read(n)}
    assert f32 == {n for n in s if n.endswith(".gamma") or "ln." in n or "ln_post." in n}
    assert not any(".dw." in n or ".fc" in n or ".down." in n or ".stem." in n for n in f32)
    units = {unit_of(n) for n in s}
    assert units == {None, "convnext.stem", "cls_head"} | {f"convnext.stages.{i}" for i in range(4)}
    store = ParamStore(s, "meta")
    from multimodal_llm_pretraining_amd.engine import Engine

    eng = Engine(cfg, store)
    assert eng.unit_order() == ["convnext.stem"] + [f"convnext.stages.{i}" for i in range(4)] + \
        ["cls_head"]
    assert "convnext.stem.weight" not in store.transposed
    assert not any(n.endswith("dw.weight") for n in store.transposed)
    assert "convnext.stages.1.down.weight" in store.transposed and "cls_head.weight" in store.transposed


@pytest.mark.parametrize("name", REFERENCE)
def test_param_count_is_hfs(name):
    from multimodal_llm_pretraining_amd.models import build_hf_model

    cfg = C.get_config(name)
    with torch.device("meta"):
        m = build_hf_model(cfg)
    hf = sum(p.numel() for p in m.parameters())
    pad = cfg.classes_padded - cfg.num_classes  # class pad rows: weights and biases
    assert C.num_params(cfg) - pad * (cfg.convnext.hidden_sizes[-1] + 1) == hf
    sd = m.state_dict()
    shapes = C.param_shapes(cfg)
    assert len(sd) == len(shapes)
    assert m.config.hidden_sizes == list(cfg.convnext.hidden_sizes)
    assert m.config.depths == list(cfg.convnext.depths) and m.config.num_labels == cfg.num_classes
    assert m.config.layer_norm_eps == 1e-12 and m.config.drop_path_rate == 0.0


def test_init_follows_hf():
    from multimodal_llm_pretraining_amd.params import ParamStore, init_normal

    cfg = C.get_config("tiny-convnext")
    store = ParamStore(C.param_shapes(cfg), "cpu")
    store.refresh_shadow = lambda: None  # (the cast runs in the device library)
    init_normal(store, 0, cfg=cfg)
    for name in store.shapes:
        t = store.p(name)
        if name.endswith(".gamma"):
            assert torch.all(t == 1e-6), name
        elif name.endswith(".bias"):
            assert torch.count_nonzero(t) == 0, name
        elif "ln" in name.split(".")[-2]:
            assert torch.all(t == 1), name
        else:
            assert 0.015 < t[:cfg.num_classes].std().item() < 0.025, name
    assert torch.count_nonzero(store.p("cls_head.weight")[1001:]) == 0


# ------------------------------------------------------------------ flops
def test_flops_are_the_reference_counters():
    from torch.utils.flop_counter import FlopCounterMode

    from multimodal_llm_pretraining_amd.benchmarking import count_flops_per_example
    from multimodal_llm_pretraining_amd.models import build_hf_model, get_model_class

    cfg = C.get_config("tiny-convnext")
    m = build_hf_model(cfg).train()
    for bsz in (1, 2):
        batch = CO.make_batch(cfg, bsz, seed=1)
        m.zero_grad()
        with FlopCounterMode(display=False) as fc:
            m(**batch).loss.backward()
        assert fc.get_total_flops() == bsz * C.flops_per_sample(cfg, 0), bsz
    # the counter reports the depthwise weight gradient at C times its MACs; executed: once
    over = sum(d * 2 * cfg.convnext.side(s) ** 2 * c * 49 * (c - 1)
               for s, (c, d) in enumerate(zip(cfg.convnext.hidden_sizes, cfg.convnext.depths)))
    assert C.executed_flops_per_sample(cfg, 0) == C.flops_per_sample(cfg, 0) - over
    big = C.get_config("convnext-large-22k")
    assert count_flops_per_example(get_model_class("convnext-large-22k-bf16")) == \
        C.flops_per_sample(big, 0)


# ------------------------------------------------------------------ oracle vs HF
def test_oracle_matches_hf():
    from multimodal_llm_pretraining_amd.models import build_hf_model

    torch.manual_seed(0)
    cfg = C.get_config("tiny-convnext")
    P = CO.init_params(cfg, seed=0)
    assert torch.all(P["cls_head.weight"][1001:] == 0) and torch.all(P["cls_head.bias"][1001:] == 0)
    g = P["convnext.stages.2.layers.1.gamma"]
    assert 0.5 <= float(g.min()) and float(g.max()) < 1.5
    m = build_hf_model(cfg).eval()
    m.load_state_dict(CO.to_hf(P, cfg, m.state_dict()))
    batch = CO.make_batch(cfg, 3, seed=1)
    with torch.no_grad():
        hf32 = m(**batch).loss.item()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            hf16 = m(**batch).loss.item()
        o32 = CO.forward_loss(P, cfg, batch, "fp32").item()
        o16 = CO.forward_loss(P, cfg, batch, "bf16", ln_policy="cpu").item()
        o16_cuda = CO.forward_loss(P, cfg, batch, "bf16", ln_policy="cuda").item()
    print(f"fp32 {o32:.7f} / HF {hf32:.7f}; bf16 cpu-policy {o16:.7f} / HF {hf16:.7f}; "
          f"cuda-policy {o16_cuda:.7f}")
    assert abs(o32 - hf32) < 2e-6, (o32, hf32)
    assert abs(o16 - hf16) < 2e-6, (o16, hf16)
    assert abs(o16_cuda - o32) < 0.05  # the other policy is still this model
    _, G = CO.loss_and_grads(P, cfg, batch, "fp32")
    assert torch.count_nonzero(G["cls_head.weight"][1001:]) == 0
    assert torch.count_nonzero(G["cls_head.bias"][1001:]) == 0
    m.zero_grad()
    m(**batch).loss.backward()
    assert all(p.grad is not None for p in m.parameters())
    hf_g = CO.from_hf({n: p.grad for n, p in m.named_parameters()}, cfg)
    assert set(hf_g) == set(G)
    for n, ref in hf_g.items():
        err = ((G[n] - ref).norm() / (ref.norm() + 1e-6)).item()
        assert err < 1e-5, (n, err)
        assert ref.norm() > 0, n  # the block branch reaches the loss (gamma is not 1e-6 here)
    back = CO.from_hf(CO.to_hf(P, cfg, m.state_dict()), cfg)
    assert all(torch.equal(back[n], P[n]) for n in P)


def test_cosine_schedule_helper_is_the_trainers():
    from multimodal_llm_pretraining_amd.optim import lr_lambda

    for warm, total in ((0, 4), (2, 10), (3466 * 5, 311940)):
        want = [4e-3 * lr_lambda("cosine", i, warm, total) for i in range(6)]
        assert CO.cosine_lrs(4e-3, warm, total, 6) == pytest.approx(want, rel=1e-12, abs=0)


# ------------------------------------------------------------------ batch
def test_image_batch_on_the_host():
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg = C.get_config("tiny-convnext")
    bd = CO.make_batch(cfg, 4, seed=1)
    b = Batch(cfg, None, bd["labels"], bd["pixel_values"], "cpu")
    assert (b.B, b.S, b.T, b.num_items) == (4, 256, 1024, 4)
    assert b.ids is None and b.segments == () and b.pixels.dtype == torch.float32
    with pytest.raises(ValueError, match="pixel_values shape"):
        Batch(cfg, None, bd["labels"], torch.rand(4, 3, 48, 48), "cpu")
    with pytest.raises(ValueError, match="input_ids"):
        Batch(cfg, torch.zeros(4, 8, dtype=torch.int64), bd["labels"], bd["pixel_values"], "cpu")
    bad = bd["labels"].clone()
    bad[1] = 1001
    with pytest.raises(ValueError, match=r"\[0, 1001\)"):
        Batch(cfg, None, bad, bd["pixel_values"], "cpu")


# ------------------------------------------------------------------ K21 surface
K21 = (("mmpt_dwconv7_fwd", 9), ("mmpt_dwconv7_bwd_input", 9),
       ("mmpt_dwconv7_bwd_weight_workspace_bytes", 4), ("mmpt_dwconv7_bwd_weight", 10),
       ("mmpt_layerscale_add_fwd", 8), ("mmpt_layerscale_bwd_workspace_bytes", 2),
       ("mmpt_layerscale_bwd", 11), ("mmpt_ln16_bwd_workspace_bytes", 2), ("mmpt_ln16_bwd", 15),
       ("mmpt_avgpool_fwd", 6), ("mmpt_avgpool_bwd", 6), ("mmpt_patchify2_nhwc", 7),
       ("mmpt_unpatchify2_nhwc", 7))


def test_k21_entry_points_are_declared_and_bound():
    from multimodal_llm_pretraining_amd import _lib
    from multimodal_llm_pretraining_amd import kernels as K

    src = open(os.path.join(ROOT, "include", "mmpt.h")).read()
    for name, nargs in K21:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"#define\s+MMPT_ABI_VERSION\s+16\b", src) and _lib.ABI_VERSION == 16
    for fn in ("dwconv7_fwd", "dwconv7_bwd_input", "dwconv7_bwd_weight", "layerscale_add_fwd",
               "layerscale_bwd", "ln16_bwd", "avgpool_fwd", "avgpool_bwd", "patchify2_nhwc",
               "unpatchify2_nhwc"):
        assert callable(getattr(K, fn)), fn
    mk = open(os.path.join(ROOT, "multimodal_llm_pretraining_amd", "csrc", "Makefile")).read()
    assert "convnext.hip" in mk


# ------------------------------------------------------------------ sharding refusal
@pytest.mark.parametrize("sharding", ["zero_2", "zero_3", "fsdp_shard_grad_op", "fsdp_full_shard"])
def test_unit_sharding_is_refused(sharding):
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    with pytest.raises(NotImplementedError, match="tiny-convnext") as e:
        # device "meta": the refusal comes before any buffer is built
        ManualTrainer(StepConfig(model="tiny-convnext", sharding=sharding), AdamConfig(), "meta")
    assert sharding in str(e.value)


# ------------------------------------------------------------------ CLI
def test_cli_lists_and_counts(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import benchmark

    names = benchmark.model_types()
    for n in REFERENCE:
        assert n in names and n + "-bf16" in names
    benchmark.main(["--num-nodes", "1", "--gpus-per-node", "8", "--gpu-type", "mi355x",
                    "--model", "convnext-large-22k-bf16", "--methods", "all", "--cmd", "count"])
    assert "cached experiments: 0 /" in capsys.readouterr().out
