"""Mamba host layers without a GPU: the configuration and its presets, the parameter layout, the
`mamba` / `mamba-2.8b` naming, the recipe against the reference's constants, the CPU oracle
(tests/mamba_oracle.py) against the live HF module (fp32, and its own roundings under CPU
autocast), FLOP counts, the sharding refusals, the absolute-min_lr schedule against transformers'
scheduler, and the K22 header / binding agreement."""

import math
import os
import re
import sys
from dataclasses import replace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mamba_oracle as MO  # noqa: E402

from multimodal_llm_pretraining_amd import config as C  # noqa: E402
from multimodal_llm_pretraining_amd import models as M  # noqa: E402


# ------------------------------------------------------------------ configuration
def test_presets():
    t = C.get_config("mamba-2.8b").text
    assert (t.arch, t.hidden, t.layers, t.d_inner, t.d_state, t.d_conv, t.rank, t.vocab, t.eps) == \
        ("mamba", 2560, 64, 5120, 16, 4, 160, 50280, 1e-5)
    assert t.xproj_dim == 160 + 32 and t.tie_embeddings and t.n_vocab == 50280 and t.mamba
    s = C.get_config("tiny-mamba").text
    assert (s.hidden, s.layers, s.d_inner, s.d_state, s.d_conv, s.rank, s.vocab, s.n_vocab) == \
        (128, 2, 256, 16, 4, 8, 520, 515)
    assert replace(s, dt_rank=0, hidden=256).rank == 16  # "auto": ceil(hidden / 16)
    assert not C.get_config("tiny-llama").text.mamba


@pytest.mark.parametrize("bad", [dict(hidden_dropout=0.1), dict(attn_dropout=0.1),
                                 dict(tie_embeddings=False), dict(rotary_pct=0.25),
                                 dict(kv_heads=2), dict(d_conv=3), dict(d_state=12),
                                 dict(dt_rank=12), dict(hidden=130), dict(expand=0)])
def test_arch_check_rejects(bad):
    with pytest.raises(ValueError):
        replace(C.get_config("tiny-mamba").text, **bad)


def test_param_shapes_and_fp32_reads():
    from multimodal_llm_pretraining_amd.params import is_fp32_read

    cfg = C.get_config("tiny-mamba")
    s = C.param_shapes(cfg)
    p = "text.layers.1."
    assert {k[len(p):]: v for k, v in s.items() if k.startswith(p)} == {
        "norm.weight": (128,), "in_proj.weight": (512, 128), "conv.weight": (4, 256),
        "conv.bias": (256,), "x_proj.weight": (40, 256), "dt_proj.weight": (256, 8),
        "dt_proj.bias": (256,), "A_log": (256, 16), "D": (256,), "out_proj.weight": (128, 256)}
    assert s["text.embed"] == (520, 128) and s["text.final_ln.weight"] == (128,)
    assert "text.lm_head" not in s and len(s) == 2 + 10 * 2
    f32 = {k for k in s if is_fp32_read(k)}
    assert f32 == {"text.embed", "text.final_ln.weight"} | {
        f"text.layers.{i}.{n}" for i in range(2) for n in ("norm.weight", "A_log", "D",
                                                            "dt_proj.bias")}
    # nothing of another family became an fp32 read through the new suffixes
    for name in ("tiny-llama", "tiny-roberta", "tiny-convnext", "tiny-mm"):
        for k in C.param_shapes(C.get_config(name)):
            assert not k.endswith((".norm.weight", ".A_log", ".D", ".dt_proj.bias")), k


def test_parameter_count_matches_hf():
    from transformers import MambaForCausalLM

    with torch.device("meta"):
        m = M.build_hf_model(C.get_config("mamba-2.8b"))
    assert isinstance(m, MambaForCausalLM)
    c = m.config
    assert (c.vocab_size, c.hidden_size, c.num_hidden_layers, c.intermediate_size, c.state_size,
            c.conv_kernel, c.time_step_rank, c.use_bias, c.use_conv_bias, c.residual_in_fp32,
            c.tie_word_embeddings) == (50280, 2560, 64, 5120, 16, 4, 160, False, True, True, True)
    hf = sum(p.numel() for p in m.parameters())  # (the tied lm_head is the same Parameter)
    assert C.num_params(C.get_config("mamba-2.8b")) == hf == 2768345600


def test_init_follows_hf():
    from multimodal_llm_pretraining_amd.params import _mamba_init

    cfg = C.get_config("tiny-mamba")
    t = cfg.text
    g = torch.Generator().manual_seed(0)
    W = {n: _mamba_init(n, s, t, g) for n, s in C.param_shapes(cfg).items()}
    p = "text.layers.0."
    assert torch.equal(W[p + "A_log"][3], torch.log(torch.arange(1, 17.0)))
    assert bool((W[p + "D"] == 1).all()) and bool((W[p + "conv.bias"] == 0).all())
    assert bool((W[p + "norm.weight"] == 1).all()) and bool((W["text.final_ln.weight"] == 1).all())
    assert float(W[p + "conv.weight"].abs().max()) <= 0.5
    assert float(W[p + "dt_proj.weight"].abs().max()) <= t.rank ** -0.5
    assert float(W[p + "out_proj.weight"].abs().max()) <= t.d_inner ** -0.5
    dt = torch.nn.functional.softplus(W[p + "dt_proj.bias"])
    assert 1e-3 * 0.99 <= float(dt.min()) and float(dt.max()) <= 0.1 * 1.01
    assert 0.08 < float(W[p + "in_proj.weight"].std()) < 0.12  # initializer_range 0.1
    assert int(W["text.embed"][t.n_vocab:].count_nonzero()) == 0
    assert all(tuple(W[n].shape) == tuple(s) for n, s in C.param_shapes(cfg).items())


# ------------------------------------------------------------------ naming and recipe
def test_mamba_stays_refused_and_mamba_2_8b_is_served():
    assert "mamba" in M.OUT_OF_SCOPE and "mamba-2.8b" not in M.OUT_OF_SCOPE
    with pytest.raises(NotImplementedError):
        M.get_model_class("mamba")
    mc = M.get_model_class("mamba-2.8b")
    assert isinstance(mc, M.MambaModelClass) and mc.model_config is C.PRESETS["mamba-2.8b"]
    assert set(M.MambaT.__args__) == {"mamba-2.8b"}
    assert "mamba-2.8b" in M.__doc__ and "hub" in M.__doc__


def test_recipe_is_the_reference_file():
    mc = M.get_model_class("mamba-2.8b")
    assert (mc.batch_size, mc.training_steps, mc.mixed_precision) == (128, 572_204, "bf16")
    assert mc.optimizer is torch.optim.AdamW
    assert mc.optimizer_kwargs == {"lr": (1.6e-4) * 5, "weight_decay": 0.1, "betas": (0.9, 0.95)}
    assert mc.scheduler_type == "cosine_with_min_lr"
    assert mc.scheduler_kwargs == {"num_warmup_steps": 57220, "min_lr": 1e-5}
    assert mc.max_grad_norm == 1.0 and mc.fsdp_layers_to_wrap == ["MambaBlock"]
    assert (mc.vocab_size, mc.sequence_length) == (50265, 4096)
    assert not mc.supports_compilation and mc.supports_activation_checkpointing
    assert mc.hf_training_args == {}
    ds = mc.load_dummy_dataset(num_samples=4)
    assert len(ds) == 4 and ds[0]["input_ids"].shape == (4096,)


def test_training_arguments_export_and_cli(capsys):
    from multimodal_llm_pretraining_amd.experiments import TrainingConfig

    tc = TrainingConfig(1, 8, "mi355x", "mamba-2.8b").training_class()
    assert tc.bf16 and not tc.fp16 and not tc.compile and tc.max_grad_norm == 1.0
    assert tc.scheduler_kwargs["min_lr"] == 1e-5
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import benchmark

    assert "mamba-2.8b" in benchmark.model_types() and "mamba" not in benchmark.model_types()
    benchmark.main(["--num-nodes", "1", "--gpus-per-node", "8", "--gpu-type", "mi355x",
                    "--model", "mamba-2.8b", "--methods", "all", "--cmd", "count"])
    assert "cached experiments: 0 /" in capsys.readouterr().out


# ------------------------------------------------------------------ oracle vs live HF
@pytest.fixture(scope="module")
def live():
    from transformers import MambaForCausalLM

    cfg = C.get_config("tiny-mamba")
    P = MO.init_params(cfg, seed=0)
    hf = MambaForCausalLM(MO.hf_config(cfg))
    hf.load_state_dict(MO.to_hf(P, cfg, hf.state_dict()))
    hf.train()
    return cfg, P, hf, MO.make_batch(cfg, 3, 70, seed=1)


def test_init_params_make_every_path_matter(live):
    cfg, P, _, _ = live
    p = "text.layers.0."
    assert not torch.allclose(P[p + "A_log"][0], torch.log(torch.arange(1, 17.0)))
    assert float((P[p + "D"] - 1).abs().min()) > 0 and float(P[p + "conv.bias"].abs().min()) > 0
    dt = torch.nn.functional.softplus(P[p + "dt_proj.bias"])
    assert float(dt.min()) < 5e-3 and float(dt.max()) > 0.5
    back = MO.from_hf(MO.to_hf(P, cfg, live[2].state_dict()), cfg)
    assert all(torch.equal(back[k], P[k]) for k in P)


def test_oracle_fp32_matches_live_hf(live):
    cfg, P, hf, batch = live
    loss, G = MO.loss_and_grads(P, cfg, batch, "fp32")
    hf.zero_grad()
    out = hf(**batch)
    out.loss.backward()
    assert loss == pytest.approx(out.loss.item(), abs=2e-6)
    g = MO.from_hf({k: v.grad for k, v in hf.named_parameters()}, cfg)
    for k in P:
        err = ((G[k] - g[k]).norm() / (g[k].norm() + 1e-30)).item()
        assert err < 1e-5, (k, err)
        assert float(g[k].norm()) > 0, k


def test_oracle_hf_policy_matches_live_hf_under_autocast(live):
    cfg, P, hf, batch = live
    loss, G = MO.loss_and_grads(P, cfg, batch, "bf16", "hf")
    hf.zero_grad()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        out = hf(**batch)
    out.loss.backward()
    assert loss == pytest.approx(out.loss.item(), abs=1e-5)
    g = MO.from_hf({k: v.grad for k, v in hf.named_parameters()}, cfg)
    for k in P:
        assert ((G[k] - g[k]).norm() / (g[k].norm() + 1e-30)).item() < 1e-3, k


def test_fused_policy_stays_near_fp32(live):
    """The engine is held to "fused"; it is a bf16 implementation like the live module's: its loss
    lies within a few σ of fp32 and its gradients within the spread the two policies show."""
    cfg, P, _, batch = live
    l32, G32 = MO.loss_and_grads(P, cfg, batch, "fp32")
    lf, Gf = MO.loss_and_grads(P, cfg, batch, "bf16", "fused")
    sigma = MO.bf16_sigma(P, cfg, 3, 70)
    assert 1e-4 < sigma < 5e-3 and abs(lf - l32) < 1e-4 + 4 * sigma
    for k in P:
        assert ((Gf[k] - G32[k]).norm() / (G32[k].norm() + 1e-30)).item() < 5e-2, k


# ------------------------------------------------------------------ FLOPs, refusals, schedule
def test_flop_counts():
    cfg = C.get_config("mamba-2.8b")
    t, S = cfg.text, 4096
    I, R, N, h = 5120, 160, 16, 2560
    layer = 2 * S * (h * 2 * I + I * (R + 2 * N) + R * I + I * h)
    want = 3.0 * (64 * layer + 2 * S * h * 50280)
    assert C.flops_per_sample(cfg, S) == want == C.executed_flops_per_sample(cfg, S)
    # against 6 x matmul parameters x tokens (the embedding counted once, as the decoder)
    mat = sum(math.prod(s) for k, s in C.param_shapes(cfg).items()
              if k.endswith("_proj.weight") or k == "text.embed")
    assert want == 6.0 * mat * S
    assert "scan" in C._mamba_flops.__doc__ and "not counted" in C._mamba_flops.__doc__
    assert t.mamba


@pytest.mark.parametrize("sharding", ["zero_2", "zero_3", "fsdp_shard_grad_op", "fsdp_full_shard"])
def test_unit_sharding_is_refused(sharding):
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    with pytest.raises(NotImplementedError, match="mamba") as e:
        ManualTrainer(StepConfig(model="tiny-mamba", sharding=sharding), AdamConfig(), "meta")
    assert sharding in str(e.value)


def test_padded_batch_is_refused_on_the_host():
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg = C.get_config("tiny-mamba")
    b = MO.make_batch(cfg, 2, 9)
    mask = torch.ones(2, 9, dtype=torch.int64)
    Batch(cfg, b["input_ids"], b["labels"], None, "cpu", attention_mask=mask)
    mask[0, -2:] = 0
    with pytest.raises(ValueError, match="padded"):
        Batch(cfg, b["input_ids"], b["labels"], None, "cpu", attention_mask=mask)


def test_min_lr_schedule_matches_transformers():
    from transformers import get_scheduler

    from multimodal_llm_pretraining_amd.optim import Schedule, min_lr_rate_of

    lr, kw = 8e-4, {"min_lr": 1e-5}
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sch = get_scheduler("cosine_with_min_lr", opt, num_warmup_steps=4, num_training_steps=40,
                        scheduler_specific_kwargs=kw)
    mine = Schedule(lr, "cosine_with_min_lr", 4, 40, min_lr_rate_of(kw, lr))
    for _ in range(40):
        assert mine.lr() == pytest.approx(sch.get_last_lr()[0], rel=1e-12, abs=1e-18)
        opt.step()
        sch.step()
        mine.step()
    assert mine.lr() == pytest.approx(1e-5, rel=1e-9)
    assert min_lr_rate_of({"min_lr_rate": 0.1}, lr) == 0.1 and min_lr_rate_of({}, lr) == 0.0
    assert MO.cosine_min_lr(lr, 1e-5, 4, 40, 41)[-1] == pytest.approx(1e-5, rel=1e-9)


# ------------------------------------------------------------------ header / binding / wrappers
C_TYPES = {"int64_t": "I64", "void*": "P", "constvoid*": "P", "constfloat*": "P", "float*": "P"}
K22 = ["mmpt_causal_conv1d_fwd", "mmpt_causal_conv1d_bwd_workspace_bytes", "mmpt_causal_conv1d_bwd",
       "mmpt_selective_scan_chunk", "mmpt_selective_scan_states_bytes",
       "mmpt_selective_scan_fwd_workspace_bytes", "mmpt_selective_scan_fwd",
       "mmpt_selective_scan_bwd_workspace_bytes", "mmpt_selective_scan_bwd"]


def test_k22_header_binding_and_wrappers_agree():
    from multimodal_llm_pretraining_amd import _lib, kernels

    src = open(os.path.join(ROOT, "include", "mmpt.h")).read()
    assert re.search(r"#define MMPT_ABI_VERSION (\d+)", src).group(1) == "16"  # entries only added
    assert _lib.ABI_VERSION == 16 and "K22" in src
    for name in K22:
        m = re.search(r"\b(int|int64_t) " + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        args = [a.strip() for a in " ".join(m.group(2).split()).split(",")]
        args = [] if args == ["void"] else args
        names = [re.split(r"[ *]", a)[-1] for a in args]
        types = [C_TYPES["".join(a.rsplit(n, 1)[0].split())] for a, n in zip(args, names)]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is (_lib.I64 if m.group(1) == "int64_t" else _lib.I32), name
        assert argtypes == [getattr(_lib, t) for t in types], (name, types)
    for w in ("causal_conv1d_fwd", "causal_conv1d_bwd", "selective_scan_fwd", "selective_scan_bwd",
              "scan_chunk", "scan_states"):
        assert callable(getattr(kernels, w)), w
    mk = open(os.path.join(ROOT, "multimodal_llm_pretraining_amd", "csrc", "Makefile")).read()
    assert "mamba.hip" in mk
    if os.path.exists(_lib.LIB_PATH):  # the library itself exports them (when it has been built)
        lib = _lib.load()
        assert all(hasattr(lib, n) for n in K22)
        assert kernels.scan_chunk() == int(re.search(r"#define MMPT_SCAN_CHUNK (\d+)", src).group(1))


def test_wrappers_refuse_cpu_tensors():
    from multimodal_llm_pretraining_amd import kernels as K

    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)  # noqa: E731
    with pytest.raises(RuntimeError, match="GPU"):
        K.causal_conv1d_fwd(z(8, 16), z(4, 16), z(16), z(8, 16), 4)
    with pytest.raises(ValueError, match="sequences"):
        K.causal_conv1d_fwd(z(8, 16), z(4, 16), z(16), z(8, 16), 3)
