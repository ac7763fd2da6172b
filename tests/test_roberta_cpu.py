"""The RoBERTa masked LM off the GPU: the CPU oracle of tests/roberta_oracle.py against live
`RobertaForMaskedLM` (loss and every parameter gradient, fp32 and bf16 autocast, on a batch with
pad ids inside the sequences), the `roberta` / `roberta-bf16` recipes against the reference's
constants (src/models/roberta.py:14-70), the parameter layout against HF's count, the FLOP
formula, the masked-LM Batch on the host (no label shift, HF's position ids, right padding), the
sharding refusals and the K20 entry points' declarations."""

import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roberta_oracle as RO  # noqa: E402

from multimodal_llm_pretraining_amd import config as C  # noqa: E402


def pad_batch(cfg, B=4, S=64, seed=1):
    """256 tokens with the pad id (1) at position 0 of a row, mid-row, and twice in a row — at
    V = 515 a random draw does not guarantee any of them."""
    b = RO.make_batch(cfg, B, S, seed=seed)
    ids = b["input_ids"]
    ids[ids == 1] = 7
    ids[0, 0] = 1
    ids[1, 20] = 1
    ids[2, 30] = ids[2, 31] = 1
    b["labels"] = ids.clone()
    return b


# ------------------------------------------------------------------ oracle vs HF
@pytest.fixture(scope="module")
def hf():
    from multimodal_llm_pretraining_amd.models import build_hf_model

    torch.manual_seed(0)
    cfg = C.get_config("tiny-roberta")
    P = RO.init_params(cfg, seed=0)
    m = build_hf_model(cfg).eval()
    m.config._attn_implementation = "sdpa"
    m.load_state_dict(RO.to_hf(P, cfg, m.state_dict()))
    return cfg, P, m


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_oracle_matches_hf(hf, precision):
    import contextlib

    cfg, P, m = hf
    batch = pad_batch(cfg)
    pos = RO.position_ids(batch["input_ids"], 1)
    assert pos[0, 0] == 1 and pos[0, 1] == 2 and pos[1, 20] == 1 and pos[1, 21] == 22
    assert pos[2, 29] == 31 and pos[2, 30] == 1 and pos[2, 31] == 1 and pos[2, 32] == 32
    assert int(pos.max()) == 64 + 1
    ctx = (lambda: torch.autocast("cpu", dtype=torch.bfloat16)) if precision == "bf16" else \
        contextlib.nullcontext
    m.zero_grad()
    with ctx():
        out = m(**batch)
    out.loss.backward()
    loss, G = RO.loss_and_grads(P, cfg, batch, precision)
    # the bars of test_vit_cls_cpu.py's oracle: the same ops in the same order leave only the
    # association of a few fp32 sums free (2e-6 on a loss of ~6.2, 1e-5 of a tensor's norm)
    assert abs(loss - out.loss.item()) < 2e-6, (loss, out.loss.item())
    assert all(p.grad is not None for p in m.parameters())
    hf_g = RO.from_hf({n: p.grad for n, p in m.named_parameters()}, cfg)
    assert set(hf_g) == set(G)
    for n, ref in hf_g.items():
        err = ((G[n] - ref).norm() / (ref.norm() + 1e-6)).item()
        assert err < 1e-5, (n, err)
    # padding_idx: position row 1 and the rows past S + 1 take no gradient at all
    gp = G["text.pos_embed"]
    assert torch.count_nonzero(gp[1]) == 0 and torch.count_nonzero(gp[66:]) == 0
    assert torch.count_nonzero(gp[0]) == 0 and torch.count_nonzero(gp[2]) > 0
    assert torch.count_nonzero(hf_g["text.pos_embed"][1]) == 0
    assert torch.count_nonzero(G["text.embed"][515:]) == 0
    assert torch.count_nonzero(G["text.mlm.bias"][515:]) == 0


def test_pad_row_of_the_word_table_gets_the_decoder_gradient_only(hf):
    cfg, P, _ = hf
    t = cfg.text
    batch = pad_batch(cfg)
    ids, labels = batch["input_ids"], batch["labels"]
    Pa = {k: v.clone().requires_grad_() for k, v in P.items()}
    dec = P["text.embed"].clone().requires_grad_()
    h = RO.encoder(Pa, t, ids, RO.position_ids(ids, 1))
    loss = RO.head_loss_sum({**Pa, "text.embed": dec}, t, h, labels) / labels.numel()
    loss.backward()
    _, G = RO.loss_and_grads(P, cfg, batch, "fp32")
    assert torch.count_nonzero(Pa["text.embed"].grad[1]) == 0  # nothing from the gather
    assert torch.count_nonzero(dec.grad[1]) > 0
    assert torch.equal(G["text.embed"][1], dec.grad[1])
    assert torch.count_nonzero(Pa["text.embed"].grad[int(ids[0, 1])]) > 0  # (any other id does)


def test_mapping_round_trips(hf):
    cfg, P, m = hf
    back = RO.from_hf(dict(m.named_parameters()), cfg)
    assert all(torch.equal(back[n], P[n]) for n in P)


# ------------------------------------------------------------------ recipe
def test_roberta_recipe_is_the_reference():
    from multimodal_llm_pretraining_amd import models as M
    from multimodal_llm_pretraining_amd.data import DummyTextModelingDataset

    mc = M.get_model_class("roberta")
    assert mc.batch_size == 8192 and mc.training_steps == 500000
    assert mc.mixed_precision == "fp16"
    assert mc.optimizer is torch.optim.Adam
    assert mc.optimizer_kwargs == {"lr": 4e-4, "betas": (0.9, 0.98), "weight_decay": 0.01}
    assert mc.scheduler_type == "linear" and mc.scheduler_kwargs == {"num_warmup_steps": 30_000}
    assert mc.max_grad_norm == 0.0 and mc.hf_training_args == {}
    assert mc.fsdp_layers_to_wrap == ["RobertaLayer"]
    assert mc.vocab_size == 50265 and mc.sequence_length == 512
    cfg = mc.model_config
    t = cfg.text
    assert cfg == C.get_config("roberta-large") and cfg.vision is None
    assert (t.arch, t.hidden, t.layers, t.heads, t.ffn) == ("roberta", 1024, 24, 16, 4096)
    assert (t.vocab, t.n_vocab, t.max_positions, t.pad_id, t.type_vocab) == (50272, 50265, 514, 1, 1)
    assert t.eps == 1e-5 and t.rot_dims == 0 and t.tie_embeddings and t.head_dim == 64
    assert t.hidden_dropout == 0.1 and t.attn_dropout == 0.1
    bf = M.get_model_class("roberta-bf16")
    assert bf.mixed_precision == "bf16" and bf.model_config == cfg
    for prop in ("batch_size", "training_steps", "optimizer", "optimizer_kwargs", "scheduler_type",
                 "scheduler_kwargs", "max_grad_norm", "fsdp_layers_to_wrap", "vocab_size",
                 "sequence_length", "hf_training_args"):
        assert getattr(bf, prop) == getattr(mc, prop), prop
    assert "roberta" not in M.OUT_OF_SCOPE and "roberta-bf16" not in M.OUT_OF_SCOPE
    assert set(M.RobertaT.__args__) == {"roberta", "roberta-bf16"}
    ds = mc.load_dummy_dataset()
    assert isinstance(ds, DummyTextModelingDataset) and len(ds) == 50_000
    assert ds[0]["input_ids"].shape == (512,)


def test_fp16_recipe_is_refused():
    from multimodal_llm_pretraining_amd.experiments import TrainingConfig

    with pytest.raises(NotImplementedError, match="bf16"):
        TrainingConfig(1, 8, "mi355x", "roberta").training_class().build_trainer(None, None)
    tc = TrainingConfig(1, 8, "mi355x", "roberta-bf16").training_class()
    assert tc.bf16 and not tc.fp16 and not tc.max_grad_norm


def test_hf_branch_is_roberta_for_masked_lm():
    from transformers import RobertaForMaskedLM

    from multimodal_llm_pretraining_amd.models import build_hf_model

    with torch.device("meta"):
        m = build_hf_model(C.get_config("roberta-large"))
    assert isinstance(m, RobertaForMaskedLM)
    c = m.config
    assert (c.vocab_size, c.hidden_size, c.num_hidden_layers, c.num_attention_heads,
            c.intermediate_size, c.max_position_embeddings, c.type_vocab_size, c.pad_token_id) == \
        (50265, 1024, 24, 16, 4096, 514, 1, 1)
    assert c.hidden_dropout_prob == 0.1 and c.attention_probs_dropout_prob == 0.1
    assert c.layer_norm_eps == 1e-5 and c.hidden_act == "gelu"
    # HF's count (the decoder and its bias are tied aliases) + 7 pad rows and 7 pad biases
    hf_n = sum(p.numel() for p in m.parameters())
    assert C.num_params(C.get_config("roberta-large")) - 7 * 1024 - 7 == hf_n


# ------------------------------------------------------------------ layout, flops, validation
def test_param_shapes():
    s = C.param_shapes(C.get_config("tiny-roberta"))
    assert s["text.embed"] == (520, 128) and s["text.pos_embed"] == (66, 128)
    assert s["text.type_embed"] == (1, 128) and s["text.mlm.bias"] == (520,)
    assert s["text.layers.1.qkv.weight"] == (384, 128) and s["text.layers.0.fc1.weight"] == (256, 128)
    per_layer = {n.split(".", 3)[3] for n in s if n.startswith("text.layers.0.")}
    assert per_layer == {f"{m}.{w}" for m in ("qkv", "dense", "ln1", "fc1", "fc2", "ln2")
                         for w in ("weight", "bias")}
    assert {n for n in s if not n.startswith("text.layers.")} == {
        "text.embed", "text.pos_embed", "text.type_embed", "text.embed_ln.weight",
        "text.embed_ln.bias", "text.mlm.dense.weight", "text.mlm.dense.bias", "text.mlm.ln.weight",
        "text.mlm.ln.bias", "text.mlm.bias"}
    assert "text.lm_head" not in s and "text.final_ln.weight" not in s


def test_fp32_read_region_and_init():
    from multimodal_llm_pretraining_amd.params import ParamStore, init_normal, is_fp32_read

    cfg = C.get_config("tiny-roberta")
    for n in ("text.embed", "text.pos_embed", "text.type_embed", "text.embed_ln.weight",
              "text.layers.0.ln1.bias", "text.layers.1.ln2.weight", "text.mlm.ln.bias"):
        assert is_fp32_read(n), n
    for n in ("text.mlm.bias", "text.mlm.dense.weight", "text.layers.0.qkv.bias"):
        assert not is_fp32_read(n), n
    store = ParamStore(C.param_shapes(cfg), "cpu")
    store.refresh_shadow = lambda: None  # (the cast kernel needs the GPU)
    init_normal(store, 3, cfg=cfg)
    assert torch.count_nonzero(store.p("text.embed")[1]) == 0
    assert torch.count_nonzero(store.p("text.pos_embed")[1]) == 0
    assert torch.count_nonzero(store.p("text.embed")[515:]) == 0
    assert torch.count_nonzero(store.p("text.mlm.bias")[515:]) == 0
    assert torch.count_nonzero(store.p("text.embed")[2]) > 0
    assert torch.count_nonzero(store.p("text.mlm.bias")[:515]) > 0
    for n in ("text.embed_ln.weight", "text.mlm.ln.weight", "text.layers.0.ln1.weight",
              "text.layers.1.ln2.weight"):
        assert torch.all(store.p(n) == 1), n


def test_flops():
    from multimodal_llm_pretraining_amd.benchmarking import count_flops_per_example
    from multimodal_llm_pretraining_amd.models import get_model_class

    cfg = C.get_config("tiny-roberta")
    S, h, F_, V, L = 48, 128, 256, 515, 2
    want = 3.0 * (L * (2 * S * h * (4 * h + 2 * F_) + 4 * S * S * h) + 2 * S * h * h + 2 * S * h * V)
    assert C.flops_per_sample(cfg, S) == want
    assert C.executed_flops_per_sample(cfg, S) == want
    big = C.get_config("roberta-large")
    S, h, F_, V, L = 512, 1024, 4096, 50265, 24
    want = 3.0 * (L * (2 * S * h * (4 * h + 2 * F_) + 4 * S * S * h) + 2 * S * h * h + 2 * S * h * V)
    assert count_flops_per_example(get_model_class("roberta-bf16")) == want
    assert C.executed_flops_per_sample(big, 512) == want


def test_config_validation():
    base = C.get_config("tiny-roberta").text
    assert C.get_config("tiny-roberta-drop").text == \
        C.with_dropout(C.get_config("tiny-roberta"), text=0.1, text_attention=0.1).text
    for kw in (dict(hidden_dropout=1.0), dict(attn_dropout=-0.1), dict(type_vocab=2),
               dict(rotary_pct=0.25), dict(tie_embeddings=False), dict(max_positions=3),
               dict(pad_id=515)):
        with pytest.raises(ValueError):
            C.replace(base, **kw)
    base.check_seq(64)
    with pytest.raises(ValueError, match="max_positions"):
        base.check_seq(65)
    C.get_config("roberta-large").text.check_seq(512)
    with pytest.raises(ValueError):
        C.get_config("roberta-large").text.check_seq(513)
    C.get_config("tiny-lm").text.check_seq(10 ** 6)  # other architectures: no position table


# ------------------------------------------------------------------ Batch on the host
def test_batch_on_the_host():
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg = C.get_config("tiny-roberta")
    bd = pad_batch(cfg, 4, 48)
    ids, labels = bd["input_ids"], bd["labels"].clone()
    b = Batch(cfg, ids, labels, None, "cpu")
    assert (b.B, b.S, b.T, b.num_items) == (4, 48, 192, 192)
    assert torch.equal(b.labels, labels.reshape(-1))  # no shift
    assert b.loss_rows is None and b.cu_seqlens is None
    assert b.pos_ids.dtype == torch.int64
    assert torch.equal(b.pos_ids, RO.position_ids(ids, 1).reshape(-1))
    # the segments of both tables leave the padding_idx rows out
    seg_id, seg_off, perm = b.segments
    assert 1 not in seg_id.tolist() and perm.numel() == int((ids != 1).sum())
    pid, poff, pperm = b.pos_segments
    assert 1 not in pid.tolist() and pperm.numel() == int((ids != 1).sum())
    assert pid.tolist() == sorted(set(b.pos_ids.tolist()) - {1})
    # 15% labelled, one row without any label: the loss rows are the labelled positions
    g = torch.Generator().manual_seed(5)
    mlm = labels.clone()
    mlm[torch.rand(mlm.shape, generator=g) >= 0.15] = -100
    mlm[3] = -100
    b = Batch(cfg, ids, mlm, None, "cpu")
    keep = (mlm != -100).reshape(-1)
    assert b.num_items == int(keep.sum()) and 0 < b.num_items < 0.3 * 192
    assert torch.equal(b.loss_rows.long(), torch.nonzero(keep).view(-1))
    assert torch.equal(b.loss_labels, mlm.reshape(-1)[keep])
    assert torch.equal(b.loss_map >= 0, keep)
    # right padding: the pads are dropped, the valid tokens keep HF's positions
    lens = (48, 17, 1, 33)
    mask = torch.zeros_like(ids)
    for r, n in enumerate(lens):
        mask[r, :n] = 1
    b = Batch(cfg, ids, labels, None, "cpu", attention_mask=mask)
    sel = mask.bool().reshape(-1)
    assert b.T == sum(lens) and b.lens == list(lens) and b.num_items == sum(lens)
    assert torch.equal(b.pos_ids, RO.position_ids(ids, 1).reshape(-1)[sel])
    assert torch.equal(b.labels, labels.reshape(-1)[sel])
    assert b.cu_seqlens.tolist() == [0, 48, 65, 66, 99]
    with pytest.raises(ValueError, match="max_positions"):
        Batch(cfg, torch.zeros(2, 65, dtype=torch.int64), torch.zeros(2, 65, dtype=torch.int64),
              None, "cpu")
    with pytest.raises(ValueError, match=r"\[0, 515\)"):
        Batch(cfg, ids, torch.full_like(ids, 515), None, "cpu")


# ------------------------------------------------------------------ sharding refusal
@pytest.mark.parametrize("sharding", ["zero_2", "zero_3", "fsdp_shard_grad_op", "fsdp_full_shard"])
def test_unit_sharding_is_refused(sharding):
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    with pytest.raises(NotImplementedError, match="roberta") as e:
        ManualTrainer(StepConfig(model="tiny-roberta", sharding=sharding), AdamConfig(), "meta")
    assert sharding in str(e.value)


def test_cli_lists_and_counts(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import benchmark

    names = benchmark.model_types()
    assert "roberta" in names and "roberta-bf16" in names
    benchmark.main(["--num-nodes", "1", "--gpus-per-node", "8", "--gpu-type", "mi355x",
                    "--model", "roberta-bf16", "--methods", "all", "--cmd", "count"])
    assert "cached experiments: 0 /" in capsys.readouterr().out


# ------------------------------------------------------------------ header / binding / wrappers
C_TYPES = {"int64_t": "I64", "double": "F64", "uint64_t": "U64", "float": "F32", "void*": "P",
           "constvoid*": "P", "constfloat*": "P", "float*": "P", "constint64_t*": "P"}
K20 = {
    "mmpt_add_layernorm_fwd": "rows h eps resid v ld_v w b s y32 y16 ld_y16 mean rstd p seed site "
                              "stream",
    "mmpt_add_layernorm_bwd_workspace_bytes": "rows h",
    "mmpt_add_layernorm_bwd": "rows h s mean rstd w dy32 dyb ld_dyb ds32 dvb ld_dvb dw db dsum "
                              "dsum2 p seed site workspace stream",
    "mmpt_roberta_embed_fwd": "rows h eps ids pos word vocab pos_table max_pos type_row w b h32 h16 "
                              "mean rstd p seed site stream",
    "mmpt_roberta_embed_bwd_workspace_bytes": "rows h",
    "mmpt_roberta_embed_bwd": "rows h ids pos word vocab pos_table max_pos type_row mean rstd w dh "
                              "dhb de dw db dtype p seed site workspace stream",
    "mmpt_mlm_ln_fwd": "rows h eps g ld_g w b n16 ld_n16 mean rstd stream",
    "mmpt_mlm_ln_bwd_workspace_bytes": "rows h",
    "mmpt_mlm_ln_bwd": "rows h g ld_g mean rstd w dn16 ld_dn16 pre ld_pre dpre ld_dpre dw db dsum "
                       "workspace stream",
}


def test_k20_header_binding_and_wrappers_agree():
    from multimodal_llm_pretraining_amd import _lib, kernels

    src = open(os.path.join(ROOT, "include", "mmpt.h")).read()
    assert re.search(r"#define MMPT_ABI_VERSION (\d+)", src).group(1) == "16"
    assert _lib.ABI_VERSION == 16
    assert "K20" in src
    for name, params in K20.items():
        m = re.search(r"\b(int|int64_t) " + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        args = [a.strip() for a in " ".join(m.group(2).split()).split(",")]
        names = [re.split(r"[ *]", a)[-1] for a in args]
        assert names == params.split(), (name, names)
        types = [C_TYPES["".join(a.rsplit(n, 1)[0].split())] for a, n in zip(args, names)]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is (_lib.I64 if name.endswith("workspace_bytes") else _lib.I32)
        assert argtypes == [getattr(_lib, t) for t in types], (name, types)
        if not name.endswith("workspace_bytes"):
            assert callable(getattr(kernels, name[len("mmpt_"):])), name
    # the library itself exports them (when it has been built)
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert all(hasattr(lib, n) for n in K20)
