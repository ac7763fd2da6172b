"""CPU restatement of the RoBERTa masked LM (test infrastructure only).

HF `RobertaForMaskedLM` (tf:models/roberta/modeling_roberta.py) in the build's parameter layout
(config.param_shapes, arch "roberta"), in plain torch ops under `torch.autocast("cpu", bf16)` or
in fp32: position ids counted over the non-pad ids, word + type + position embeddings with
padding_idx rows, LayerNorm, the post-LN layers (`LayerNorm(dropout(dense(x)) + input)` twice),
the MLM head (dense, GELU, LayerNorm, the decoder tied to the word embedding plus its bias) over
the first `vocab_valid` rows, and the cross entropy with ignore_index -100 and no label shift.
Pinned against the live HF module by tests/test_roberta_cpu.py.  With `drop` (a
tests/test_dropout_gpu.py `Masks`) the engine's own hidden-dropout masks are applied at HF's
sites; attention-probability dropout enters through a patched
torch.nn.functional.scaled_dot_product_attention (tests/test_attn_dropout_gpu.py MaskedSDPA).
"""

import contextlib
import statistics

import numpy as np
import torch
import torch.nn.functional as F

BF16 = torch.bfloat16


def init_params(cfg, seed: int = 0, std: float = 0.02) -> dict[str, torch.Tensor]:
    """N(0, std) matrices, embeddings and (non-zero) biases, unit LayerNorm gains; the
    padding_idx rows of the word and position tables zero (RobertaPreTrainedModel._init_weights),
    the vocabulary pad rows and their decoder-bias entries zero."""
    from multimodal_llm_pretraining_amd import config as C

    g = torch.Generator().manual_seed(seed)
    t = cfg.text
    out = {}
    for name, shape in C.param_shapes(cfg).items():
        if name.endswith(("ln1.weight", "ln2.weight", "embed_ln.weight", "mlm.ln.weight")):
            out[name] = torch.ones(shape)
        else:
            out[name] = torch.randn(shape, generator=g) * std
    out["text.embed"][t.pad_id] = 0
    out["text.pos_embed"][t.pad_id] = 0
    out["text.embed"][t.n_vocab:] = 0
    out["text.mlm.bias"][t.n_vocab:] = 0
    return out


def make_batch(cfg, batch: int, seq: int, seed: int = 1) -> dict[str, torch.Tensor]:
    """DummyTextModelingDataset's distribution: ids U{0..V-1}, every position labelled."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, cfg.text.n_vocab, (batch, seq), generator=g)
    return {"input_ids": ids, "labels": ids.clone(), "attention_mask": torch.ones_like(ids)}


def position_ids(ids: torch.Tensor, pad_id: int) -> torch.Tensor:
    """RobertaEmbeddings.create_position_ids_from_input_ids."""
    mask = ids.ne(pad_id).int()
    return (torch.cumsum(mask, dim=1).type_as(mask) * mask).long() + pad_id


def encoder(P, t, ids, pos, drop=None, total_rows=None, rows=None):
    """Embeddings + layers over ids [B, S]; returns the last LayerNorm's output (fp32)."""
    B, S = ids.shape
    h_, H = t.hidden, t.heads
    D = h_ // H
    T = B * S if total_rows is None else total_rows
    ph = t.hidden_dropout
    dr = (lambda x, unit, k: x) if drop is None else \
        (lambda x, unit, k: drop(x, ph, unit, k, T, rows))
    e = F.embedding(ids, P["text.embed"], padding_idx=t.pad_id) + P["text.type_embed"][0]
    e = e + F.embedding(pos, P["text.pos_embed"], padding_idx=t.pad_id)
    h = F.layer_norm(e, (h_,), P["text.embed_ln.weight"], P["text.embed_ln.bias"], t.eps)
    h = dr(h, 0, 0)
    for i in range(t.layers):
        p = f"text.layers.{i}."
        # query | key | value as HF's three Linears: under autocast each returns its own bf16
        # input gradient and autograd adds the three in bf16
        W, bq = P[p + "qkv.weight"], P[p + "qkv.bias"]
        q, k, v = (F.linear(h, W[j * h_:(j + 1) * h_], bq[j * h_:(j + 1) * h_])
                   .reshape(B, S, H, D).transpose(1, 2) for j in range(3))
        a = F.scaled_dot_product_attention(q, k, v, is_causal=False, scale=D ** -0.5)
        a = a.transpose(1, 2).reshape(B, S, h_)
        ao = dr(F.linear(a, P[p + "dense.weight"], P[p + "dense.bias"]), 1 + i, 0)
        h = F.layer_norm(ao + h, (h_,), P[p + "ln1.weight"], P[p + "ln1.bias"], t.eps)
        m = F.linear(F.gelu(F.linear(h, P[p + "fc1.weight"], P[p + "fc1.bias"])),
                     P[p + "fc2.weight"], P[p + "fc2.bias"])
        h = F.layer_norm(dr(m, 1 + i, 1) + h, (h_,), P[p + "ln2.weight"], P[p + "ln2.bias"], t.eps)
    return h


def head_loss_sum(P, t, h, labels, reduction="sum"):
    """RobertaLMHead + the CE over the labelled positions (fp32 upcast, ignore_index -100)."""
    x = F.gelu(F.linear(h, P["text.mlm.dense.weight"], P["text.mlm.dense.bias"]))
    x = F.layer_norm(x, (t.hidden,), P["text.mlm.ln.weight"], P["text.mlm.ln.bias"], t.eps)
    V = t.n_vocab
    logits = F.linear(x, P["text.embed"][:V], P["text.mlm.bias"][:V])
    return F.cross_entropy(logits.float().view(-1, V), labels.reshape(-1), ignore_index=-100,
                           reduction=reduction)


def forward_loss(P, cfg, batch, precision: str = "bf16", drop=None, num_items=None, lens=None):
    """Mean CE over the labelled tokens (num_items: another denominator).  lens: a right-padded
    batch run sequence by sequence over its valid tokens — the packed rows the engine computes
    over; the position ids come from the padded ids, as HF computes them."""
    t = cfg.text
    ids, labels = batch["input_ids"], batch["labels"]
    pos = position_ids(ids, t.pad_id)
    ctx = torch.autocast("cpu", dtype=BF16) if precision == "bf16" else contextlib.nullcontext()
    with ctx:
        if lens is None:
            h = encoder(P, t, ids, pos, drop)
            if num_items is None:  # HF's own call: CrossEntropyLoss(), the mean inside the op
                return head_loss_sum(P, t, h, labels, "mean")
            total = head_loss_sum(P, t, h, labels)
            n = int((labels != -100).sum())
        else:
            T, cu = sum(lens), np.concatenate(([0], np.cumsum(lens)))
            total, n = 0.0, 0
            for b, ln in enumerate(lens):
                rows = slice(int(cu[b]), int(cu[b + 1]))
                h = encoder(P, t, ids[b:b + 1, :ln], pos[b:b + 1, :ln], drop, T, rows)
                total = total + head_loss_sum(P, t, h, labels[b:b + 1, :ln])
                n += int((labels[b, :ln] != -100).sum())
    return total / (max(1, n) if num_items is None else num_items)


def loss_and_grads(P, cfg, batch, precision="bf16", drop=None, lens=None):
    Pr = {k: v.clone().requires_grad_() for k, v in P.items()}
    loss = forward_loss(Pr, cfg, batch, precision, drop, lens=lens)
    loss.backward()
    return loss.item(), {k: (v.grad if v.grad is not None else torch.zeros_like(v))
                         for k, v in Pr.items()}


def bf16_sigma(P, cfg, batch_size: int, seq: int, seeds=range(100, 108)) -> float:
    """Standard deviation of (bf16 oracle − fp32 oracle) over batch seeds at this shape: the
    distance two valid bf16 implementations keep from fp32, each on its own side."""
    d = []
    with torch.no_grad():
        for s in seeds:
            b = make_batch(cfg, batch_size, seq, seed=s)
            d.append(forward_loss(P, cfg, b, "bf16").item() - forward_loss(P, cfg, b, "fp32").item())
    return statistics.pstdev(d)


def train_steps(P, cfg, batches, lrs, precision="bf16", betas=(0.9, 0.98), eps=1e-8,
                weight_decay=0.0):
    """torch.optim.Adam steps, one per batch (the recipe's optimizer; HF Trainer's effective
    weight decay is 0); returns the per-step losses and the final parameters."""
    params = {k: v.clone().requires_grad_() for k, v in P.items()}
    o = torch.optim.Adam(list(params.values()), lr=lrs[0], betas=betas, eps=eps,
                         weight_decay=weight_decay, foreach=False)
    losses = []
    for i, b in enumerate(batches):
        for gr in o.param_groups:
            gr["lr"] = lrs[i]
        loss = forward_loss(params, cfg, b, precision)
        loss.backward()
        for v in params.values():
            if v.grad is None:
                v.grad = torch.zeros_like(v)
        o.step()
        o.zero_grad(set_to_none=True)
        losses.append(loss.item())
    return losses, {k: v.detach() for k, v in params.items()}


# ---- HF names (transformers 5.15 RobertaForMaskedLM) ----------------------------------------
_LAYER = (("attention.output.dense", "dense"), ("attention.output.LayerNorm", "ln1"),
          ("intermediate.dense", "fc1"), ("output.dense", "fc2"), ("output.LayerNorm", "ln2"))
_TOP = (("roberta.embeddings.word_embeddings.weight", "text.embed"),
        ("roberta.embeddings.position_embeddings.weight", "text.pos_embed"),
        ("roberta.embeddings.token_type_embeddings.weight", "text.type_embed"),
        ("roberta.embeddings.LayerNorm.weight", "text.embed_ln.weight"),
        ("roberta.embeddings.LayerNorm.bias", "text.embed_ln.bias"),
        ("lm_head.dense.weight", "text.mlm.dense.weight"),
        ("lm_head.dense.bias", "text.mlm.dense.bias"),
        ("lm_head.layer_norm.weight", "text.mlm.ln.weight"),
        ("lm_head.layer_norm.bias", "text.mlm.ln.bias"),
        ("lm_head.bias", "text.mlm.bias"))


def to_hf(P, cfg, hf_sd) -> dict[str, torch.Tensor]:
    """The build layout as a RobertaForMaskedLM state dict: query | key | value split, the
    vocabulary pad rows dropped, the decoder's tied aliases filled in."""
    t = cfg.text
    V, h = t.n_vocab, t.hidden
    out = {}
    for hf, mine in _TOP:
        x = P[mine]
        out[hf] = (x[:V] if mine in ("text.embed", "text.mlm.bias") else x).clone()
    out["lm_head.decoder.weight"] = out["roberta.embeddings.word_embeddings.weight"]
    out["lm_head.decoder.bias"] = out["lm_head.bias"]
    for i in range(t.layers):
        p, q = f"roberta.encoder.layer.{i}.", f"text.layers.{i}."
        for j, n in enumerate(("query", "key", "value")):
            out[p + f"attention.self.{n}.weight"] = P[q + "qkv.weight"][j * h:(j + 1) * h].clone()
            out[p + f"attention.self.{n}.bias"] = P[q + "qkv.bias"][j * h:(j + 1) * h].clone()
        for hf, mine in _LAYER:
            for s in ("weight", "bias"):
                out[p + f"{hf}.{s}"] = P[q + f"{mine}.{s}"].clone()
    assert set(out) == set(hf_sd), set(out) ^ set(hf_sd)
    return out


def from_hf(sd, cfg) -> dict[str, torch.Tensor]:
    """Inverse of to_hf over named parameters (weights or gradients): the build layout, the pad
    rows zero."""
    from multimodal_llm_pretraining_amd import config as C

    t = cfg.text
    V = t.n_vocab
    out = {n: torch.zeros(s) for n, s in C.param_shapes(cfg).items()}
    for hf, mine in _TOP:
        if mine in ("text.embed", "text.mlm.bias"):
            out[mine][:V] = sd[hf]
        else:
            out[mine] = sd[hf].clone()
    for i in range(t.layers):
        p, q = f"roberta.encoder.layer.{i}.", f"text.layers.{i}."
        for s in ("weight", "bias"):
            out[q + f"qkv.{s}"] = torch.cat([sd[p + f"attention.self.{n}.{s}"]
                                             for n in ("query", "key", "value")], 0)
            for hf, mine in _LAYER:
                out[q + f"{mine}.{s}"] = sd[p + f"{hf}.{s}"].clone()
    return out
