"""CPU restatement of the vision-only classifier (test infrastructure only).

HF `ViTForImageClassification` (tf:models/vit/modeling_vit.py) in the build's parameter
layout: `oracle.model.vision_forward` with every layer used (feature_layer = -1), then
vit.layernorm, the CLS row, the classifier over the first `num_classes` rows of the padded
head and `F.cross_entropy(logits.float(), labels)` — under `torch.autocast("cpu", bf16)` or in
fp32.  Pinned against the live HF module by tests/test_vit_cls_cpu.py.  With `drop` (a
tests/test_dropout_gpu.py `Masks`) the encoder is `masked_vision_forward`: the engine's own
dropout masks at HF's three sites.
"""

import statistics

import torch
import torch.nn.functional as F

from oracle import model as O

BF16 = torch.bfloat16


def vision_cfg(cfg) -> O.VisionCfg:
    v = cfg.vision
    assert v.feature_layer == -1 and v.used_layers == v.layers
    return O.VisionCfg(hidden=v.hidden, layers=v.layers, heads=v.heads, ffn=v.ffn, image=v.image,
                       patch=v.patch, eps=v.eps, feature_layer=-1, act=v.act, pre_ln=v.pre_ln,
                       patch_bias=v.patch_bias)


def init_params(cfg, seed: int = 0, std: float = 0.02) -> dict[str, torch.Tensor]:
    """oracle.model.init_params' convention over config.param_shapes(cfg): N(0, std) matrices
    and (non-zero) biases, unit LayerNorm gains, zero im2col pad columns and class pad rows."""
    from multimodal_llm_pretraining_amd import config as C

    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in C.param_shapes(cfg).items():
        if name.endswith(("ln1.weight", "ln2.weight", "ln_post.weight")):
            out[name] = torch.ones(shape)
        else:
            out[name] = torch.randn(shape, generator=g) * std
    v = cfg.vision
    out["vision.patch.weight"][:, v.channels * v.patch ** 2:] = 0
    out["cls_head.weight"][cfg.num_classes:] = 0
    out["cls_head.bias"][cfg.num_classes:] = 0
    return out


def make_batch(cfg, batch: int, seed: int = 1) -> dict[str, torch.Tensor]:
    """DummyImageClassificationDataset's distributions: pixels U[0, 1), labels U{0..C-1}."""
    g = torch.Generator().manual_seed(seed)
    v = cfg.vision
    return {"pixel_values": torch.rand(batch, v.channels, v.image, v.image, generator=g),
            "labels": torch.randint(0, cfg.num_classes, (batch,), generator=g)}


def forward_loss(P, cfg, batch, precision: str = "bf16", drop=None, num_items=None):
    """Mean CE over the batch's images (num_items: another denominator — the global batch)."""
    v = vision_cfg(cfg)
    ctx = torch.autocast("cpu", dtype=BF16) if precision == "bf16" else O._null()
    with ctx:
        if drop is None:
            h = O.vision_forward(P, v, batch["pixel_values"])
        else:
            from test_dropout_gpu import masked_vision_forward

            h = masked_vision_forward(P, v, batch["pixel_values"], cfg.vision.hidden_dropout, drop)
        s = F.layer_norm(h, (v.hidden,), P["vision.ln_post.weight"], P["vision.ln_post.bias"], v.eps)
        C = cfg.num_classes
        logits = F.linear(s[:, 0, :], P["cls_head.weight"][:C], P["cls_head.bias"][:C])
    if num_items is None:
        return F.cross_entropy(logits.float(), batch["labels"])
    return F.cross_entropy(logits.float(), batch["labels"], reduction="sum") / num_items


def loss_and_grads(P, cfg, batch, precision="bf16", drop=None):
    Pr = {k: t.clone().requires_grad_() for k, t in P.items()}
    loss = forward_loss(Pr, cfg, batch, precision, drop)
    loss.backward()
    return loss.item(), {k: (t.grad if t.grad is not None else torch.zeros_like(t))
                         for k, t in Pr.items()}


def bf16_sigma(P, cfg, batch_size: int, seeds=range(100, 108)) -> float:
    """Standard deviation of (bf16 oracle − fp32 oracle) over batch seeds at this shape: the
    distance two valid bf16 implementations keep from fp32, each on its own side."""
    d = []
    with torch.no_grad():
        for s in seeds:
            b = make_batch(cfg, batch_size, seed=s)
            d.append(forward_loss(P, cfg, b, "bf16").item() - forward_loss(P, cfg, b, "fp32").item())
    return statistics.pstdev(d) if len(d) > 1 else abs(d[0])


def linear_lrs(lr: float, warmup: int, total: int, steps: int) -> list[float]:
    """transformers get_linear_schedule_with_warmup: lr at optimizer steps 0 .. steps-1."""
    out = []
    for i in range(steps):
        f = i / max(1, warmup) if i < warmup else max(0.0, (total - i) / max(1, total - warmup))
        out.append(lr * f)
    return out


def train_steps(P, cfg, batches, lrs, precision="bf16", betas=(0.9, 0.999), eps=1e-8,
                weight_decay=0.03, max_grad_norm=1.0):
    """The reference recipe's step (src/models/vit.py: torch.optim.Adam with weight decay —
    L2 added to the gradient — and clipping at 1.0), one optimizer step per batch."""
    params = {k: t.clone().requires_grad_() for k, t in P.items()}
    o = torch.optim.Adam(list(params.values()), lr=lrs[0], betas=betas, eps=eps,
                         weight_decay=weight_decay, foreach=False)
    losses = []
    for i, b in enumerate(batches):
        for gr in o.param_groups:
            gr["lr"] = lrs[i]
        loss = forward_loss(params, cfg, b, precision)
        loss.backward()
        for t in params.values():  # (a pad-free parameter never lacks a gradient; be explicit)
            if t.grad is None:
                t.grad = torch.zeros_like(t)
        if max_grad_norm > 0:
            torch.nn.utils.clip_grad_norm_(list(params.values()), max_grad_norm)
        o.step()
        o.zero_grad(set_to_none=True)
        losses.append(loss.item())
    return losses, {k: t.detach() for k, t in params.items()}


# ---- HF names (transformers 5.15 ViTForImageClassification) -------------------------------
def to_hf(P, cfg, hf_sd) -> dict[str, torch.Tensor]:
    """The build layout as a ViTForImageClassification state dict (shapes from hf_sd): the
    stacked qkv split, the im2col pad columns and the class pad rows dropped."""
    v = cfg.vision
    out = {}
    w = hf_sd["vit.embeddings.patch_embeddings.projection.weight"]
    out["vit.embeddings.patch_embeddings.projection.weight"] = \
        P["vision.patch.weight"][:, :w[0].numel()].reshape(w.shape).clone()
    out["vit.embeddings.patch_embeddings.projection.bias"] = P["vision.patch.bias"].clone()
    out["vit.embeddings.cls_token"] = P["vision.cls"].view(1, 1, -1).clone()
    out["vit.embeddings.position_embeddings"] = P["vision.pos"].unsqueeze(0).clone()
    h = v.hidden
    for i in range(v.layers):
        p, q = f"vit.layers.{i}.", f"vision.layers.{i}."
        out[p + "layernorm_before.weight"] = P[q + "ln1.weight"].clone()
        out[p + "layernorm_before.bias"] = P[q + "ln1.bias"].clone()
        for j, n in enumerate("qkv"):
            out[p + f"attention.{n}_proj.weight"] = P[q + "qkv.weight"][j * h:(j + 1) * h].clone()
            out[p + f"attention.{n}_proj.bias"] = P[q + "qkv.bias"][j * h:(j + 1) * h].clone()
        out[p + "attention.o_proj.weight"] = P[q + "o.weight"].clone()
        out[p + "attention.o_proj.bias"] = P[q + "o.bias"].clone()
        out[p + "layernorm_after.weight"] = P[q + "ln2.weight"].clone()
        out[p + "layernorm_after.bias"] = P[q + "ln2.bias"].clone()
        for n in ("fc1", "fc2"):
            out[p + f"mlp.{n}.weight"] = P[q + f"{n}.weight"].clone()
            out[p + f"mlp.{n}.bias"] = P[q + f"{n}.bias"].clone()
    out["vit.layernorm.weight"] = P["vision.ln_post.weight"].clone()
    out["vit.layernorm.bias"] = P["vision.ln_post.bias"].clone()
    C = cfg.num_classes
    out["classifier.weight"] = P["cls_head.weight"][:C].clone()
    out["classifier.bias"] = P["cls_head.bias"][:C].clone()
    assert set(out) == set(hf_sd), set(out) ^ set(hf_sd)
    return out


def from_hf(sd, cfg) -> dict[str, torch.Tensor]:
    """Inverse of to_hf: HF-named tensors (weights or gradients) in the build layout, the pad
    columns / rows zero."""
    from multimodal_llm_pretraining_amd import config as C

    v = cfg.vision
    out = {n: torch.zeros(s) for n, s in C.param_shapes(cfg).items()}
    w = sd["vit.embeddings.patch_embeddings.projection.weight"]
    out["vision.patch.weight"][:, :w[0].numel()] = w.reshape(w.shape[0], -1)
    out["vision.patch.bias"] = sd["vit.embeddings.patch_embeddings.projection.bias"].clone()
    out["vision.cls"] = sd["vit.embeddings.cls_token"].reshape(-1).clone()
    out["vision.pos"] = sd["vit.embeddings.position_embeddings"][0].clone()
    for i in range(v.layers):
        p, q = f"vit.layers.{i}.", f"vision.layers.{i}."
        out[q + "ln1.weight"] = sd[p + "layernorm_before.weight"].clone()
        out[q + "ln1.bias"] = sd[p + "layernorm_before.bias"].clone()
        out[q + "qkv.weight"] = torch.cat([sd[p + f"attention.{n}_proj.weight"] for n in "qkv"], 0)
        out[q + "qkv.bias"] = torch.cat([sd[p + f"attention.{n}_proj.bias"] for n in "qkv"], 0)
        out[q + "o.weight"] = sd[p + "attention.o_proj.weight"].clone()
        out[q + "o.bias"] = sd[p + "attention.o_proj.bias"].clone()
        out[q + "ln2.weight"] = sd[p + "layernorm_after.weight"].clone()
        out[q + "ln2.bias"] = sd[p + "layernorm_after.bias"].clone()
        for n in ("fc1", "fc2"):
            out[q + f"{n}.weight"] = sd[p + f"mlp.{n}.weight"].clone()
            out[q + f"{n}.bias"] = sd[p + f"mlp.{n}.bias"].clone()
    out["vision.ln_post.weight"] = sd["vit.layernorm.weight"].clone()
    out["vision.ln_post.bias"] = sd["vit.layernorm.bias"].clone()
    C_ = cfg.num_classes
    out["cls_head.weight"][:C_] = sd["classifier.weight"]
    out["cls_head.bias"][:C_] = sd["classifier.bias"]
    return out
