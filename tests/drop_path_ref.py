"""CPU restatement of the ConvNeXt classifier in training mode with stochastic depth (test
infrastructure only): convnext_oracle.logits_of / loss_and_grads with a `keep` argument.

`keep[j]` is a list of B bools for block j (counted over all stages): who HF's ConvNextDropPath
would keep.  The block's branch is applied as that module does, `h.div(keep_prob) * mask` on the
fp32 product gamma * h, with keep_prob = 1 - p_j and p_j = HF's linspace rate of the block; a block
with p_j == 0 is the plain residual (the module returns its input).  Pinned against the live HF
module, with torch.rand patched to give the wanted masks, by tests/test_drop_path_cpu.py.
"""

import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_oracle as CO  # noqa: E402

BF16 = torch.bfloat16


def rates(cfg) -> list:
    """HF ConvNextEncoder's per-block drop probabilities (fp32 values as Python floats)."""
    cn = cfg.convnext
    return torch.linspace(0, cn.drop_path_rate, sum(cn.depths), device="cpu").tolist()


def logits_of(P, cfg, pixels, keep, precision: str = "bf16", ln_policy: str = "cuda"):
    cn = cfg.convnext
    pr = rates(cfg)
    assert len(keep) == len(pr) and all(len(k) == pixels.shape[0] for k in keep)

    def ln(x, name, eps):  # x channels-last
        if ln_policy == "cuda":
            x = x.float()
        return F.layer_norm(x, (x.shape[-1],), P[name + ".weight"], P[name + ".bias"], eps)

    def ln_cf(x, name):
        return ln(x.permute(0, 2, 3, 1), name, cn.eps).permute(0, 3, 1, 2)

    ctx = torch.autocast("cpu", dtype=BF16) if precision == "bf16" else CO._null()
    blk = 0
    with ctx:
        x = F.conv2d(pixels, CO.conv_weights(P, cfg, "convnext.stem.weight"),
                     P["convnext.stem.bias"], stride=cn.patch)
        x = ln_cf(x, "convnext.stem_ln")
        for s, (C, depth) in enumerate(zip(cn.hidden_sizes, cn.depths)):
            p = f"convnext.stages.{s}."
            if s > 0:
                x = ln_cf(x, p + "down_ln")
                x = F.conv2d(x, CO.conv_weights(P, cfg, p + "down.weight"), P[p + "down.bias"],
                             stride=2)
            for j in range(depth):
                q = f"{p}layers.{j}."
                c = F.conv2d(x, CO.conv_weights(P, cfg, q + "dw.weight"), P[q + "dw.bias"],
                             padding=3, groups=C)
                h = ln(c.permute(0, 2, 3, 1), q + "ln", cn.eps)
                h = F.linear(h, P[q + "fc1.weight"], P[q + "fc1.bias"])
                h = F.gelu(h)
                h = F.linear(h, P[q + "fc2.weight"], P[q + "fc2.bias"])
                h = (P[q + "gamma"] * h).permute(0, 3, 1, 2)
                if pr[blk] != 0.0:  # ConvNextDropPath.forward in training mode
                    mask = torch.tensor(keep[blk], dtype=h.dtype).view(-1, 1, 1, 1)
                    h = h.div(1 - pr[blk]) * mask
                x = x + h
                blk += 1
        pooled = x.mean([-2, -1])
        if ln_policy == "cuda":
            pooled = pooled.float()
        pooled = F.layer_norm(pooled, (pooled.shape[-1],), P["convnext.ln_post.weight"],
                              P["convnext.ln_post.bias"], cn.head_eps)
        n = cfg.num_classes
        return F.linear(pooled, P["cls_head.weight"][:n], P["cls_head.bias"][:n])


def forward_loss(P, cfg, batch, keep, precision: str = "bf16", ln_policy: str = "cuda"):
    logits = logits_of(P, cfg, batch["pixel_values"], keep, precision, ln_policy)
    return F.cross_entropy(logits.float(), batch["labels"])


def loss_and_grads(P, cfg, batch, keep, precision="bf16", ln_policy="cuda"):
    Pr = {k: t.clone().requires_grad_() for k, t in P.items()}
    loss = forward_loss(Pr, cfg, batch, keep, precision, ln_policy)
    loss.backward()
    return loss.item(), {k: (t.grad if t.grad is not None else torch.zeros_like(t))
                         for k, t in Pr.items()}


def train_steps(P, cfg, batches, keeps, lrs, precision="bf16", betas=(0.9, 0.999), eps=1e-8,
                weight_decay=0.05):
    """convnext_oracle.train_steps with the masks of each step: torch.optim.AdamW, decoupled
    weight decay, no clipping, one optimizer step per batch."""
    params = {k: t.clone().requires_grad_() for k, t in P.items()}
    o = torch.optim.AdamW(list(params.values()), lr=lrs[0], betas=betas, eps=eps,
                          weight_decay=weight_decay, foreach=False)
    losses = []
    for i, (b, keep) in enumerate(zip(batches, keeps)):
        for gr in o.param_groups:
            gr["lr"] = lrs[i]
        loss = forward_loss(params, cfg, b, keep, precision)
        loss.backward()
        for t in params.values():
            if t.grad is None:
                t.grad = torch.zeros_like(t)
        o.step()
        o.zero_grad(set_to_none=True)
        losses.append(loss.item())
    return losses, {k: t.detach() for k, t in params.items()}
