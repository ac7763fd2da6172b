"""Hidden dropout on the GPU: the four mmpt_dropout_* entries against the numpy Philox
restatement of tests/test_dropout_cpu.py (masks bitwise, values bitwise the torch composition
of their definitions), then the engine at p = 0.1 against a masked CPU reference.

The masked reference restates the layer loops of oracle.model.text_forward / vision_forward
(with the oracle's own helpers) and injects, at the HF dropout sites (GPTNeoX emb_dropout /
post_attention_dropout / post_mlp_dropout, ViTEmbeddings / ViTSelfOutput / ViTOutput .dropout),
the masks mmpt_dropout_mask reports for the engine's sites, applied with the kernels'
one-rounding multiply.  Bars: the project's own from test_parity_gpu.py::test_loss_and_grads
(loss within 1e-4 of the fp32 reference and within 1e-4 + |bf16 - fp32| of the bf16 one, every
gradient tensor ‖Δ‖/‖ref‖ < 3e-2): dropout adds one multiply and one rounding per element.
"""

import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dropout_cpu import keep_mask, scale  # noqa: E402
from test_parity_gpu import oracle_cfg  # noqa: E402

from oracle import model as O  # noqa: E402

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
HI_SEED, HI_SITE = (0xDEADBEEF << 32) | 5, (0x12345678 << 32) | 0x9ABC
P_DROP, SEED = 0.1, 77


@pytest.fixture(scope="module")
def K():
    from multimodal_llm_pretraining_amd import kernels

    return kernels


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def np_mask(rows, h, p, seed, site) -> torch.Tensor:
    return torch.from_numpy(keep_mask(rows * h, p, seed, site)).view(rows, h)


def ref_drop(x: torch.Tensor, keep: torch.Tensor, p: float) -> torch.Tensor:
    """keep ? dtype(f32(x) * float(1/(1-p))) : +0 — one rounding; differentiable (the backward
    is the same map on the gradient)."""
    s = torch.tensor(float(scale(p)), dtype=torch.float32)
    return torch.where(keep.view_as(x), (x.float() * s).to(x.dtype), torch.zeros((), dtype=x.dtype))


# ------------------------------------------------------------------ masks
@pytest.mark.parametrize("rows,h", [(1, 8), (3, 72), (130, 256)])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed,site", [(1234, 7), (HI_SEED, 3), (42, HI_SITE)])
def test_mask_is_numpy_mask(K, rows, h, p, seed, site):
    want = np_mask(rows, h, p, seed, site)
    got = K.dropout_mask(rows * h, p, seed, site).cpu().view(rows, h)
    assert torch.equal(got.bool(), want)
    assert set(got.unique().tolist()) <= {0, 1}
    # the kernels walk (row, column octet): the same mask through the 2-D entries
    ones = torch.ones(rows, h, dtype=BF16, device="cuda")
    out = torch.empty_like(ones)
    K.dropout_bf16(ones, out, p, seed, site)
    assert torch.equal(out.cpu() != 0, want)
    onesf = torch.ones(rows, h, device="cuda")
    outf = torch.empty_like(onesf)
    K.dropout_f32(onesf, outf, p, seed, site)
    assert torch.equal(outf.cpu() != 0, want)
    K.dropout_add_f32(ones, site, torch.zeros_like(onesf), outf, p, seed)
    assert torch.equal(outf.cpu() != 0, want)


def test_sites_differing_in_the_high_word(K):
    n, lo = 130 * 256, 0x51
    a = K.dropout_mask(n, 0.5, 9, lo).cpu()
    b = K.dropout_mask(n, 0.5, 9, (1 << 32) | lo).cpu()
    c = K.dropout_mask(n, 0.5, 9 | (1 << 32), lo).cpu()  # and seeds likewise
    assert not torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(b, c)
    assert torch.equal(b.bool(), torch.from_numpy(keep_mask(n, 0.5, 9, (1 << 32) | lo)))
    # two different masks of p = 0.5 agree on about half the elements
    assert 0.45 < (a == b).float().mean().item() < 0.55


def test_p_zero_keeps_everything_bitwise(K):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(130, 256, generator=g).to(BF16).cuda()
    xf = torch.randn(130, 256, generator=g).cuda()
    assert bool(K.dropout_mask(130 * 256, 0.0, 5, 6).all())
    out = torch.empty_like(x)
    K.dropout_bf16(x, out, 0.0, 5, 6)
    assert torch.equal(bits(out), bits(x))
    outf = torch.empty_like(xf)
    K.dropout_f32(xf, outf, 0.0, 5, 6)
    assert torch.equal(bits(outf), bits(xf))
    K.dropout_add_f32(x, 6, xf, outf, 0.0, 5)
    assert torch.equal(bits(outf), bits(xf + x.float()))


def test_mask_statistics(K):
    """A condition on the generator (the kernel itself must match numpy exactly, above): the
    dropped share of n = 2^20 elements within 5 sigma of p, sigma = sqrt(p (1 - p) / n)."""
    n, p = 1 << 20, 0.1
    keep = K.dropout_mask(n, p, 1234, 7)
    dropped = 1.0 - keep.float().mean().item()
    sigma = (p * (1 - p) / n) ** 0.5
    print(f"dropped share {dropped:.6f} ({abs(dropped - p) / sigma:.2f} sigma)")
    assert abs(dropped - p) < 5 * sigma, (dropped, sigma)
    assert torch.equal(keep.cpu().bool(), torch.from_numpy(keep_mask(n, p, 1234, 7)))


# ------------------------------------------------------------------ values
@pytest.fixture(scope="module")
def vals():
    g = torch.Generator().manual_seed(3)
    rows, h = 130, 256
    return dict(rows=rows, h=h, x=torch.randn(rows, h, generator=g).to(BF16),
                x2=(torch.randn(rows, h, generator=g) * 3).to(BF16),
                xf=torch.randn(rows, h, generator=g), keep=np_mask(rows, h, 0.1, SEED, 11),
                keep2=np_mask(rows, h, 0.1, SEED, 12))


def test_dropout_bf16_values(K, vals):
    x, keep = vals["x"], vals["keep"]
    want = ref_drop(x, keep, 0.1)
    assert (bits(want)[~keep] == 0).all()  # +0, not -0
    xd = x.cuda()
    out = torch.empty_like(xd)
    K.dropout_bf16(xd, out, 0.1, SEED, 11)
    assert torch.equal(bits(out), bits(want))
    assert torch.equal(bits(xd), bits(x))  # the source is left alone
    K.dropout_bf16(xd, xd, 0.1, SEED, 11)  # in place
    assert torch.equal(bits(xd), bits(want))


def test_dropout_bf16_strided(K, vals):
    """ld_src > h and another ld_dst: the mask follows the logical index row*h + col."""
    x, keep, rows, h = vals["x"], vals["keep"], vals["rows"], vals["h"]
    src = torch.full((rows, h + 16), 7.0, dtype=BF16, device="cuda")
    src[:, :h] = x.cuda()
    dst = torch.full((rows, h + 40), 5.0, dtype=BF16, device="cuda")
    K.dropout_bf16(src[:, :h], dst[:, :h], 0.1, SEED, 11)
    assert torch.equal(bits(dst[:, :h]), bits(ref_drop(x, keep, 0.1)))
    assert bool((dst[:, h:] == 5.0).all()) and bool((src[:, h:] == 7.0).all())


def test_dropout_f32_values(K, vals):
    xf, keep = vals["xf"], vals["keep"]
    want = ref_drop(xf, keep, 0.1)
    xd = xf.cuda()
    out = torch.empty_like(xd)
    K.dropout_f32(xd, out, 0.1, SEED, 11)
    assert torch.equal(bits(out), bits(want))
    K.dropout_f32(xd, xd, 0.1, SEED, 11)
    assert torch.equal(bits(xd), bits(want))


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("alias", [False, True])
def test_dropout_add_f32_values(K, vals, two, alias):
    """out = resid + f32(v); v = drop(y), or bf16(drop(y2) + drop(y))."""
    y, y2, resid = vals["x"], vals["x2"], vals["xf"]
    v = ref_drop(y, vals["keep"], 0.1)
    if two:
        v = (ref_drop(y2, vals["keep2"], 0.1).float() + v.float()).to(BF16)
    want = resid + v.float()
    rd = resid.cuda()
    out = rd if alias else torch.empty_like(rd)
    K.dropout_add_f32(y.cuda(), 11, rd, out, 0.1, SEED, y2=y2.cuda() if two else None, site_y2=12)
    assert torch.equal(bits(out), bits(want))


def test_argument_errors(K):
    x = torch.zeros(2, 12, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 8"):
        K.dropout_bf16(x, torch.empty_like(x), 0.1, 1, 1)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        K.dropout_f32(x.float(), x.float(), 0.1, 1, 1)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        K.dropout_add_f32(x, 1, x.float(), x.float(), 0.1, 1)
    x = torch.zeros(2, 16, dtype=BF16, device="cuda")
    for p in (1.0, -0.25):
        with pytest.raises(RuntimeError, match=r"p must lie in \[0, 1\)"):
            K.dropout_bf16(x, torch.empty_like(x), p, 1, 1)
        with pytest.raises(RuntimeError, match=r"p must lie in \[0, 1\)"):
            K.dropout_f32(x.float(), x.float(), p, 1, 1)
        with pytest.raises(RuntimeError, match=r"p must lie in \[0, 1\)"):
            K.dropout_add_f32(x, 1, x.float(), x.float(), p, 1)
        with pytest.raises(RuntimeError, match=r"p must lie in \[0, 1\)"):
            K.dropout_mask(16, p, 1, 1)
    with pytest.raises(RuntimeError, match="aligned"):  # a view 2 bytes into the buffer
        K.dropout_bf16(torch.zeros(33, dtype=BF16, device="cuda")[1:].view(2, 16), x, 0.1, 1, 1)


# ------------------------------------------------------------------ engine vs masked reference
class Masks:
    """The keep masks of one micro-step's sites as the library reports them (mmpt_dropout_mask),
    applied the kernels' way.  rows: the packed token rows a tensor covers."""

    def __init__(self, K, cfg, seed, step, rank=0):
        from multimodal_llm_pretraining_amd.engine import dropout_site

        self.K, self.cfg, self.seed = K, cfg, seed
        self.site = lambda unit, k: dropout_site(step, rank, unit, k)
        self.cache = {}

    def __call__(self, x, p, unit, k, total_rows, rows=None):
        h = x.shape[-1]
        key = (unit, k)
        if key not in self.cache:
            m = self.K.dropout_mask(total_rows * h, p, self.seed, self.site(unit, k))
            self.cache[key] = m.cpu().bool().view(total_rows, h)
        m = self.cache[key]
        return ref_drop(x, m if rows is None else m[rows], p)


def masked_vision_forward(P, v, pixel_values, p, drop):
    """oracle.model.vision_forward (ViT: no pre_ln) with ViTEmbeddings.dropout,
    ViTSelfOutput.dropout and ViTOutput.dropout."""
    from multimodal_llm_pretraining_amd.engine import VISION_UNIT as VU

    B = pixel_values.shape[0]
    kk = v.channels * v.patch * v.patch
    w = P["vision.patch.weight"][:, :kk].reshape(v.hidden, v.channels, v.patch, v.patch)
    x = F.conv2d(pixel_values, w, P["vision.patch.bias"], stride=v.patch)
    x = x.flatten(2).transpose(1, 2)
    cls = P["vision.cls"].view(1, 1, -1).expand(B, -1, -1)
    h = torch.cat((cls, x), dim=1) + P["vision.pos"].unsqueeze(0)
    S = h.shape[1]
    T = B * S
    h = drop(h, p, VU, 0, T)
    D = v.hidden // v.heads
    for i in range(v.used_layers):
        pre = f"vision.layers.{i}."
        r = h
        y = F.layer_norm(h, (v.hidden,), P[pre + "ln1.weight"], P[pre + "ln1.bias"], v.eps)
        qkv = F.linear(y, P[pre + "qkv.weight"], P[pre + "qkv.bias"])
        q, k, vv = qkv.split(v.hidden, dim=-1)
        q, k, vv = (t.reshape(B, S, v.heads, D).transpose(1, 2) for t in (q, k, vv))
        a = O._sdpa(q, k, vv, False, D ** -0.5).transpose(1, 2).reshape(B, S, v.hidden)
        h = drop(F.linear(a, P[pre + "o.weight"], P[pre + "o.bias"]), p, VU + 1 + i, 0, T) + r
        r = h
        y = F.layer_norm(h, (v.hidden,), P[pre + "ln2.weight"], P[pre + "ln2.bias"], v.eps)
        y = F.gelu(F.linear(y, P[pre + "fc1.weight"], P[pre + "fc1.bias"]))
        h = drop(F.linear(y, P[pre + "fc2.weight"], P[pre + "fc2.bias"]), p, VU + 1 + i, 1, T) + r
    return h


def masked_text_forward(P, t, emb, p, drop, total_rows, rows=None):
    """oracle.model.text_forward with emb_dropout, post_attention_dropout, post_mlp_dropout;
    emb [B, S, h] covers the packed token rows `rows` (None: all of them)."""
    B, S, _ = emb.shape
    D, rot = t.head_dim, t.rot_dims
    cos, sin = O.rope_tables(t, S)
    cos = cos.to(emb.dtype)[None, None]
    sin = sin.to(emb.dtype)[None, None]
    h = drop(emb, p, 0, 0, total_rows, rows)
    for i in range(t.layers):
        pre = f"text.layers.{i}."
        y1 = F.layer_norm(h, (t.hidden,), P[pre + "ln1.weight"], P[pre + "ln1.bias"], t.eps)
        qkv = F.linear(y1, P[pre + "qkv.weight"], P[pre + "qkv.bias"])
        qkv = qkv.view(B, S, t.heads, 3 * D).transpose(1, 2)
        q, k, vv = qkv.chunk(3, dim=-1)
        qr, qp = q[..., :rot], q[..., rot:]
        kr, kp = k[..., :rot], k[..., rot:]
        q = torch.cat([qr * cos + O._rotate_half(qr) * sin, qp], dim=-1)
        k = torch.cat([kr * cos + O._rotate_half(kr) * sin, kp], dim=-1)
        a = O._sdpa(q, k, vv, True, D ** -0.5).transpose(1, 2).reshape(B, S, t.hidden)
        attn = F.linear(a, P[pre + "dense.weight"], P[pre + "dense.bias"])
        attn = drop(attn, p, 1 + i, 0, total_rows, rows)
        y2 = F.layer_norm(h, (t.hidden,), P[pre + "ln2.weight"], P[pre + "ln2.bias"], t.eps)
        mlp = F.linear(F.gelu(F.linear(y2, P[pre + "fc1.weight"], P[pre + "fc1.bias"])),
                       P[pre + "fc2.weight"], P[pre + "fc2.bias"])
        mlp = drop(mlp, p, 1 + i, 1, total_rows, rows)
        h = mlp + attn + h
    h = F.layer_norm(h, (t.hidden,), P["text.final_ln.weight"], P["text.final_ln.bias"], t.eps)
    return F.linear(h, P["text.lm_head"])


def masked_forward_loss(P, cfg, ocfg, batch, precision, drop, lens=None):
    """oracle.model.forward_loss with the dropout sites; lens: a right-padded text batch, run
    sequence by sequence over its valid tokens (the packed rows the engine computes over)."""
    pt = cfg.text.hidden_dropout
    ctx = torch.autocast("cpu", dtype=BF16) if precision == "bf16" else O._null()
    ids, labels = batch["input_ids"], batch["labels"]
    with ctx:
        if lens is not None:
            total, cu = sum(lens), np.concatenate(([0], np.cumsum(lens)))
            loss = 0.0
            for b, n in enumerate(lens):
                emb = F.embedding(ids[b:b + 1, :n], P["text.embed"])
                logits = masked_text_forward(P, ocfg.text, emb, pt, drop, total,
                                             slice(int(cu[b]), int(cu[b + 1])))
                loss = loss + O.causal_lm_loss(logits, labels[b:b + 1, :n], 1)
            return loss / sum(n - 1 for n in lens)
        emb = F.embedding(ids, P["text.embed"])
        if ocfg.vision is not None:
            feats = masked_vision_forward(P, ocfg.vision, batch["pixel_values"],
                                          cfg.vision.hidden_dropout, drop)[:, 1:]
            x = F.linear(feats, P["proj.fc1.weight"], P["proj.fc1.bias"])
            x = F.linear(F.gelu(x), P["proj.fc2.weight"], P["proj.fc2.bias"])
            mask = (ids == ocfg.image_token_id).unsqueeze(-1).expand_as(emb)
            emb = emb.masked_scatter(mask, x.to(emb.dtype))
        logits = masked_text_forward(P, ocfg.text, emb, pt, drop, ids.numel())
    return O.causal_lm_loss(logits, labels)


def engine_run(cfg, P, batch, seed=SEED, checkpointing=False, steps=1, mask=None, rank=0):
    """Fresh engine, `steps` micro-steps on the same batch: ([loss per step], flat grads)."""
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.engine import Batch, Engine
    from multimodal_llm_pretraining_amd.params import ParamStore

    store = ParamStore(C.param_shapes(cfg), "cuda")
    store.load(P)
    store.refresh_shadow()
    eng = Engine(cfg, store)
    eng.dropout_seed, eng.checkpointing, eng.rank = seed, checkpointing, rank
    b = Batch(cfg, batch["input_ids"], batch["labels"], batch.get("pixel_values"), store.device,
              attention_mask=mask)
    losses = []
    for _ in range(steps):
        loss_sum = eng.forward(b, 1.0 / b.num_items)
        eng.backward(b)
        losses.append(loss_sum.item() / b.num_items)
    torch.cuda.synchronize()
    return losses, store, b


def drop_cfg(name):
    from multimodal_llm_pretraining_amd import config as C

    return C.with_dropout(C.get_config("tiny-lm"), text=P_DROP) if name == "tiny-lm" else \
        C.get_config(name)


@pytest.fixture(scope="module")
def runs(K):
    """Per config: the engine's first micro-step at p = 0.1 and the masked references."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        cfg = drop_cfg(name)
        ocfg = oracle_cfg(cfg)
        P = O.init_params(ocfg, seed=0)
        batch = O.make_batch(ocfg, 3, 130 if name == "tiny-lm" else 47, seed=1)
        (loss,), store, _ = engine_run(cfg, P, batch)
        cache[name] = dict(cfg=cfg, ocfg=ocfg, P=P, batch=batch, loss=loss, store=store,
                           grad=store.grad.clone())
        return cache[name]

    return get


@pytest.mark.parametrize("name", ["tiny-lm", "tiny-mm-drop"])
def test_engine_matches_masked_reference(K, runs, name):
    r = runs(name)
    cfg, ocfg, P, batch = r["cfg"], r["ocfg"], r["P"], r["batch"]
    drop = Masks(K, cfg, SEED, step=0)
    Pr = {k: v.clone().requires_grad_() for k, v in P.items()}
    ref = masked_forward_loss(Pr, cfg, ocfg, batch, "bf16", drop)
    ref.backward()
    with torch.no_grad():
        ref32 = masked_forward_loss(P, cfg, ocfg, batch, "fp32", drop).item()
    # the same bars against the reference WITHOUT masks must fail, or they would show nothing
    P0 = {k: v.clone().requires_grad_() for k, v in P.items()}
    nodrop = O.forward_loss(P0, ocfg, batch, "bf16")
    nodrop.backward()
    floor = abs(ref.item() - ref32)
    loss = r["loss"]
    print(f"{name}: GPU {loss:.7f}, masked fp32 {ref32:.7f} (d {loss - ref32:+.2e}), masked bf16 "
          f"{ref.item():.7f} (d {loss - ref.item():+.2e}, floor {floor:.2e}); p = 0 bf16 "
          f"{nodrop.item():.7f}")
    unmasked = max(((r["store"].g(k).cpu() - P0[k].grad).norm() / P0[k].grad.norm()).item()
                   for k in P)
    assert unmasked > 0.1, unmasked
    assert abs(loss - ref32) < 1e-4, (loss, ref32)
    assert abs(loss - ref.item()) < 1e-4 + floor, (loss, ref.item(), floor)
    worst = ("", 0.0)
    for k in P:
        g = r["store"].g(k).cpu()
        rg = Pr[k].grad
        err = ((g - rg).norm() / (rg.norm() + 1e-20)).item()
        worst = max(worst, (k, err), key=lambda e: e[1])
        assert err < 3e-2, (k, err)
    print(f"{name}: worst gradient {worst[0]} {worst[1]:.2e}")


def test_padded_batch_matches_masked_reference(K, runs):
    """Right-padded tiny-lm batch: the sites act on the packed token rows.

    32 sequences of 33 .. 130 tokens (2649 valid tokens), because the 1e-4 bar is a bar on bf16
    rounding noise, which the batch has to average down — the reason test_loss_and_grads runs
    tiny-clip-d80 on 32 samples.  Measured on the CPU reference alone (std of its bf16 loss
    under 1e-7 relative weight perturbations; the fp32 loss moves by 2e-7): 3.3e-5 for three
    sequences of 130 / 77 / 101 tokens, where its own |bf16 - fp32| reached 1.9e-4 at p = 0 and
    1.3e-4 at p = 0.1 (six seeds), so no bf16 implementation holds 1e-4 there (the engine:
    -1.4e-4 .. +2e-5 over the same seeds, no sign); 9e-6 for this batch."""
    r = runs("tiny-lm")
    cfg, ocfg, P = r["cfg"], r["ocfg"], r["P"]
    lens = [130] + [33 + (37 * i) % 98 for i in range(1, 32)]
    batch = O.make_batch(ocfg, len(lens), 130, seed=1)
    mask = torch.zeros_like(batch["input_ids"])
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    (loss,), _, bt = engine_run(cfg, P, batch, mask=mask)
    assert bt.T == sum(lens) and bt.num_items == sum(n - 1 for n in lens)
    drop = Masks(K, cfg, SEED, step=0)
    with torch.no_grad():
        ref = masked_forward_loss(P, cfg, ocfg, batch, "bf16", drop, lens).item()
        ref32 = masked_forward_loss(P, cfg, ocfg, batch, "fp32", drop, lens).item()
    floor = abs(ref - ref32)
    print(f"padded: GPU {loss:.7f}, masked fp32 {ref32:.7f}, masked bf16 {ref:.7f}")
    assert abs(loss - ref32) < 1e-4, (loss, ref32)
    assert abs(loss - ref) < 1e-4 + floor, (loss, ref, floor)


# ------------------------------------------------------------------ engine behaviour
@pytest.mark.parametrize("name", ["tiny-lm", "tiny-mm-drop"])
def test_checkpointing_draws_the_same_masks(runs, name):
    r = runs(name)
    (loss,), store, _ = engine_run(r["cfg"], r["P"], r["batch"], checkpointing=True)
    assert loss == r["loss"]
    assert torch.equal(store.grad, r["grad"])


def test_seed_and_micro_step(runs):
    r = runs("tiny-lm")
    losses, store, _ = engine_run(r["cfg"], r["P"], r["batch"], steps=2)
    assert losses[0] == r["loss"]  # the same seed on a fresh engine: bitwise
    assert losses[1] != losses[0]  # the second micro-step draws new masks
    assert not torch.equal(store.grad, r["grad"])  # (two micro-steps accumulated)
    (again,), store2, _ = engine_run(r["cfg"], r["P"], r["batch"])
    assert again == r["loss"] and torch.equal(store2.grad, r["grad"])
    (other,), store3, _ = engine_run(r["cfg"], r["P"], r["batch"], seed=SEED + 1)
    assert other != r["loss"] and not torch.equal(store3.grad, r["grad"])


def test_ranks_draw_different_masks(runs):
    r = runs("tiny-lm")
    (loss,), store, _ = engine_run(r["cfg"], r["P"], r["batch"], rank=1)
    assert loss != r["loss"] and not torch.equal(store.grad, r["grad"])


def test_eval_is_the_p0_model(runs):
    """MMPTForPretraining: dropout iff train() and p > 0; eval() is bitwise the p = 0 model."""
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining

    r = runs("tiny-mm-drop")
    bd = {k: v.cuda() for k, v in r["batch"].items()}

    def model(cfg):
        m = MMPTForPretraining(cfg, "cuda", seed=SEED)
        m.store.load(r["P"])
        m.store.refresh_shadow()
        return m

    md, m0 = model(r["cfg"]), model(C.get_config("tiny-mm"))
    assert md.engine.dropout_seed == SEED
    train = md(**bd).loss.item()
    assert abs(train - r["loss"]) < 1e-6  # the engine's first micro-step (the loss / denom form)
    md.eval()
    ev = md(**bd).loss.item()
    base = m0(**bd).loss.item()
    assert ev == base and ev != train
    md.train()
    md.set_dropout_seed(SEED + 5)
    assert md(**bd).loss.item() not in (train, ev)
