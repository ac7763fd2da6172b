"""Padded batches on the GPU: the varlen attention kernels and the positional rope through
kernels.py, then the whole model (`MMPTForPretraining(attention_mask=...)`, the trainer) on
right-padded batches against the same sequences run one at a time through the dense path."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
NAN = float("nan")
SENTINEL = 64  # rows allocated past total_tokens in out / dqkv (must stay untouched)


@pytest.fixture(scope="module")
def K():
    from multimodal_llm_pretraining_amd import kernels

    return kernels


def bf(x):
    return x.to(torch.bfloat16)


def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def same_bits(a, b):
    """Bitwise equality that also holds for NaN payloads."""
    if a.dtype == torch.bfloat16:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ kernels
class Layout:
    """Fused-qkv geometry in the mmpt_attention_gqa_* terms."""

    def __init__(self, kind, H, Hk, D):
        self.kind, self.H, self.Hk, self.D = kind, H, Hk, D
        if kind == "interleaved":  # GPTNeoX: [t][h][q|k|v][D]
            assert H == Hk
            self.hs, self.koff, self.voff, self.width = 3 * D, D, 2 * D, 3 * H * D
        else:  # Llama: [t][q heads | k heads | v heads]
            self.hs, self.koff, self.voff, self.width = D, H * D, (H + Hk) * D, (H + 2 * Hk) * D

    def cols(self, part, h):
        """Columns of q head h (part 0) or of kv head h (part 1: k, 2: v)."""
        if part == 0:
            o = h * self.hs
        else:
            o = (self.koff if part == 1 else self.voff) + h * self.hs
        return slice(o, o + self.D)

    def dense_fwd(self, K, qkv, B, S, causal, scale, out, lse):
        if self.kind == "interleaved":
            K.attention_fwd(qkv, B, S, self.H, self.D, self.hs, self.D, causal, scale, out, lse)
        else:
            K.attention_gqa_fwd(qkv, B, S, self.H, self.Hk, self.D, self.koff, self.voff, causal,
                                scale, out, lse)

    def dense_bwd(self, K, qkv, B, S, causal, scale, out, dout, lse, dqkv):
        if self.kind == "interleaved":
            K.attention_bwd(qkv, B, S, self.H, self.D, self.hs, self.D, causal, scale, out, dout,
                            lse, dqkv)
        else:
            K.attention_gqa_bwd(qkv, B, S, self.H, self.Hk, self.D, self.koff, self.voff, causal,
                                scale, out, dout, lse, dqkv)


def run_varlen(K, L, lens, causal, seed, max_seq=None):
    """Varlen forward + backward over NaN-filled outputs with sentinel rows."""
    torch.manual_seed(seed)
    T, B, mx = sum(lens), len(lens), max_seq or max(lens)
    cu = K.cu_seqlens_of(lens).to(dev)
    qkv = bf(torch.randn(T + SENTINEL, L.width, device=dev))
    dout = bf(torch.randn(T + SENTINEL, L.H * L.D, device=dev))
    out = torch.full((T + SENTINEL, L.H * L.D), NAN, device=dev, dtype=torch.bfloat16)
    lse = torch.full((B * L.H * mx,), NAN, device=dev)
    dqkv = torch.full((T + SENTINEL, L.width), NAN, device=dev, dtype=torch.bfloat16)
    scale = L.D ** -0.5
    K.attention_varlen_fwd(qkv, lens, cu, L.H, L.Hk, L.D, L.hs, L.koff, L.voff, causal, scale, out,
                           lse, max_seq=mx)
    K.attention_varlen_bwd(qkv, lens, cu, L.H, L.Hk, L.D, L.hs, L.koff, L.voff, causal, scale, out,
                           dout, lse, dqkv, max_seq=mx)
    torch.cuda.synchronize()
    return dict(qkv=qkv, dout=dout, out=out, lse=lse.view(B, L.H, mx), dqkv=dqkv, cu=cu.tolist(),
                scale=scale, T=T, mx=mx)


def dense_single(K, L, r, b, n, causal):
    """The existing dense entry on sequence b alone (batch = 1, seq = n)."""
    rows = slice(r["cu"][b], r["cu"][b + 1])
    qkv, dout = r["qkv"][rows], r["dout"][rows]
    out = torch.full((n, L.H * L.D), NAN, device=dev, dtype=torch.bfloat16)
    lse = torch.full((L.H * n,), NAN, device=dev)
    L.dense_fwd(K, qkv, 1, n, causal, r["scale"], out, lse)
    dqkv = torch.full((n, L.width), NAN, device=dev, dtype=torch.bfloat16)
    L.dense_bwd(K, qkv, 1, n, causal, r["scale"], out, dout, lse, dqkv)
    return out, lse.view(L.H, n), dqkv


def sdpa_single(L, r, b, causal):
    """fp32 reference of sequence b: out [n][H*D] and the gradient of the fused qkv rows."""
    rows = slice(r["cu"][b], r["cu"][b + 1])
    x = r["qkv"][rows].float().requires_grad_()
    G = L.H // L.Hk
    outs = []
    for h in range(L.H):
        q, k, v = x[:, L.cols(0, h)], x[:, L.cols(1, h // G)], x[:, L.cols(2, h // G)]
        s = (q @ k.t()) * r["scale"]
        if causal:
            n = s.shape[0]
            s = s.masked_fill(torch.triu(torch.ones(n, n, device=dev, dtype=torch.bool), 1), -math.inf)
        outs.append(torch.softmax(s, -1) @ v)
    o = torch.cat(outs, 1)
    o.backward(r["dout"][rows].float())
    return o.detach(), x.grad


KERNEL_CASES = [(D, causal, "interleaved", 2, 2, [1, 64, 65, 200])
                for D in (64, 80, 128) for causal in (True, False)]
KERNEL_CASES += [(256, causal, "interleaved", 2, 2, [1, 70, 128, 129, 257]) for causal in (True, False)]
KERNEL_CASES += [(64, True, "llama", 4, 2, [1, 64, 65, 200])]  # GQA


@pytest.mark.parametrize("D,causal,kind,H,Hk,lens", KERNEL_CASES)
def test_varlen_attention(K, D, causal, kind, H, Hk, lens):
    """(a) fp32 per-sequence SDPA reference at test_attention_fwd_bwd's tolerances; (b) every
    sequence bitwise the dense entry on that sequence alone; (d) no NaN left in a valid row,
    sentinel rows and lse tails untouched.

    D = 256: the dense entry's default backward is the wave-pair dK/dV kernel + dQ from the dS
    tiles, the varlen backward the ring dK/dV kernel + the recomputing dQ kernel (what
    MMPT_ATTN_DS=0 selects).  dK / dV rely on test_attention_dkdv_pair_bitwise_vs_ring's
    equality; dQ is compared bitwise with the dense entry both under MMPT_ATTN_DS=0 (the same
    kernel) and as it runs by default (measured on an MI355X: 0 differing elements in all ten
    (causal, length) cases here, although the existing test_attention_dq_recompute_path only
    pins the two dense dQ paths to 1e-2)."""
    from multimodal_llm_pretraining_amd import _lib

    L = Layout(kind, H, Hk, D)
    r = run_varlen(K, L, lens, causal, seed=100 + D)
    T = r["T"]
    # (d)
    assert not torch.isnan(r["out"][:T].float()).any()
    assert not torch.isnan(r["dqkv"][:T].float()).any()  # (q, k, v parts fill the row)
    assert torch.isnan(r["out"][T:].float()).all() and torch.isnan(r["dqkv"][T:].float()).all()
    for b, n in enumerate(lens):
        assert not torch.isnan(r["lse"][b, :, :n]).any()
        assert torch.isnan(r["lse"][b, :, n:]).all()
    # (a) over the packed tensors, as test_attention_fwd_bwd takes its relative errors over the
    # batch (a one-token causal sequence has dQ = dK = 0 exactly: no relative error of its own)
    refs = [sdpa_single(L, r, b, causal) for b in range(len(lens))]
    o_ref, g_ref = (torch.cat([x[i] for x in refs]) for i in (0, 1))
    assert relerr(r["out"][:T], o_ref) < 1e-2
    for part, heads in ((0, H), (1, Hk), (2, Hk)):
        cols = torch.cat([torch.arange(L.width, device=dev)[L.cols(part, h)] for h in range(heads)])
        assert relerr(r["dqkv"][:T][:, cols], g_ref[:, cols]) < 2e-2, part
    for b, n in enumerate(lens):
        rows = slice(r["cu"][b], r["cu"][b + 1])
        # (b)
        out1, lse1, dqkv1 = dense_single(K, L, r, b, n, causal)
        assert same_bits(r["out"][rows], out1), (b, n)
        assert same_bits(r["lse"][b, :, :n].contiguous(), lse1), (b, n)
        dq_ref = dqkv1
        if D == 256:
            prev = _lib.set_switch("MMPT_ATTN_DS", 0)
            try:
                dq_ref = dense_single(K, L, r, b, n, causal)[2]
            finally:
                _lib.set_switch("MMPT_ATTN_DS", prev)
            nd = sum(int((r["dqkv"][rows, L.cols(0, h)].view(torch.int16) !=
                          dqkv1[:, L.cols(0, h)].view(torch.int16)).sum()) for h in range(H))
            print(f"D=256 causal={causal} len={n}: dQ elements differing from the default "
                  f"(dS-tile) dense path: {nd} of {n * H * D}")
        for h in range(H):
            c = L.cols(0, h)
            assert same_bits(r["dqkv"][rows, c].contiguous(), dq_ref[:, c].contiguous()), (b, n, h)
            assert same_bits(r["dqkv"][rows, c].contiguous(), dqkv1[:, c].contiguous()), (b, n, h)
        for j in range(Hk):
            for part in (1, 2):
                c = L.cols(part, j)
                assert same_bits(r["dqkv"][rows, c].contiguous(), dqkv1[:, c].contiguous()), \
                    (b, n, j, part)


@pytest.mark.parametrize("D,S", [(64, 130), (80, 130), (128, 130), (256, 257)])
@pytest.mark.parametrize("causal", [True, False])
def test_varlen_equal_lengths_is_dense(K, D, S, causal):
    """(c) all lengths equal to max_seq: bitwise the dense call (D = 256 dQ: the dense call
    under MMPT_ATTN_DS=0, see test_varlen_attention)."""
    from multimodal_llm_pretraining_amd import _lib

    B, H = 3, 2
    L = Layout("interleaved", H, H, D)
    r = run_varlen(K, L, [S] * B, causal, seed=7)
    T = B * S
    qkv, dout = r["qkv"][:T], r["dout"][:T]
    out = torch.full((T, H * D), NAN, device=dev, dtype=torch.bfloat16)
    lse = torch.full((B * H * S,), NAN, device=dev)
    L.dense_fwd(K, qkv, B, S, causal, r["scale"], out, lse)
    got = {}
    prev = _lib.set_switch("MMPT_ATTN_DS", 1)
    try:
        for mode in ((1, 0) if D == 256 else (1,)):
            _lib.set_switch("MMPT_ATTN_DS", mode)
            dqkv = torch.full((T, L.width), NAN, device=dev, dtype=torch.bfloat16)
            L.dense_bwd(K, qkv, B, S, causal, r["scale"], out, dout, lse, dqkv)
            got[mode] = dqkv
    finally:
        _lib.set_switch("MMPT_ATTN_DS", prev)
    assert same_bits(r["out"][:T], out)
    assert same_bits(r["lse"].reshape(-1), lse)
    for h in range(H):
        assert same_bits(r["dqkv"][:T, L.cols(0, h)].contiguous(),
                         got[0 if D == 256 else 1][:, L.cols(0, h)].contiguous())
        for part in (1, 2):
            c = L.cols(part, h)
            assert same_bits(r["dqkv"][:T, c].contiguous(), got[1][:, c].contiguous())


def test_varlen_max_seq_wider_than_longest(K):
    """max_seq above the longest length (the engine passes the batch's longest, a caller may
    pass the padded width): more empty work items, the same bits."""
    L = Layout("interleaved", 2, 2, 128)
    lens = [1, 64, 65, 200]
    a = run_varlen(K, L, lens, True, seed=3)
    b = run_varlen(K, L, lens, True, seed=3, max_seq=333)
    assert same_bits(a["out"], b["out"]) and same_bits(a["dqkv"], b["dqkv"])
    for i, n in enumerate(lens):
        assert same_bits(a["lse"][i, :, :n].contiguous(), b["lse"][i, :, :n].contiguous())
        assert torch.isnan(b["lse"][i, :, n:]).all()


def _tables(rot, rows):
    inv = 1.0 / (10000 ** (torch.arange(0, rot, 2, dtype=torch.float) / rot))
    fr = torch.arange(rows, dtype=torch.float)[:, None] * inv[None]
    emb = torch.cat([fr, fr], -1)
    return emb.cos().to(dev).contiguous(), emb.sin().to(dev).contiguous()


@pytest.mark.parametrize("rot", [64, 20, 10])  # 16-B vector path / pair kernel (two / one pairs)
def test_rope_positions(K, rot):
    """(e) pos = t % seq: bitwise the existing call, forward and inverse; ragged positions
    against a torch restatement at test_rope_roundtrip's tolerance (4e-3)."""
    torch.manual_seed(4)
    S, H, D = 50, 2, 256
    T = 2 * S
    qkv = bf(torch.randn(T, H * 3 * D, device=dev))
    cos, sin = _tables(rot, S)
    pos = (torch.arange(T, device=dev) % S).to(torch.int32)
    for inverse in (False, True):
        a, b = qkv.clone(), qkv.clone()
        K.rope_inplace(a, S, H, D, rot, 3 * D, D, cos, sin, inverse=inverse)
        K.rope_inplace(b, S, H, D, rot, 3 * D, D, cos, sin, inverse=inverse, pos=pos)
        assert same_bits(a, b)
    lens = [1, 17, 50, 32]
    rag = torch.cat([torch.arange(n) for n in lens]).to(dev, torch.int32)
    x = qkv.clone()
    K.rope_inplace(x, S, H, D, rot, 3 * D, D, cos, sin, pos=rag)
    v = qkv.view(T, H, 3, D).float()
    c, s_ = cos[rag.long()][:, None, :], sin[rag.long()][:, None, :]
    for p in (0, 1):
        r = v[:, :, p, :rot]
        rh = torch.cat([-r[..., rot // 2:], r[..., :rot // 2]], -1)
        ref = torch.cat([r * c + rh * s_, v[:, :, p, rot:]], -1)
        assert relerr(x.view(T, H, 3, D)[:, :, p], ref) < 4e-3
    assert torch.equal(x.view(T, H, 3, D)[:, :, 2], qkv.view(T, H, 3, D)[:, :, 2])
    K.rope_inplace(x, S, H, D, rot, 3 * D, D, cos, sin, inverse=True, pos=rag)
    assert relerr(x, qkv) < 8e-3
    with pytest.raises(ValueError):
        K.rope_inplace(x, S, H, D, rot, 3 * D, D, cos, sin, pos=rag[:-1])


def test_varlen_argument_errors(K):
    """(f) the C entries refuse a null cu_seqlens, max_seq = 0 and an unsupported head dim; the
    wrappers refuse a malformed host length list before calling into C."""
    from multimodal_llm_pretraining_amd import _lib

    H, D, lens = 2, 64, [3, 5]
    T = sum(lens)
    qkv = bf(torch.randn(T, 3 * H * D, device=dev))
    out = torch.empty(T, H * D, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(2 * H * 5, device=dev)
    cu = K.cu_seqlens_of(lens).to(dev)
    ws = torch.empty(4096, device=dev, dtype=torch.uint8)

    def fwd(batch=2, mx=5, total=T, d=D, cup=cu.data_ptr()):
        _lib.call("mmpt_attention_varlen_fwd", batch, mx, total, H, H, d, qkv.data_ptr(), 3 * H * D,
                  3 * D, D, 2 * D, 1, 0.125, cup, out.data_ptr(), H * D, lse.data_ptr(), None)

    def bwd(batch=2, mx=5, total=T, d=D, cup=cu.data_ptr()):
        _lib.call("mmpt_attention_varlen_bwd", batch, mx, total, H, H, d, qkv.data_ptr(), 3 * H * D,
                  3 * D, D, 2 * D, 1, 0.125, cup, out.data_ptr(), out.data_ptr(), H * D,
                  lse.data_ptr(), qkv.data_ptr(), ws.data_ptr(), None)

    for f in (fwd, bwd):
        with pytest.raises(RuntimeError, match="cu_seqlens"):
            f(cup=None)
        with pytest.raises(RuntimeError, match="max_seq"):
            f(mx=0)
        with pytest.raises(RuntimeError, match="head_dim"):
            f(d=72)
        with pytest.raises(RuntimeError, match="total_tokens"):
            f(total=1)
        with pytest.raises(RuntimeError, match="total_tokens"):
            f(total=11)
    for bad in ([3, 0], [], [3, 6]):
        with pytest.raises(ValueError):
            K.attention_varlen_fwd(qkv, bad, cu, H, H, D, 3 * D, D, 2 * D, True, 0.125, out, lse,
                                   max_seq=5)
    with pytest.raises(ValueError):  # cu_seqlens of another batch size
        K.attention_varlen_fwd(qkv, [3, 4, 1], cu, H, H, D, 3 * D, D, 2 * D, True, 0.125, out, lse)
    assert _lib.query("mmpt_attention_varlen_bwd_workspace_bytes", 3, 100, 4, 256) == 3 * 100 * 4 * 4


# ------------------------------------------------------------------ model
# Tolerance of the padded step against its sequences run one at a time (same denominator):
# twice the discrepancy the DENSE path of the parent commit shows between a dense [3, L] batch
# and its three single-sequence runs — pure summation-order noise (bf16 rounding of a weight
# gradient summed over another set of rows) in code the varlen path does not change.  Measured
# on an MI355X at the parent commit with `dense_noise` below (same configs, widths and seeds;
# the kernels have no atomics, so the figures reproduce): the worst per-parameter relative L2
# error of the gradient, and the relative loss difference.
DENSE_NOISE = {
    "tiny-lm": (2.3953e-3, 0.0),
    "tiny-lm-d80": (2.4228e-3, 3.805e-8),
    "tiny-mm": (2.5734e-3, 6.774e-8),
    "tiny-llava": (3.0946e-3, 6.803e-8),
}
MODELS = list(DENSE_NOISE)
# The loss is one fp32 scalar: its discrepancy is a whole number of fp32 roundings (2^-24 =
# 5.96e-8 relative each), and tiny-lm's dense figure is 0 because that draw happened to round
# the same way, not because its sum is exact.  The loss bound is therefore twice the WORST
# dense figure of the four models (6.803e-8), for every model; the gradient bound stays per
# model.
LOSS_NOISE = max(v[1] for v in DENSE_NOISE.values())


def tolerances(name):
    return 2 * DENSE_NOISE[name][0], 2 * LOSS_NOISE
TEXT_LEN = 37  # full-width row: odd, several rope positions; a second row in between


def model_batch(name, seed=0, text_lens=None):
    """Right-padded batch of 3 sequences: one of full width, one of the minimum length that
    still carries a label (2 tokens text-only, num_patches + 1 multimodal: a sequence without
    any label cannot be run alone through the dense path, whose loss rows would be empty), one
    in between."""
    from multimodal_llm_pretraining_amd import config as C

    cfg = C.get_config(name)
    g = torch.Generator().manual_seed(seed)
    npch = cfg.vision.num_patches if cfg.multimodal else 0
    text_lens = text_lens or [TEXT_LEN, 1 if cfg.multimodal else 2, 18]
    lens = [npch + n for n in text_lens]
    W, B = max(lens), len(lens)
    ids = torch.zeros((B, W), dtype=torch.int64)
    labels = torch.full((B, W), -100, dtype=torch.int64)
    mask = torch.zeros((B, W), dtype=torch.int64)
    hi = cfg.image_token_id if cfg.multimodal else cfg.text.n_vocab
    for b, (n, L) in enumerate(zip(text_lens, lens)):
        row = torch.cat([torch.full((npch,), cfg.image_token_id if cfg.multimodal else 0),
                         torch.randint(0, hi, (n,), generator=g)])
        ids[b, :L], labels[b, :L], mask[b, :L] = row, row, 1
        labels[b, :npch] = -100
    pix = torch.rand(B, 3, cfg.vision.image, cfg.vision.image, generator=g) if cfg.multimodal \
        else None
    shifted = torch.full_like(labels, -100)
    shifted[:, :-1] = labels[:, 1:]
    return dict(cfg=cfg, ids=ids, labels=labels, mask=mask, pix=pix, lens=lens,
                denom=int((shifted != -100).sum()))


def run_model(model, ids, labels, pix, denom, mask=None):
    """One forward + backward that ACCUMULATES into the flat gradient buffer; returns the
    loss (the fp32 scalar as a python float)."""
    kw = {} if mask is None else {"attention_mask": mask}
    loss = model(input_ids=ids, labels=labels, pixel_values=pix, num_items_in_batch=denom,
                 **kw).loss
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().double().item()


def singles(model, mb):
    """The sequences one at a time through the dense path (B = 1, no mask), gradients
    accumulated, the batch's denominator."""
    model.store.zero_grad()
    total = 0.0
    for b, n in enumerate(mb["lens"]):
        pix = None if mb["pix"] is None else mb["pix"][b:b + 1]
        total += run_model(model, mb["ids"][b:b + 1, :n], mb["labels"][b:b + 1, :n], pix, mb["denom"])
    return total, model.store.grad.clone()


def grad_errors(model, got, ref):
    """Worst per-parameter relative L2 error over the trainable parameters with a gradient."""
    worst, where = 0.0, None
    for n in model.store.names():
        o, k = model.store.offsets[n], model.store.g(n).numel()
        a, b = got[o:o + k].double(), ref[o:o + k].double()
        if float(b.norm()) == 0.0:
            assert float(a.norm()) == 0.0, n
            continue
        e = float((a - b).norm() / b.norm())
        if e > worst:
            worst, where = e, n
    return worst, where


def dense_noise(name):
    """The yardstick: a dense [3, L] batch (all rows of full width, no mask) against its three
    single-sequence runs, on the dense path only."""
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining

    mb = model_batch(name, text_lens=[TEXT_LEN] * 3)
    model = MMPTForPretraining(mb["cfg"], dev, seed=0)
    model.store.zero_grad()
    loss = run_model(model, mb["ids"], mb["labels"], mb["pix"], mb["denom"])
    g = model.store.grad.clone()
    loss1, g1 = singles(model, mb)
    return grad_errors(model, g, g1)[0], abs(loss - loss1) / abs(loss1)


@pytest.fixture(scope="module")
def padded_runs():
    """Per model: the module, the batch, the padded run and the single-sequence reference —
    computed once, shared by the tests below and left unchanged."""
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining

    cache = {}

    def get(name):
        if name not in cache:
            mb = model_batch(name)
            model = MMPTForPretraining(mb["cfg"], dev, seed=0)
            loss1, g1 = singles(model, mb)
            model.store.zero_grad()
            loss = run_model(model, mb["ids"], mb["labels"], mb["pix"], mb["denom"], mb["mask"])
            cache[name] = dict(model=model, mb=mb, loss=loss, grad=model.store.grad.clone(),
                               loss1=loss1, grad1=g1)
        return cache[name]

    return get


@pytest.mark.parametrize("name", MODELS)
def test_padded_batch_matches_single_sequences(padded_runs, name):
    """Loss and every parameter gradient of the right-padded batch equal the accumulated
    result of its three sequences run alone through the dense path, within 2x the dense path's
    own batch-against-singles discrepancy.  Measured on an MI355X (worst per-parameter relative
    L2 gradient error / relative loss error), dense [3, L] against singles at the parent commit
    -> the padded batch against singles here:
      tiny-lm      2.395e-3 / 0        -> 2.470e-3 / 1.43e-8
      tiny-lm-d80  2.423e-3 / 3.80e-8  -> 2.354e-3 / 7.35e-8
      tiny-mm      2.573e-3 / 6.77e-8  -> 2.691e-3 / 4.46e-8
      tiny-llava   3.095e-3 / 6.80e-8  -> 2.729e-3 / 4.67e-8
    (bounds: 2x the model's own gradient figure; 2x 6.80e-8 for the loss, see LOSS_NOISE)."""
    r = padded_runs(name)
    gtol, ltol = tolerances(name)
    gerr, where = grad_errors(r["model"], r["grad"], r["grad1"])
    lerr = abs(r["loss"] - r["loss1"]) / abs(r["loss1"])
    print(f"{name}: grad err {gerr:.3e} ({where}) tol {gtol:.3e}; loss err {lerr:.3e} tol {ltol:.3e}")
    assert math.isfinite(r["loss"]) and gerr <= gtol and lerr <= ltol


@pytest.mark.parametrize("name", MODELS)
def test_pad_contents_change_no_bit(padded_runs, name):
    """Other pad token ids, and real ids left in the labels under the mask: the same bits."""
    r = padded_runs(name)
    mb, model = r["mb"], r["model"]
    pad = mb["mask"] == 0
    ids = torch.where(pad, torch.full_like(mb["ids"], 5), mb["ids"])
    labels = torch.where(pad, torch.full_like(mb["ids"], 9), mb["labels"])
    model.store.zero_grad()
    loss = run_model(model, ids, labels, mb["pix"], mb["denom"], mb["mask"])
    assert loss == r["loss"] and torch.equal(model.store.grad, r["grad"])


@pytest.mark.parametrize("name", MODELS)
def test_padded_batch_with_checkpointing(padded_runs, name):
    """gradient_checkpointing_enable(): the recompute runs the same kernels on the same
    inputs, so loss and gradients are bitwise the non-checkpointed padded run's (as on the
    dense path)."""
    r = padded_runs(name)
    mb, model = r["mb"], r["model"]
    model.gradient_checkpointing_enable()
    try:
        model.store.zero_grad()
        loss = run_model(model, mb["ids"], mb["labels"], mb["pix"], mb["denom"], mb["mask"])
    finally:
        model.gradient_checkpointing_disable()
    assert loss == r["loss"] and torch.equal(model.store.grad, r["grad"])


def test_padded_batch_from_device_tensors(padded_runs):
    """Batch._from_device: the same bits as the host staging."""
    r = padded_runs("tiny-mm")
    mb, model = r["mb"], r["model"]
    model.store.zero_grad()
    loss = run_model(model, mb["ids"].to(dev), mb["labels"].to(dev), mb["pix"].to(dev), mb["denom"],
                     mb["mask"].to(dev))
    assert loss == r["loss"] and torch.equal(model.store.grad, r["grad"])


@pytest.mark.parametrize("name", ["tiny-mm"])
def test_trainer_step_with_padded_batch(name):
    """One optimizer step fed the padded batch (attention_mask in the loader's dict) against
    the same step fed the three sequences as accumulated micro-batches: loss sum and the
    parameter update within 2x DENSE_NOISE (measured: update error 2.211e-3 against the dense
    figure 2.573e-3, loss sums equal).  Adam's eps is 1 so that the first update,
    lr * g / (|g| + eps), is linear in the gradient for |g| << 1 — with the default 1e-8 it
    is lr * sign(g), which turns noise in a near-zero gradient into a full step."""
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    mb = model_batch(name)

    def trainer():
        return ManualTrainer(StepConfig(model=name, scheduler="constant"),
                             AdamConfig(lr=1e-3, eps=1.0), dev)

    a, b = trainer(), trainer()
    p0 = a.store.master.clone()
    assert torch.equal(p0, b.store.master)
    padded = a.stage({"input_ids": mb["ids"], "labels": mb["labels"], "pixel_values": mb["pix"],
                      "attention_mask": mb["mask"]})
    assert padded.T == sum(mb["lens"]) and padded.num_items == mb["denom"]
    la = a.train_step([padded], mb["denom"]).item()
    mbs = [b.stage({"input_ids": mb["ids"][i:i + 1, :n], "labels": mb["labels"][i:i + 1, :n],
                    "pixel_values": mb["pix"][i:i + 1]}) for i, n in enumerate(mb["lens"])]
    lb = b.train_step(mbs, mb["denom"]).item()
    torch.cuda.synchronize()
    gtol, ltol = tolerances(name)
    da, db = (a.store.master - p0).double(), (b.store.master - p0).double()
    assert float(db.norm()) > 0
    uerr = float((da - db).norm() / db.norm())
    lerr = abs(la - lb) / abs(lb)
    print(f"{name}: update err {uerr:.3e} tol {gtol:.3e}; loss err {lerr:.3e} tol {ltol:.3e}")
    assert uerr <= gtol and lerr <= ltol
