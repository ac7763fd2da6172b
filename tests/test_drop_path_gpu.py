"""ConvNeXt stochastic depth on the GPU: the host keep rule against mmpt_dropout_mask, the
sample-indexed depthwise kernels against the dense ones on the gathered planes (bitwise), the
drop-path residual and its backward against fp32 torch restatements of the rule stated in
include/mmpt.h (bitwise; dgamma within test_layerscale's bound), the argument errors, then the
engine, the trainer and the drop-in module on `tiny-convnext-dp` / `-dp8` against the CPU reference
of tests/drop_path_ref.py with the masks of the host rule.

Engine bars: test_convnext_gpu.py's — every gradient ‖g − g_ref‖/‖g_ref‖ < 3e-2 against the bf16
"cuda"-policy reference, the loss within 1e-4 + 3σ of it (second optimizer step 3e-4 + 3σ), σ =
convnext_oracle.bf16_sigma at the test's own batch size.
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_oracle as CO  # noqa: E402
import drop_path_ref as DR  # noqa: E402
from test_roberta_gpu import same, strided  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
ERR_ARG = "status -1"
U = 2.0 ** -24
P3, P5 = 0.30000001192092896, 0.5  # fp32 values, as the per-block rates are


@pytest.fixture(scope="module")
def K():
    from multimodal_llm_pretraining_amd import kernels

    return kernels


def fbits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32)


def scale(p: float) -> torch.Tensor:
    """s = float(1 / (1 - p)): philox.h dropout_scale, as a 0-dim fp32 device tensor."""
    return torch.tensor(np.float32(1.0 / (1.0 - np.float64(p))), device="cuda")


# ------------------------------------------------------------------ keep rule
@pytest.mark.parametrize("n", [1, 2, 5, 8, 64])
def test_host_keep_rule_is_the_device_rule(K, n):
    from multimodal_llm_pretraining_amd import droppath
    from multimodal_llm_pretraining_amd.engine import VISION_UNIT, dropout_site

    for p in (0.0, 0.10000000149011612, P5, 0.800000011920929):
        for seed, site in ((0, dropout_site(0, 0, VISION_UNIT + 1, 3)),
                           (5, dropout_site(3, 1, VISION_UNIT + 6, 3)), ((1 << 63) + 7, 3)):
            dev = K.dropout_mask(n, p, seed, site).cpu().numpy().astype(bool)
            assert np.array_equal(droppath.keep_mask(n, p, seed, site), dev), (n, p, seed, site)


# ------------------------------------------------------------------ indexed depthwise kernels
IDX_CASES = [((3, 2, 2, 24), (0, 2)), ((4, 7, 7, 192), (1, 3)), ((3, 16, 16, 24), (2,)),
             ((2, 14, 14, 96), (0, 1))]


def idx_id(case):
    return "x".join(map(str, case[0])) + "-" + "_".join(map(str, case[1]))


def idx_operands(shape, idx):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(1000003 * B + 7919 * H + 31 * W + C + len(idx))
    x = (torch.randn(B, H, W, C, generator=g) * 1.5 + 0.25).cuda()
    w = (torch.randn(49, C, generator=g) * 0.2).to(BF16).cuda()
    bias = (torch.randn(C, generator=g) * 0.5).to(BF16).cuda()
    dc = torch.randn(len(idx), H, W, C, generator=g).to(BF16).cuda()
    gr = torch.randn(B, H, W, C, generator=g).cuda()
    return x, w, bias, dc, gr


@pytest.mark.parametrize("case", IDX_CASES, ids=idx_id)
def test_dwconv7_idx_fwd(K, case):
    shape, idx = case
    B, H, W, C = shape
    x, w, bias, _, _ = idx_operands(shape, idx)
    kept = K.KeptSamples(B, idx, "cuda")
    want = torch.full((len(idx), H, W, C), float("nan"), dtype=BF16, device="cuda")
    K.dwconv7_fwd(x[list(idx)].contiguous(), w, bias, want)
    got = torch.full_like(want, float("nan"))
    K.dwconv7_idx_fwd(x, kept, w, bias, got)
    assert not bool(want.isnan().any()) and same(got, want)


@pytest.mark.parametrize("case", IDX_CASES, ids=idx_id)
def test_dwconv7_idx_bwd_input(K, case):
    shape, idx = case
    B, H, W, C = shape
    _, w, _, dc, gr = idx_operands(shape, idx)
    kept = K.KeptSamples(B, idx, "cuda")
    rest = [b for b in range(B) if b not in idx]
    # in place on the stream's gradient: the engine's call
    want = torch.empty(len(idx), H, W, C, device="cuda")
    K.dwconv7_bwd_input(dc, w, want, dx_in=gr[list(idx)].contiguous())
    g = gr.clone()
    K.dwconv7_idx_bwd_input(dc, kept, w, g, dx_in=g)
    assert same(g[list(idx)], want)
    assert same(g[rest], gr[rest])  # the unmapped planes: untouched, bit for bit
    # dx_in = None (zero) into a sentinel-filled buffer
    want0 = torch.empty(len(idx), H, W, C, device="cuda")
    K.dwconv7_bwd_input(dc, w, want0)
    sent = torch.full((B, H, W, C), float("nan"), device="cuda")
    K.dwconv7_idx_bwd_input(dc, kept, w, sent)
    assert same(sent[list(idx)], want0) and bool(sent[rest].isnan().all())
    assert not bool(want0.isnan().any())


@pytest.mark.parametrize("case", IDX_CASES, ids=idx_id)
def test_dwconv7_idx_bwd_weight(K, case):
    shape, idx = case
    B, H, W, C = shape
    x, _, _, dc, _ = idx_operands(shape, idx)
    kept = K.KeptSamples(B, idx, "cuda")
    g = torch.Generator().manual_seed(C)
    dw0, db0 = torch.randn(49, C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
    dw1, db1 = dw0.clone(), db0.clone()
    K.dwconv7_bwd_weight(x[list(idx)].contiguous(), dc, dw1, db1)
    dw2, db2 = dw0.clone(), db0.clone()
    K.dwconv7_idx_bwd_weight(x, kept, dc, dw2, db2)
    assert same(dw2, dw1) and same(db2, db1)
    assert not same(dw1, dw0)


# ------------------------------------------------------------------ the residual and its backward
ADD_CASES = [(1, 1, 8, (0,)), (1, 1, 8, (-1,)), (3, 4, 24, (-1, 0, 1)),
             (4, 49, 192, (0, -1, -1, 1)), (2, 256, 40, (-1, -1))]


def kept_of_slot(K, slot):
    idx = [b for b, s in enumerate(slot) if s >= 0]
    assert [slot[b] for b in idx] == list(range(len(idx)))
    kept = K.KeptSamples(len(slot), idx, "cuda")
    assert kept.slot_dev.cpu().tolist() == list(slot)
    return kept, idx


@pytest.mark.parametrize("B,rows,C,slot", ADD_CASES,
                         ids=[f"{b}x{r}x{c}-" + "_".join(map(str, s)) for b, r, c, s in ADD_CASES])
def test_droppath_add_fwd(K, B, rows, C, slot):
    kept, idx = kept_of_slot(K, slot)
    g = torch.Generator().manual_seed(131 * rows + C + B)
    resid = torch.randn(B, rows, C, generator=g).cuda()
    gamma = (torch.rand(C, generator=g) + 0.5).cuda()
    y = strided(torch.randn(len(idx) * rows, C, generator=g).to(BF16).cuda(), 24) if idx else None
    for p in (P3, P5):
        # the stated rule: gamma * f32(y) rounded, times s rounded, plus the residual rounded
        want = resid.clone()
        if idx:
            branch = (gamma * y.float()) * scale(p)
            want[idx] = resid[idx] + branch.view(len(idx), rows, C)
        out = torch.full_like(resid, float("nan"))
        K.droppath_add_fwd(resid, gamma, y, kept, p, out)
        assert same(out, want), p
        al = resid.clone()
        K.droppath_add_fwd(al, gamma, y, kept, p, al)
        assert same(al, want), p
    if idx:  # the factor is there: p = 0 is the plain layer-scale residual on the kept planes
        out0 = torch.empty_like(resid)
        K.droppath_add_fwd(resid, gamma, y, kept, 0.0, out0)
        assert not same(out0, want)
        assert same(out0[idx], resid[idx] + (gamma * y.float()).view(len(idx), rows, C))


@pytest.mark.parametrize("B,rows,C,idx", [(1, 1, 8, (0,)), (3, 4, 24, (1, 2)),
                                          (4, 49, 192, (0, 3)), (3, 171, 40, (0, 1, 2))])
def test_droppath_bwd(K, B, rows, C, idx):
    kept = K.KeptSamples(B, idx, "cuda")
    Rk = len(idx) * rows
    g = torch.Generator().manual_seed(977 * rows + C + B)
    gr = torch.randn(B, rows, C, generator=g).cuda()
    gamma = (torch.rand(C, generator=g) + 0.5).cuda()
    y = strided(torch.randn(Rk, C, generator=g).to(BF16).cuda(), 24)
    start = torch.randn(C, generator=g).cuda()
    p = P3

    def run():
        dy = strided(torch.full((Rk, C), float("nan"), dtype=BF16, device="cuda"), 8)
        dg = start.clone()
        K.droppath_bwd(gr, kept, gamma, y, p, dy, dg)
        return dy, dg

    dy, dg = run()
    gp = (gr[list(idx)] * scale(p)).view(Rk, C)  # g' = g*s rounded to fp32
    assert same(dy, (gamma * gp).to(BF16))
    # test_layerscale's bound on mmpt_layerscale_bwd's dgamma, over the kept rows with g' for g
    terms = gp.double().cpu() * y.double().cpu()
    ref = start.double().cpu() + terms.sum(0)
    a = start.double().cpu().abs() + terms.abs().sum(0)
    err = (dg.double().cpu() - ref).abs()
    assert bool((err <= (Rk + 1) * U * a).all()), (err / a).max()
    dy2, dg2 = run()
    assert same(dy2, dy) and same(dg2, dg)
    # the same rows through mmpt_layerscale_bwd on the gathered, scaled gradient: the same bits
    dy3 = torch.empty(Rk, C, dtype=BF16, device="cuda")
    dg3 = start.clone()
    K.layerscale_bwd(gp.contiguous(), gamma, y, dy3, dg3)
    assert same(dy3, dy) and same(dg3, dg)


# ------------------------------------------------------------------ argument errors
def test_drop_path_argument_errors(K):
    from multimodal_llm_pretraining_amd import _lib

    st = torch.cuda.current_stream().cuda_stream
    nan = float("nan")
    B, H, C = 3, 4, 16
    x = torch.randn(B, H, H, C, device="cuda")
    w, b = torch.zeros(49, C, dtype=BF16, device="cuda"), torch.zeros(C, dtype=BF16, device="cuda")
    c = torch.full((2, H, H, C), nan, dtype=BF16, device="cuda")
    g = torch.full((B, H, H, C), nan, device="cuda")
    dw, db = torch.full((49, C), nan, device="cuda"), torch.full((C,), nan, device="cuda")
    gamma = torch.ones(C, device="cuda")
    dgam = torch.full((C,), nan, device="cuda")
    out = torch.full((B, H * H, C), nan, device="cuda")
    good = K.KeptSamples(B, (0, 2), "cuda")
    ws = torch.zeros(1 << 16, device="cuda")
    # the wrappers check the host copy of idx: increasing, in range, over this stream's planes
    for idx in ((2, 0), (0, 0), (0, 3), (-1, 1)):
        bad = K.KeptSamples(B, idx, "cuda")
        with pytest.raises(ValueError, match="strictly increasing"):
            K.dwconv7_idx_fwd(x, bad, w, b, c)
        with pytest.raises(ValueError, match="strictly increasing"):
            K.dwconv7_idx_bwd_input(c, bad, w, g)
        with pytest.raises(ValueError, match="strictly increasing"):
            K.dwconv7_idx_bwd_weight(x, bad, c, dw, db)
        with pytest.raises(ValueError, match="strictly increasing"):
            K.droppath_add_fwd(x.view(B, H * H, C), gamma, c.view(-1, C), bad, P3, out)
        with pytest.raises(ValueError, match="strictly increasing"):
            K.droppath_bwd(x.view(B, H * H, C), bad, gamma, c.view(-1, C), P3, c.view(-1, C), dgam)
    with pytest.raises(ValueError, match="planes"):
        K.dwconv7_idx_fwd(x, K.KeptSamples(B + 1, (0, 2), "cuda"), w, b, c)
    with pytest.raises(ValueError, match="no kept sample"):
        K.dwconv7_idx_fwd(x, K.KeptSamples(B, (), "cuda"), w, b, c[:0])
    for p in (-0.1, 1.0):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            K.droppath_add_fwd(x.view(B, H * H, C), gamma, c.view(-1, C), good, p, out)
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            K.droppath_bwd(x.view(B, H * H, C), good, gamma, c.view(-1, C), p, c.view(-1, C), dgam)
    # the entries themselves: Bk outside [1, B], p outside [0, 1)
    ip, sp = good.idx_dev.data_ptr(), good.slot_dev.data_ptr()
    for Bk in (0, B + 1):
        with pytest.raises(RuntimeError, match=ERR_ARG):
            _lib.call("mmpt_dwconv7_idx_fwd", B, Bk, H, H, C, x.data_ptr(), ip, w.data_ptr(),
                      b.data_ptr(), c.data_ptr(), st)
        with pytest.raises(RuntimeError, match=ERR_ARG):
            _lib.call("mmpt_dwconv7_idx_bwd_input", B, Bk, H, H, C, c.data_ptr(), ip, w.data_ptr(),
                      None, g.data_ptr(), st)
        with pytest.raises(RuntimeError, match=ERR_ARG):
            _lib.call("mmpt_dwconv7_idx_bwd_weight", B, Bk, H, H, C, x.data_ptr(), ip,
                      c.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), st)
        with pytest.raises(RuntimeError, match=ERR_ARG):
            _lib.call("mmpt_droppath_bwd", B, Bk, H * H, C, x.data_ptr(), ip, gamma.data_ptr(),
                      c.data_ptr(), C, P3, c.data_ptr(), C, dgam.data_ptr(), ws.data_ptr(), st)
    with pytest.raises(RuntimeError, match=ERR_ARG):
        _lib.call("mmpt_droppath_add_fwd", B, B + 1, H * H, C, x.data_ptr(), gamma.data_ptr(),
                  c.data_ptr(), C, sp, P3, out.data_ptr(), st)
    for p in (-0.1, 1.0):
        with pytest.raises(RuntimeError, match=ERR_ARG):
            _lib.call("mmpt_droppath_add_fwd", B, 2, H * H, C, x.data_ptr(), gamma.data_ptr(),
                      c.data_ptr(), C, sp, p, out.data_ptr(), st)
        with pytest.raises(RuntimeError, match=ERR_ARG):
            _lib.call("mmpt_droppath_bwd", B, 2, H * H, C, x.data_ptr(), ip, gamma.data_ptr(),
                      c.data_ptr(), C, p, c.data_ptr(), C, dgam.data_ptr(), ws.data_ptr(), st)
    # C % 8 != 0
    x12 = torch.randn(B, H, H, 12, device="cuda")
    w12, b12 = torch.zeros(49, 12, dtype=BF16, device="cuda"), torch.zeros(12, dtype=BF16, device="cuda")
    c12 = torch.full((2, H, H, 12), nan, dtype=BF16, device="cuda")
    o12 = torch.full((B, H * H, 12), nan, device="cuda")
    with pytest.raises(RuntimeError, match=ERR_ARG):
        K.dwconv7_idx_fwd(x12, good, w12, b12, c12)
    with pytest.raises(RuntimeError, match=ERR_ARG):
        K.dwconv7_idx_bwd_weight(x12, good, c12, torch.zeros(49, 12, device="cuda"),
                                 torch.zeros(12, device="cuda"))
    with pytest.raises(RuntimeError, match=ERR_ARG):
        K.droppath_add_fwd(x12.view(B, H * H, 12), torch.ones(12, device="cuda"), c12.view(-1, 12),
                           good, P3, o12)

    # misaligned pointers: a dense view that starts one element into its buffer
    def off(shape, dtype):
        n = int(np.prod(shape))
        return torch.zeros(n + 8, dtype=dtype, device="cuda")[1:1 + n].view(shape)

    with pytest.raises(RuntimeError, match=ERR_ARG):
        K.dwconv7_idx_fwd(off(x.shape, F32), good, w, b, c)
    with pytest.raises(RuntimeError, match=ERR_ARG):
        K.dwconv7_idx_fwd(x, good, w, b, off(c.shape, BF16))
    with pytest.raises(RuntimeError, match=ERR_ARG):
        K.dwconv7_idx_bwd_input(off(c.shape, BF16), good, w, g)
    with pytest.raises(RuntimeError, match=ERR_ARG):
        K.dwconv7_idx_bwd_weight(x, good, c, off((49, C), F32), db)
    with pytest.raises(RuntimeError, match=ERR_ARG):
        K.droppath_add_fwd(off((B, H * H, C), F32), gamma, c.view(-1, C), good, P3, out)
    with pytest.raises(RuntimeError, match=ERR_ARG):
        K.droppath_bwd(x.view(B, H * H, C), good, gamma, c.view(-1, C), P3, c.view(-1, C),
                       off((C,), F32))
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its sentinel
    for t in (c, g, dw, db, dgam, out, c12, o12):
        assert bool(t.isnan().all())


# ------------------------------------------------------------------ engine
def masks(cfg, B, seed, step):
    """keep[j]: block j's keep bits from the host rule at (seed, micro-step `step`, rank 0)."""
    from multimodal_llm_pretraining_amd import droppath
    from multimodal_llm_pretraining_amd.engine import VISION_UNIT, dropout_site

    return [droppath.keep_mask(B, p, seed, dropout_site(step, 0, VISION_UNIT + 1 + j, 3)).tolist()
            for j, p in enumerate(cfg.convnext.drop_path_rates())]


def engine_for(cfg, P, seed=0, checkpointing=False):
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.engine import Engine
    from multimodal_llm_pretraining_amd.params import ParamStore

    store = ParamStore(C.param_shapes(cfg), "cuda")
    store.load(P)
    store.refresh_shadow()
    eng = Engine(cfg, store)
    eng.checkpointing = checkpointing
    eng.dropout_seed = seed
    return store, eng


def run(cfg, P, batch, steps=1, enabled=True, **kw):
    """([loss per micro-step], the store with the flat grads of the last one, the micro-step
    counter each forward ran at)."""
    from multimodal_llm_pretraining_amd.engine import Batch

    store, eng = engine_for(cfg, P, **kw)
    eng.dropout_enabled = enabled
    assert eng.rank == 0
    b = Batch(cfg, None, batch["labels"], batch["pixel_values"], store.device)
    losses, at = [], []
    for _ in range(steps):
        store.zero_grad()
        at.append(eng.dropout_step)
        s = eng.forward(b, 1.0 / b.num_items)
        eng.backward(b)
        losses.append(s.item() / b.num_items)
    assert eng.cache == {}
    return losses, store, at


def check_grads(store, G):
    worst = (0.0, None)
    for k, r in G.items():
        g = store.g(k).cpu()
        err = ((g - r).norm() / (r.norm() + 1e-20)).item()
        worst = max(worst, (err, k))
        assert err < 3e-2, (k, err)
    return worst


@pytest.fixture(scope="module")
def ref():
    """Seed-0 weights (gamma ~ U(0.5, 1.5)) and one B = 8 batch, shared and left unchanged; σ at
    this shape."""
    from multimodal_llm_pretraining_amd import config as C

    cfg = C.get_config("tiny-convnext-dp")
    P = CO.init_params(cfg, seed=0)
    batch = CO.make_batch(cfg, 8, seed=1)
    sigma = CO.bf16_sigma(P, cfg, 8)
    return dict(cfg=cfg, base=C.get_config("tiny-convnext"), P=P, batch=batch, sigma=sigma)


def test_engine_against_the_reference(ref):
    cfg, P, bd, sigma = ref["cfg"], ref["P"], ref["batch"], ref["sigma"]
    B = 8
    (loss,), store, (step,) = run(cfg, P, bd)
    keep = masks(cfg, B, 0, step)
    counts = [sum(k) for k in keep]
    if step == 0:
        assert counts == [8, 6, 5, 3, 3, 4]
    assert counts[0] == B and sum(0 < n < B for n in counts) >= 3, counts
    loss16, G = DR.loss_and_grads(P, cfg, bd, keep, "bf16")
    dense16 = CO.forward_loss(P, cfg, bd, "bf16").item()
    worst = max((((store.g(k).cpu() - r).norm() / (r.norm() + 1e-20)).item(), k)
                for k, r in G.items())
    print(f"tiny-convnext-dp B={B} kept {counts}: GPU {loss:.7f}, bf16 reference {loss16:.7f} "
          f"(no drop path {dense16:.7f}), sigma {sigma:.3e}, worst gradient error {worst}")
    assert abs(loss16 - dense16) > 1e-3  # the masks matter at this tolerance
    assert abs(loss - loss16) < 1e-4 + 3 * sigma, (loss, loss16, sigma)
    check_grads(store, G)


def test_whole_blocks_dropped_and_kept(ref):
    """tiny-convnext-dp8 at B = 2: a seed where one block keeps nobody (identity, its parameter
    gradients exactly zero) and another block with p > 0 keeps everybody (the compact path with
    the identity map)."""
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg, P = C.get_config("tiny-convnext-dp8"), ref["P"]
    B = 2
    bd = CO.make_batch(cfg, B, seed=1)
    pr = cfg.convnext.drop_path_rates()
    store, eng = engine_for(cfg, P)
    step = eng.dropout_step

    def qualifies(s):
        counts = [sum(k) for k in masks(cfg, B, s, step)]
        return any(n == 0 for n in counts) and any(n == B and p > 0 for n, p in zip(counts, pr))

    seed = next((s for s in range(64) if qualifies(s)), None)
    assert seed is not None
    if step == 0:
        assert qualifies(5) and [sum(k) for k in masks(cfg, B, 5, 0)] == [2, 1, 2, 2, 1, 0]
        assert qualifies(6) and [sum(k) for k in masks(cfg, B, 6, 0)] == [2, 1, 2, 0, 0, 0]
    keep = masks(cfg, B, seed, step)
    eng.dropout_seed = seed
    seen = []
    eng.grad_ready_hook = lambda lo, hi: seen.append((lo, hi))
    b = Batch(cfg, None, bd["labels"], bd["pixel_values"], store.device)
    store.zero_grad()
    loss = eng.forward(b, 1.0 / B).item() / B
    eng.backward(b)
    torch.cuda.synchronize()
    assert eng.cache == {}
    sigma = CO.bf16_sigma(P, cfg, B)
    loss16, G = DR.loss_and_grads(P, cfg, bd, keep, "bf16")
    print(f"tiny-convnext-dp8 B={B} seed {seed} kept {[sum(k) for k in keep]}: GPU {loss:.7f}, "
          f"bf16 reference {loss16:.7f}, sigma {sigma:.3e}")
    assert abs(loss - loss16) < 1e-4 + 3 * sigma, (loss, loss16, sigma)
    check_grads(store, G)
    names = [f"convnext.stages.{s}.layers.{j}." for s, d in enumerate(cfg.convnext.depths)
             for j in range(d)]
    dropped = [n for n, k in zip(names, keep) if sum(k) == 0]
    assert dropped
    for n in store.offsets:
        if n.startswith(tuple(dropped)):
            assert int(store.g(n).count_nonzero()) == 0, n
            assert int(G[n].count_nonzero()) == 0, n
    # the hook: every parameter announced, none twice (the fully dropped block's included)
    assert seen
    seen.sort()
    for (_, hi), (lo, _) in zip(seen, seen[1:]):
        assert hi <= lo, seen
    for name, off in store.offsets.items():
        n = store.g(name).numel()
        assert any(lo <= off and off + n <= hi for lo, hi in seen), name


def test_stage_checkpointing_is_bitwise(ref):
    cfg, P, bd = ref["cfg"], ref["P"], ref["batch"]
    la, a, at = run(cfg, P, bd, steps=2)
    lb, b, bt = run(cfg, P, bd, steps=2, checkpointing=True)
    assert at == bt and at[1] == at[0] + 1  # one mask counter tick per micro-step
    assert la == lb and torch.equal(fbits(a.grad), fbits(b.grad))
    assert masks(cfg, 8, 0, at[0]) != masks(cfg, 8, 0, at[1])
    assert la[0] != la[1]  # other masks: the same micro-batch gives another loss


def count_indexed_calls(K, monkeypatch):
    calls = []
    for fn in ("dwconv7_idx_fwd", "dwconv7_idx_bwd_input", "dwconv7_idx_bwd_weight",
               "droppath_add_fwd", "droppath_bwd"):
        real = getattr(K, fn)

        def spy(*a, _real=real, _fn=fn, **kw):
            calls.append(_fn)
            return _real(*a, **kw)

        monkeypatch.setattr(K, fn, spy)
    return calls


def test_eval_and_rate_zero_take_the_dense_path(K, ref, monkeypatch):
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.engine import Batch
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining

    cfg, base, P, bd = ref["cfg"], ref["base"], ref["P"], ref["batch"]
    calls = count_indexed_calls(K, monkeypatch)
    (want,), dense, _ = run(base, P, bd)
    assert calls == []
    # rate 0 through with_drop_path: today's calls, today's bits
    zero = C.with_drop_path(cfg, 0.0)
    assert zero == base
    (l0,), s0, _ = run(zero, P, bd)
    assert calls == [] and l0 == want and torch.equal(fbits(s0.grad), fbits(dense.grad))
    # dropout_enabled = False: the dense step, and the mask counter stays
    (l1,), s1, _ = run(cfg, P, bd, enabled=False)
    assert calls == [] and l1 == want and torch.equal(fbits(s1.grad), fbits(dense.grad))
    # a forward without gradients is dense too, and leaves the counter alone
    store, eng = engine_for(cfg, P)
    b = Batch(cfg, None, bd["labels"], bd["pixel_values"], store.device)
    ev = eng.forward(b, 1.0 / 8, need_grad=False).item() / 8
    bstore, beng = engine_for(base, P)
    bev = beng.forward(Batch(base, None, bd["labels"], bd["pixel_values"], bstore.device), 1.0 / 8,
                       need_grad=False).item() / 8
    assert calls == [] and ev == bev and eng.dropout_step == 0 and eng.cache == {}
    assert ev == pytest.approx(want, abs=1e-6)
    # the drop-in module in eval(): tiny-convnext's forward, bit for bit
    m = MMPTForPretraining(cfg)
    m.store.load(P)
    m.store.refresh_shadow()
    m.eval()
    with torch.no_grad():
        got = m(pixel_values=bd["pixel_values"], labels=bd["labels"]).loss.item()
    mb = MMPTForPretraining(base)
    mb.store.load(P)
    mb.store.refresh_shadow()
    mb.eval()
    with torch.no_grad():
        plain = mb(pixel_values=bd["pixel_values"], labels=bd["labels"]).loss.item()
    assert calls == [] and got == plain
    # and the training step does take the indexed entries
    (l2,), _, _ = run(cfg, P, bd)
    assert {"dwconv7_idx_fwd", "dwconv7_idx_bwd_input", "dwconv7_idx_bwd_weight",
            "droppath_add_fwd", "droppath_bwd"} <= set(calls) and l2 != want


def test_two_adamw_steps(ref):
    """Two AdamW steps through trainer.ManualTrainer against the reference with each step's masks
    plus torch.optim.AdamW: test_convnext_gpu.py::test_two_adamw_steps' bounds."""
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    cfg, P, sigma = ref["cfg"], ref["P"], ref["sigma"]
    B = 8
    batches = [ref["batch"], CO.make_batch(cfg, B, seed=2)]
    lrs = CO.cosine_lrs(1e-3, 0, 4, 2)
    tr = ManualTrainer(StepConfig(model="tiny-convnext-dp", scheduler="cosine", num_warmup_steps=0,
                                  num_training_steps=4),
                       AdamConfig(lr=1e-3, weight_decay=0.05, adamw=True, max_grad_norm=0.0), "cuda")
    tr.store.load(P)
    tr.store.refresh_shadow()
    got, keeps = [], []
    for bd in batches:
        b = tr.stage(bd)
        keeps.append(masks(cfg, B, tr.engine.dropout_seed, tr.engine.dropout_step))
        got.append(tr.train_step([b], b.num_items).item() / b.num_items)
    assert keeps[0] != keeps[1] and tr.engine.dropout_step == 2
    want, _ = DR.train_steps(P, cfg, batches, keeps, lrs, "bf16")
    print(f"two AdamW steps: GPU {got}, bf16 reference {want}, sigma {sigma:.3e}")
    assert abs(got[0] - want[0]) < 1e-4 + 3 * sigma, (got, want, sigma)
    assert abs(got[1] - want[1]) < 3e-4 + 3 * sigma, (got, want, sigma)
    assert got[1] != got[0]
    C_ = cfg.num_classes
    assert int(tr.store.p("cls_head.weight")[C_:].count_nonzero()) == 0
    assert int(tr.store.p("cls_head.bias")[C_:].count_nonzero()) == 0


def test_dropin_module_trains_with_drop_path(ref):
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining

    cfg, P, bd, sigma = ref["cfg"], ref["P"], ref["batch"], ref["sigma"]
    m = MMPTForPretraining(cfg)
    m.store.load(P)
    m.store.refresh_shadow()
    m.train()
    m.set_dropout_seed(0)
    step = m.engine.dropout_step
    out = m(pixel_values=bd["pixel_values"], labels=bd["labels"])
    out.loss.backward()
    assert m.engine.cache == {} and m.engine.dropout_step == step + 1
    keep = masks(cfg, 8, 0, step)
    loss16, G = DR.loss_and_grads(P, cfg, bd, keep, "bf16")
    assert abs(out.loss.item() - loss16) < 1e-4 + 3 * sigma, (out.loss.item(), loss16, sigma)
    for name, p in m.named_parameters():
        assert p.grad is not None and p.grad.data_ptr() == m.store.g(name).data_ptr(), name
    check_grads(m.store, G)
    (loss,), eng_store, _ = run(cfg, P, bd)
    if step == 0:  # the engine's own first micro-step drew the same masks
        assert out.loss.item() == pytest.approx(loss, abs=1e-6)
        assert torch.equal(fbits(m.store.grad), fbits(eng_store.grad))
