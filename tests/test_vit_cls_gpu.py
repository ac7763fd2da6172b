"""The vision-only classifier on the GPU: the K18 head kernels against the LayerNorm entries
on a dense copy of the CLS rows (bitwise), then the engine, the trainer and the drop-in module
on `tiny-vit-cls` against the CPU oracle of tests/vit_cls_oracle.py.

Bars.  Gradients: ‖g − g_ref‖/‖g_ref‖ < 3e-2 per tensor against the bf16 oracle
(tests/test_parity_gpu.py's bar).  Loss: the loss averages B = 8 rows, so the distance between
two valid bf16 implementations is measured, not assumed: σ = the standard deviation of
(bf16 oracle − fp32 oracle) over 8 batch seeds at the test's own shape, on the CPU; the GPU
loss must lie within 1e-4 + 3σ of the bf16 oracle (second optimizer step: 3e-4 + 3σ).
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vit_cls_oracle as VO  # noqa: E402
from test_dropout_gpu import Masks  # noqa: E402

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
B = 8  # images of the parity batches (σ is measured at this shape)
ERR_ARG = "status -1"


@pytest.fixture(scope="module")
def K():
    from multimodal_llm_pretraining_amd import kernels

    return kernels


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


# ------------------------------------------------------------------ kernels
def _case(batch, tokens, h, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * batch + 10 * tokens + h)
    x = (torch.randn(batch * tokens, h, generator=g) * 2 + 0.5).cuda()
    w = (1 + 0.1 * torch.randn(h, generator=g)).cuda()
    b = (0.1 * torch.randn(h, generator=g)).cuda()
    dy = torch.randn(batch, h, generator=g).to(BF16).cuda()
    acc = [torch.randn(h, generator=g).cuda() for _ in range(3)]  # dw, db, dsum start values
    return x, w, b, dy, acc


def _cls_rows(t, batch, tokens):
    return t.view(batch, tokens, -1)[:, 0].contiguous()


SHAPES = [(b, t, h) for b in (1, 3, 65) for t in (1, 2, 17, 197) for h in (72, 128, 1024)]
# widths that reach MAXJ = 2, 12, 16 / PT = 2, 4, masked lanes in the last vector (520), and more
# CLS rows than backward workgroups (1029)
SHAPES += [(5, 2, 512), (5, 2, 520), (129, 2, 3072), (5, 2, 4096), (1029, 2, 64)]


@pytest.mark.parametrize("batch,tokens,h", SHAPES)
def test_cls_ln_fwd_is_layernorm_on_the_cls_rows(K, batch, tokens, h):
    x, w, b, _, _ = _case(batch, tokens, h)
    eps = 1e-12
    xc = _cls_rows(x, batch, tokens)
    y0 = torch.empty(batch, h, dtype=BF16, device="cuda")
    m0, r0 = torch.empty(batch, device="cuda"), torch.empty(batch, device="cuda")
    K.layernorm_fwd(xc, w, b, eps, y0, m0, r0)
    y = torch.full((batch, h), 7.0, dtype=BF16, device="cuda")
    m, r = torch.empty(batch, device="cuda"), torch.empty(batch, device="cuda")
    K.cls_ln_fwd(x, batch, tokens, w, b, eps, y, m, r)
    assert torch.equal(bits(y), bits(y0))
    assert torch.equal(bits(m), bits(m0)) and torch.equal(bits(r), bits(r0))
    ref = torch.nn.functional.layer_norm(xc.cpu(), (h,), w.cpu(), b.cpu(), eps)
    assert (y.cpu().float() - ref).abs().max() < 0.05  # and it is a LayerNorm


def test_cls_ln_fwd_row_stride(K):
    """ld_y > h: the rows land ld_y apart and the columns past h are left alone."""
    batch, tokens, h = 3, 17, 128
    x, w, b, _, _ = _case(batch, tokens, h)
    y0 = torch.empty(batch, h, dtype=BF16, device="cuda")
    m, r = torch.empty(batch, device="cuda"), torch.empty(batch, device="cuda")
    K.cls_ln_fwd(x, batch, tokens, w, b, 1e-5, y0, m, r)
    wide = torch.full((batch, h + 24), 7.0, dtype=BF16, device="cuda")
    K.cls_ln_fwd(x, batch, tokens, w, b, 1e-5, wide[:, :h], m, r)
    assert torch.equal(bits(wide[:, :h]), bits(y0)) and bool((wide[:, h:] == 7.0).all())


def _bwd_reference(K, x, w, b, dy, acc, batch, tokens, want_bf16=True, want_dsum=True):
    h = x.shape[1]
    xc = _cls_rows(x, batch, tokens)
    y = torch.empty(batch, h, dtype=BF16, device="cuda")
    m, r = torch.empty(batch, device="cuda"), torch.empty(batch, device="cuda")
    K.layernorm_fwd(xc, w, b, 1e-12, y, m, r)
    dx = torch.empty(batch, h, device="cuda")
    dxb = torch.empty(batch, h, dtype=BF16, device="cuda") if want_bf16 else None
    dw, db, ds = (a.clone() for a in acc)
    K.layernorm_bwd(xc, m, r, dy, w, dx, dw, db, dx_bf16=dxb, dsum=ds if want_dsum else None)
    return m, r, dx, dxb, dw, db, ds


@pytest.mark.parametrize("batch,tokens,h", SHAPES)
def test_cls_ln_bwd_is_layernorm_bwd_plus_zero_rows(K, batch, tokens, h):
    x, w, b, dy, acc = _case(batch, tokens, h)
    m, r, dx0, dxb0, dw0, db0, ds0 = _bwd_reference(K, x, w, b, dy, acc, batch, tokens)
    dx = torch.full((batch * tokens, h), float("nan"), device="cuda")
    dxb = torch.full((batch * tokens, h), float("nan"), dtype=BF16, device="cuda")
    dw, db, ds = (a.clone() for a in acc)
    K.cls_ln_bwd(x, batch, tokens, m, r, dy, w, dx, dxb, dw, db, dsum=ds)
    # the CLS rows and the three accumulated vectors: the bits of mmpt_layernorm_bwd_ex
    assert torch.equal(bits(_cls_rows(dx, batch, tokens)), bits(dx0))
    assert torch.equal(bits(_cls_rows(dxb, batch, tokens)), bits(dxb0))
    assert torch.equal(bits(dw), bits(dw0)) and torch.equal(bits(db), bits(db0))
    assert torch.equal(bits(ds), bits(ds0))
    assert not torch.equal(bits(dw), bits(acc[0]))  # (and they did accumulate something)
    # every other row: the bit pattern of +0 in both outputs
    rest = bits(dx).view(batch, tokens, h)[:, 1:]
    restb = bits(dxb).view(batch, tokens, h)[:, 1:]
    assert rest.numel() == batch * (tokens - 1) * h
    assert int(rest.count_nonzero()) == 0 and int(restb.count_nonzero()) == 0


@pytest.mark.parametrize("batch,tokens,h", [(3, 17, 128), (65, 2, 1024), (1, 197, 72)])
def test_cls_ln_bwd_nulls(K, batch, tokens, h):
    """dx_bf16 = NULL and dsum = NULL, dw / db = NULL: the other outputs keep their bits."""
    x, w, b, dy, acc = _case(batch, tokens, h)
    m, r, dx0, dxb0, dw0, db0, _ = _bwd_reference(K, x, w, b, dy, acc, batch, tokens)
    dx = torch.full((batch * tokens, h), float("nan"), device="cuda")
    dw, db = acc[0].clone(), acc[1].clone()
    K.cls_ln_bwd(x, batch, tokens, m, r, dy, w, dx, None, dw, db)
    assert torch.equal(bits(_cls_rows(dx, batch, tokens)), bits(dx0))
    assert int(bits(dx).view(batch, tokens, h)[:, 1:].count_nonzero()) == 0
    assert torch.equal(bits(dw), bits(dw0)) and torch.equal(bits(db), bits(db0))
    dx.fill_(float("nan"))
    dxb = torch.full((batch * tokens, h), float("nan"), dtype=BF16, device="cuda")
    K.cls_ln_bwd(x, batch, tokens, m, r, dy, w, dx, dxb)  # no parameter gradients, no dsum
    assert torch.equal(bits(_cls_rows(dx, batch, tokens)), bits(dx0))
    assert torch.equal(bits(_cls_rows(dxb, batch, tokens)), bits(dxb0))
    assert int(bits(dxb).view(batch, tokens, h)[:, 1:].count_nonzero()) == 0


def test_cls_ln_bwd_dy_row_stride(K):
    batch, tokens, h = 3, 17, 128
    x, w, b, dy, acc = _case(batch, tokens, h)
    m, r, dx0, _, dw0, _, _ = _bwd_reference(K, x, w, b, dy, acc, batch, tokens)
    wide = torch.full((batch, h + 8), float("nan"), dtype=BF16, device="cuda")
    wide[:, :h] = dy
    dx = torch.empty(batch * tokens, h, device="cuda")
    dw = acc[0].clone()
    K.cls_ln_bwd(x, batch, tokens, m, r, wide[:, :h], w, dx, None, dw, acc[1].clone())
    assert torch.equal(bits(_cls_rows(dx, batch, tokens)), bits(dx0))
    assert torch.equal(bits(dw), bits(dw0))


def test_cls_ln_argument_errors():
    from multimodal_llm_pretraining_amd import _lib
    from multimodal_llm_pretraining_amd import kernels as K

    batch, tokens = 2, 3

    def bufs(h):
        f = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
        return dict(x=f(batch * tokens * h + 4), w=f(h + 4), b=f(h), m=f(batch), r=f(batch),
                    y=torch.zeros(batch * (h + 8) + 8, dtype=BF16, device="cuda"),
                    dx=f(batch * tokens * h + 4),
                    dxb=torch.zeros(batch * tokens * h + 8, dtype=BF16, device="cuda"),
                    dw=f(h), db=f(h), ds=f(h),
                    ws=K.workspace(_lib.query("mmpt_cls_ln_bwd_workspace_bytes", batch, h), slot=2))

    def fwd(h, x=None, y=None, ld_y=None):
        t = bufs(h)
        _lib.call("mmpt_cls_ln_fwd", batch, tokens, h, 1e-5, x or t["x"].data_ptr(),
                  t["w"].data_ptr(), t["b"].data_ptr(), y or t["y"].data_ptr(),
                  h if ld_y is None else ld_y, t["m"].data_ptr(), t["r"].data_ptr(), 0)

    def bwd(h, x=None, dx=None, dxb="yes", ds=None, ld_dy=None):
        t = bufs(h)
        _lib.call("mmpt_cls_ln_bwd", batch, tokens, h, x or t["x"].data_ptr(), t["m"].data_ptr(),
                  t["r"].data_ptr(), t["y"].data_ptr(), h if ld_dy is None else ld_dy,
                  t["w"].data_ptr(), dx or t["dx"].data_ptr(),
                  t["dxb"].data_ptr() if dxb == "yes" else dxb, t["dw"].data_ptr(),
                  t["db"].data_ptr(), ds, t["ws"].data_ptr(), 0)

    fwd(16), bwd(16)  # the well-formed calls pass
    torch.cuda.synchronize()
    t = bufs(16)
    for call in (lambda: fwd(12), lambda: bwd(12),                       # h % 8 != 0
                 lambda: fwd(16, x=t["x"].data_ptr() + 4),               # misaligned pointers
                 lambda: fwd(16, y=t["y"].data_ptr() + 2),
                 lambda: bwd(16, dx=t["dx"].data_ptr() + 4),
                 lambda: bwd(16, dxb=t["dxb"].data_ptr() + 2),
                 lambda: fwd(16, ld_y=8), lambda: bwd(16, ld_dy=8),      # ld < h
                 lambda: bwd(16, dxb=None, ds=t["ds"].data_ptr())):      # dsum without dx_bf16
        with pytest.raises(RuntimeError, match=ERR_ARG):
            call()


# ------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def ref():
    """The oracle side, computed once: seed-0 weights (non-zero biases), one B = 8 batch, the
    bf16 loss and gradients, the fp32 loss and σ at this shape."""
    from multimodal_llm_pretraining_amd import config as C

    cfg = C.get_config("tiny-vit-cls")
    P = VO.init_params(cfg, seed=0)
    batch = VO.make_batch(cfg, B, seed=1)
    loss16, G = VO.loss_and_grads(P, cfg, batch, "bf16")
    with torch.no_grad():
        loss32 = VO.forward_loss(P, cfg, batch, "fp32").item()
    sigma = VO.bf16_sigma(P, cfg, B)
    print(f"tiny-vit-cls B={B}: bf16 {loss16:.7f} fp32 {loss32:.7f} sigma {sigma:.3e}")
    return dict(cfg=cfg, P=P, batch=batch, loss16=loss16, loss32=loss32, G=G, sigma=sigma)


def engine_for(cfg, P, seed=1234, checkpointing=False):
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.engine import Engine
    from multimodal_llm_pretraining_amd.params import ParamStore

    store = ParamStore(C.param_shapes(cfg), "cuda")
    store.load(P)
    store.refresh_shadow()
    eng = Engine(cfg, store)
    eng.dropout_seed, eng.checkpointing = seed, checkpointing
    return store, eng


def run(cfg, P, batch, steps=1, scale=None, **kw):
    """([loss per micro-step], flat grads after the last one — zeroed between the steps)."""
    from multimodal_llm_pretraining_amd.engine import Batch

    store, eng = engine_for(cfg, P, **kw)
    b = Batch(cfg, None, batch["labels"], batch["pixel_values"], store.device)
    losses = []
    for _ in range(steps):
        store.zero_grad()
        s = eng.forward(b, (1.0 / b.num_items) if scale is None else scale)
        eng.backward(b)
        losses.append(s.item() / b.num_items)
    assert eng.cache == {}
    return losses, store


def check_grads(store, G, cfg):
    for k, r in G.items():
        g = store.g(k).cpu()
        err = ((g - r).norm() / (r.norm() + 1e-20)).item()
        assert err < 3e-2, (k, err)
    C_ = cfg.num_classes
    assert int(store.g("cls_head.weight")[C_:].count_nonzero()) == 0
    assert int(store.g("cls_head.bias")[C_:].count_nonzero()) == 0


def test_loss_and_grads(ref):
    (loss,), store = run(ref["cfg"], ref["P"], ref["batch"])
    sigma = ref["sigma"]
    print(f"GPU loss {loss:.7f} (bf16 oracle {ref['loss16']:.7f}, fp32 {ref['loss32']:.7f}), "
          f"sigma {sigma:.3e}")
    assert abs(loss - ref["loss16"]) < 1e-4 + 3 * sigma, (loss, ref["loss16"], ref["loss32"], sigma)
    check_grads(store, ref["G"], ref["cfg"])


def test_two_adam_steps(ref):
    """The reference recipe's optimizer (Adam with L2 weight decay 0.03, lr 1e-3, linear
    schedule, clipping at 1.0) through trainer.ManualTrainer against torch.optim.Adam."""
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    cfg, P, sigma = ref["cfg"], ref["P"], ref["sigma"]
    batches = [ref["batch"], VO.make_batch(cfg, B, seed=2)]
    lrs = VO.linear_lrs(1e-3, 0, 4, 2)
    assert lrs == [1e-3, 7.5e-4]
    want, _ = VO.train_steps(P, cfg, batches, lrs, "bf16")
    tr = ManualTrainer(StepConfig(model="tiny-vit-cls", scheduler="linear", num_warmup_steps=0,
                                  num_training_steps=4),
                       AdamConfig(lr=1e-3, weight_decay=0.03, adamw=False, max_grad_norm=1.0), "cuda")
    tr.store.load(P)
    tr.store.refresh_shadow()
    got = []
    for bd in batches:
        b = tr.stage(bd)
        assert b.num_items == B
        got.append(tr.train_step([b], b.num_items).item() / b.num_items)
    print(f"two Adam steps: GPU {got}, bf16 oracle {want}, sigma {sigma:.3e}")
    assert abs(got[0] - want[0]) < 1e-4 + 3 * sigma, (got, want, sigma)
    assert abs(got[1] - want[1]) < 3e-4 + 3 * sigma, (got, want, sigma)
    assert got[1] != got[0]
    C_ = cfg.num_classes  # the pad rows stay exactly zero through the decayed update
    assert int(tr.store.p("cls_head.weight")[C_:].count_nonzero()) == 0
    assert int(tr.store.p("cls_head.bias")[C_:].count_nonzero()) == 0


def test_grad_accumulation_equals_big_batch(ref):
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg, bd = ref["cfg"], ref["batch"]
    _, full = run(cfg, ref["P"], bd)
    store, eng = engine_for(cfg, ref["P"])
    total = 0.0
    for sl in (slice(0, 4), slice(4, 8)):
        b = Batch(cfg, None, bd["labels"][sl], bd["pixel_values"][sl], store.device)
        total += eng.forward(b, 1.0 / B).item()
        eng.backward(b)
    err = ((store.grad - full.grad).norm() / full.grad.norm()).item()
    assert err < 1e-2, err
    assert abs(total / B - ref["loss16"]) < 1e-4 + 3 * ref["sigma"]


def test_reset_and_eval_forward(ref):
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg, bd = ref["cfg"], ref["batch"]
    (loss,), full = run(cfg, ref["P"], bd)
    store, eng = engine_for(cfg, ref["P"])
    b = Batch(cfg, None, bd["labels"], bd["pixel_values"], store.device)
    eng.forward(b, 1.0 / B)
    assert eng.cache
    eng.reset()
    assert eng.cache == {}
    ev = eng.forward(b, 1.0 / B, need_grad=False).item() / B
    assert eng.cache == {} and ev == pytest.approx(loss, abs=1e-6)
    eng.forward(b, 1.0 / B)
    eng.backward(b)
    assert torch.equal(bits(store.grad), bits(full.grad))


# ------------------------------------------------------------------ dropout
@pytest.fixture(scope="module")
def drop_ref(K, ref):
    from multimodal_llm_pretraining_amd import config as C

    cfg = C.get_config("tiny-vit-cls-drop")
    assert cfg.vision.hidden_dropout == 0.1
    loss16, G = VO.loss_and_grads(ref["P"], cfg, ref["batch"], "bf16", drop=Masks(K, cfg, 1234, 0))
    return dict(cfg=cfg, loss16=loss16, G=G)


def test_dropout_against_masked_oracle(ref, drop_ref):
    cfg = drop_ref["cfg"]
    (loss,), store = run(cfg, ref["P"], ref["batch"], seed=1234)
    print(f"dropout: GPU loss {loss:.7f}, masked bf16 oracle {drop_ref['loss16']:.7f}, "
          f"sigma {ref['sigma']:.3e}")
    assert abs(loss - drop_ref["loss16"]) < 1e-4 + 3 * ref["sigma"], (loss, drop_ref["loss16"])
    assert abs(loss - ref["loss16"]) > 1e-3  # and the masks did something
    check_grads(store, drop_ref["G"], cfg)


def test_dropout_checkpointing_steps_and_eval(ref, drop_ref):
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg, P, bd = drop_ref["cfg"], ref["P"], ref["batch"]
    la, a = run(cfg, P, bd, steps=2, seed=1234)
    lb, b = run(cfg, P, bd, steps=2, seed=1234, checkpointing=True)
    assert la == lb and torch.equal(bits(a.grad), bits(b.grad))  # recompute repeats the masks
    assert la[0] != la[1]  # the second micro-step draws other masks
    (l0,), s0 = run(cfg, P, bd, seed=1234)
    assert l0 == la[0] and not torch.equal(bits(s0.grad), bits(a.grad))
    # dropout_enabled = False is the p = 0 model, bit for bit
    (lp,), plain = run(ref["cfg"], P, bd)
    store, eng = engine_for(cfg, P)
    eng.dropout_enabled = False
    bt = Batch(cfg, None, bd["labels"], bd["pixel_values"], store.device)
    le = eng.forward(bt, 1.0 / B).item() / B
    eng.backward(bt)
    assert le == lp and torch.equal(bits(store.grad), bits(plain.grad))
    assert eng.dropout_step == 0


# ------------------------------------------------------------------ drop-in module, hook
def test_dropin_module(ref):
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining

    cfg, P, bd = ref["cfg"], ref["P"], ref["batch"]
    (loss,), eng_store = run(cfg, P, bd)
    m = MMPTForPretraining(cfg)
    assert (m.config.hidden_size, m.config.num_labels, m.config.image_size) == (128, 1001, 64)
    m.store.load(P)
    m.store.refresh_shadow()
    out = m(pixel_values=bd["pixel_values"], labels=bd["labels"])
    assert out.loss.item() == pytest.approx(loss, abs=1e-6)
    out.loss.backward()
    assert m.engine.cache == {}
    for name, p in m.named_parameters():
        assert p.grad is not None and p.grad.data_ptr() == m.store.g(name).data_ptr(), name
        assert torch.equal(bits(p.grad), bits(eng_store.g(name))), name
    half = m(pixel_values=bd["pixel_values"], labels=bd["labels"], num_items_in_batch=2 * B)
    assert half.loss.item() == pytest.approx(loss / 2, rel=1e-6)
    m.engine.reset()
    with torch.no_grad():
        ev = m(pixel_values=bd["pixel_values"], labels=bd["labels"])
    assert m.engine.cache == {} and ev.loss.item() == pytest.approx(loss, abs=1e-6)
    with pytest.raises(ValueError, match="input_ids"):
        m(input_ids=torch.zeros(B, 4, dtype=torch.int64), pixel_values=bd["pixel_values"],
          labels=bd["labels"])


def test_dropin_eval_switches_dropout_off(ref, drop_ref):
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining

    bd = ref["batch"]
    m = MMPTForPretraining(drop_ref["cfg"], seed=1234)
    m.store.load(ref["P"])
    m.store.refresh_shadow()
    with torch.no_grad():
        train = m(pixel_values=bd["pixel_values"], labels=bd["labels"]).loss.item()
        m.eval()
        ev = m(pixel_values=bd["pixel_values"], labels=bd["labels"]).loss.item()
    assert train == pytest.approx(drop_ref["loss16"], abs=1e-4 + 3 * ref["sigma"])
    assert ev == pytest.approx(ref["loss16"], abs=1e-4 + 3 * ref["sigma"]) and ev != train


def test_grad_ready_hook_covers_every_parameter_once(ref):
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg, bd = ref["cfg"], ref["batch"]
    store, eng = engine_for(cfg, ref["P"])
    seen = []
    eng.grad_ready_hook = lambda lo, hi: seen.append((lo, hi))
    b = Batch(cfg, None, bd["labels"], bd["pixel_values"], store.device)
    eng.forward(b, 1.0 / B)
    eng.backward(b)
    torch.cuda.synchronize()
    assert seen
    seen.sort()
    for (_, hi), (lo, _) in zip(seen, seen[1:]):
        assert hi <= lo, seen  # no element announced twice
    for name, off in store.offsets.items():
        n = store.g(name).numel()
        assert any(lo <= off and off + n <= hi for lo, hi in seen), name


# ------------------------------------------------------------------ offload, harness
def test_offloaded_optimizer_matches_device_adam(ref):
    """Optimizer offload only touches the flat buffers and gates each unit's first forward on
    its host update (cls_head is a unit of its own): first-step losses equal (same gradients),
    later ones within the project's 1e-4 (tests/test_sharding_gpu.py's offload bar)."""
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig
    from multimodal_llm_pretraining_amd.zero3 import unit_of

    assert unit_of("cls_head.weight") == unit_of("cls_head.bias") == "cls_head"
    assert unit_of("vision.ln_post.weight") is None
    cfg, P = ref["cfg"], ref["P"]
    batches = [ref["batch"], VO.make_batch(cfg, B, seed=2), VO.make_batch(cfg, B, seed=3)]
    got = {}
    for offload in (False, True):
        tr = ManualTrainer(StepConfig(model="tiny-vit-cls", scheduler="constant", offload=offload),
                           AdamConfig(lr=1e-3, weight_decay=0.03, adamw=False, max_grad_norm=1.0),
                           "cuda")
        tr.store.load(P)
        tr.store.refresh_shadow()
        got[offload] = []
        for bd in batches:
            b = tr.stage(bd)
            got[offload].append(tr.train_step([b], b.num_items).item() / b.num_items)
        tr.flush()
    assert got[True][0] == got[False][0], got
    for a, b in zip(got[True][1:], got[False][1:]):
        assert abs(a - b) < 1e-4, got


def test_harness_runs_the_image_batches(ref):
    """TrainingClass.build_trainer → benchmarking.ManualTrainer → estimate_step_time over the
    dummy image dataset (plain and zero_1 with optimizer offload); ZeRO-2 is refused by name
    before the module's storage is touched."""
    from multimodal_llm_pretraining_amd.benchmarking import estimate_step_time
    from multimodal_llm_pretraining_amd.data import DummyImageClassificationDataset
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining
    from multimodal_llm_pretraining_amd.train import TrainingClass

    cfg = ref["cfg"]
    ds = DummyImageClassificationDataset(cfg.vision.image, cfg.num_classes, num_samples=32)
    kw = dict(num_training_steps=4, micro_batch_size=4, gradient_accumulation_steps=1, bf16=True,
              optimizer=torch.optim.Adam,
              optimizer_kwargs={"lr": 1e-3, "betas": (0.9, 0.999), "weight_decay": 0.03},
              scheduler_type="linear", scheduler_kwargs={"num_warmup_steps": 1}, max_grad_norm=1.0)
    for extra in ({}, {"zero_stage": "1", "zero_offload_optimizer": True}):
        m = MMPTForPretraining(cfg)
        tr = TrainingClass(**kw, **extra).build_trainer(m, ds)
        before = m.store.w("cls_head.weight").clone()
        assert estimate_step_time(tr, 4, 8, 1) > 0
        torch.cuda.synchronize()
        assert not torch.equal(m.store.w("cls_head.weight"), before)  # the steps trained it
    m = MMPTForPretraining(cfg)
    with pytest.raises(NotImplementedError, match="zero_2"):
        TrainingClass(**kw, zero_stage="2").build_trainer(m, ds)
    assert not m.partitioned and m.store.master.numel() == m.store.padded
