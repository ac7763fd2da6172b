"""Label smoothing on the GPU (include/mmpt.h K12, mmpt_cross_entropy_smooth).

Kernels, through the C ABI: the smoothed loss rows and gradients against the fp64 row formulas of
tests/label_smoothing_ref.py computed from the same bf16 logits, at every kernel form (the
register form's four chunk counts, fewer chunks than threads, the streaming kernel), in place,
out of place and forward-only; an out-of-range label; eps = 0 through the new entry bitwise the
old entry; the register form bitwise the streaming form; bad factors refused before any launch.

Engine and trainer: gradient parity of every family against its oracle with
torch.nn.functional.cross_entropy smoothed (label_smoothing_ref.smoothed_cross_entropy), each at
the bar of that family's own parity test; two optimizer steps through the facade; activation
checkpointing and zero_3 on one rank bitwise the plain step; the forward-only loss.
"""

import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import label_smoothing_ref as LS  # noqa: E402

pytestmark = pytest.mark.gpu

dev = "cuda"
EPS = 0.1  # the engine / trainer tests' factor
R = 41  # rows of the kernel tests: every fifth ignored, one labelled 0, one labelled V - 1
SCALE = 0.5
# (vocab, vocab_valid): fewer chunks than threads, NC = 8 with padding, NC = 16, 25, 32, streaming
SHAPES = [(16, 10), (2048, 2000), (16392, 16392), (50304, 50304), (65536, 65536), (128264, 128257)]
REG_SHAPES = SHAPES[:5]
# the fp32 term of the gradient bound (derived in test_rows_match_fp64's docstring)
A_FP32 = 2.0 ** -17


def _inputs(V, vv):
    g = torch.Generator(device=dev).manual_seed(6 + V)
    logits = (torch.randn(R, V, device=dev, generator=g) * 3).to(torch.bfloat16)
    labels = torch.randint(0, vv, (R,), device=dev, generator=g)
    labels[1], labels[2] = 0, vv - 1
    labels[::5] = -100
    return logits, labels


_cache: dict = {}


def inputs(V, vv):
    """The seeded logits / labels of a shape, made once and never written (runs work on clones)."""
    if (V, vv) not in _cache:
        _cache[(V, vv)] = _inputs(V, vv)
    return _cache[(V, vv)]


def smooth(logits, labels, vv, eps, mode="inplace", entry="mmpt_cross_entropy_smooth", scale=SCALE):
    """(loss rows, dlogits or None) of one call; mode: inplace / outofplace / null."""
    from multimodal_llm_pretraining_amd import _lib

    rows, V = logits.shape
    x = logits.clone()
    loss = torch.full((rows,), 7.0, device=dev)
    dl = {"inplace": x, "outofplace": torch.full_like(x, 7.0), "null": None}[mode]
    args = [rows, V, vv, x.data_ptr(), V, labels.data_ptr(), -100, scale]
    if entry == "mmpt_cross_entropy_smooth":
        args.append(eps)
    _lib.call(entry, *args, loss.data_ptr(), 0 if dl is None else dl.data_ptr(),
              0 if dl is None else V, torch.cuda.current_stream().cuda_stream)
    if mode != "inplace":
        assert torch.equal(x, logits)  # the logits are only read
    return loss, dl


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def grad_excess(got, ref, p, eps, vv, scale=SCALE):
    """The largest a the gradient bound |got - ref| <= 2^-8 |ref| + a scale (softmax + eps / V)
    would need over all elements (<= 0: the first term alone covers every element)."""
    err = (got.double() - ref).abs() - 2.0 ** -8 * ref.abs()
    return (err / (scale * (p + eps / vv)).clamp_min(1e-300)).max().item()


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("eps", [0.1, 0.9])
@pytest.mark.parametrize("V,vv", SHAPES)
def test_rows_match_fp64(V, vv, eps):
    """Loss rows within 1e-4 (the bound of test_kernels_gpu's cross-entropy tests) and every
    gradient element within 2^-8 |ref| + a grad_scale (softmax_v + eps / V) of the fp64 formulas
    on the same bf16 logits: one bf16 rounding, doubled, plus the fp32 evaluation of the two terms.

    a = 2^-17.  The same formula at eps = 0 on mmpt_cross_entropy needs no second term at these
    inputs (measured on an MI355X: the largest excess over 2^-8 |ref| is 0 at all six shapes —
    without smoothing no gradient element is a difference of nearly equal terms, so the bf16
    rounding covers every element and the measurement sets no lower limit for a).  a is therefore
    the fp32 error of softmax_v itself: __expf(t) = exp2(t log2 e) carries the rounding of its
    argument, |t| 2^-24 relative with |t| = max - x <= 2^5 for these logits (3 sigma bf16 rows):
    2^-19; the sum of the row's exponentials, about 2^9 sequential fp32 additions per thread, adds
    about 2^-20 as a random walk; the reciprocal, the product and the addend one ulp each: 2^-18.3
    in all, and 2^-17 is the smallest power of two with a factor of two to spare.  It is 2^9 below
    the bf16 rounding that the first term allows, so a dropped or doubled eps / V, or a label
    term of 1 instead of 1 - eps, misses the bound by orders of magnitude.  The smoothed kernels
    need a <= 2^-23.6 (the figure each case prints)."""
    logits, labels = inputs(V, vv)
    ref_loss, ref_d, p = LS.ce_rows(logits, labels, eps, vocab_valid=vv, grad_scale=SCALE)
    ign = labels == -100
    for mode in ("outofplace", "inplace", "null"):
        loss, dl = smooth(logits, labels, vv, eps, mode)
        lerr = (loss.double() - ref_loss).abs().max().item()
        print(f"V={V} vv={vv} eps={eps} {mode}: loss rows max err {lerr:.3e}", end="")
        assert lerr < 1e-4, (mode, lerr)
        assert loss[ign].eq(0).all()
        if dl is None:
            print()
            continue
        need = grad_excess(dl, ref_d, p, eps, vv)
        print(f", gradient bound needs a = {need:.3e} (2^{math.log2(max(need, 1e-300)):.1f})")
        bound = 2.0 ** -8 * ref_d.abs() + A_FP32 * SCALE * (p + eps / vv)
        assert ((dl.double() - ref_d).abs() <= bound).all(), (mode, need)
        assert bits(dl[ign]).eq(0).all() and bits(dl[:, vv:]).eq(0).all()
        if mode == "outofplace":
            first = dl
        else:  # in place gives the out-of-place bits
            assert torch.equal(bits(dl), bits(first))


@pytest.mark.parametrize("V,vv", [(2048, 2000), (128264, 128257)])
def test_out_of_range_label(V, vv):
    """A label outside [0, V) that is not ignore_index (a padding column here): that row's loss
    is NaN and its gradient zero; every other row is bitwise what it is without the bad row."""
    logits, labels = inputs(V, vv)
    bad = labels.clone()
    bad[7] = vv
    loss0, d0 = smooth(logits, labels, vv, EPS)
    loss1, d1 = smooth(logits, bad, vv, EPS)
    assert labels[7] != -100 and torch.isnan(loss1[7]) and not torch.isnan(loss0).any()
    assert bits(d1[7]).eq(0).all() and not bits(d0[7]).eq(0).all()
    keep = torch.arange(R, device=dev) != 7
    assert torch.equal(bits(loss1[keep]), bits(loss0[keep]))
    assert torch.equal(bits(d1[keep]), bits(d0[keep]))


@pytest.mark.parametrize("V,vv", [(2048, 2000), (50304, 50304), (128264, 128257)])
def test_zero_factor_is_the_old_entry(V, vv):
    """eps = 0 through the new entry runs the unsmoothed kernels: loss rows and gradient bits
    of mmpt_cross_entropy, register form, streaming form (switch off) and past 65,536 columns."""
    from multimodal_llm_pretraining_amd import _lib

    logits, labels = inputs(V, vv)
    prev = _lib.set_switch("MMPT_CE_REG", 1)
    try:
        for reg in (1, 0):
            _lib.set_switch("MMPT_CE_REG", reg)
            for mode in ("inplace", "outofplace", "null"):
                l0, d0 = smooth(logits, labels, vv, 0.0, mode, entry="mmpt_cross_entropy")
                l1, d1 = smooth(logits, labels, vv, 0.0, mode)
                assert torch.equal(bits(l0), bits(l1)), (reg, mode)
                assert d0 is None or torch.equal(bits(d0), bits(d1)), (reg, mode)
    finally:
        _lib.set_switch("MMPT_CE_REG", prev)


@pytest.mark.parametrize("eps", [0.1, 0.9])
@pytest.mark.parametrize("V,vv", REG_SHAPES)
def test_register_form_is_the_streaming_form(V, vv, eps):
    """With smoothing on, the register-resident kernel is bitwise the two-pass kernel — the same
    chunk-per-thread assignment, so the same order of the max, the sum of exponentials and the
    sum of the logits — for loss rows and gradients, in place and not."""
    from multimodal_llm_pretraining_amd import _lib

    logits, labels = inputs(V, vv)
    out = {}
    prev = _lib.set_switch("MMPT_CE_REG", 0)
    try:
        for reg in (0, 1):
            _lib.set_switch("MMPT_CE_REG", reg)
            out[reg] = [smooth(logits, labels, vv, eps, m) for m in ("inplace", "outofplace")]
    finally:
        _lib.set_switch("MMPT_CE_REG", prev)
    for (l0, d0), (l1, d1) in zip(out[0], out[1]):
        assert torch.equal(bits(l0), bits(l1))
        assert torch.equal(bits(d0), bits(d1))
    assert not torch.equal(bits(out[1][0][1]), bits(smooth(logits, labels, vv, 0.0)[1]))


@pytest.mark.parametrize("bad", [-0.1, 1.0, float("nan")])
def test_bad_factor_is_refused(bad):
    """RuntimeError naming label_smoothing, and nothing launched: the outputs keep their fill."""
    logits, labels = inputs(2048, 2000)
    x = logits.clone()
    loss = torch.full((R,), 7.0, device=dev)
    dl = torch.full_like(x, 7.0)
    from multimodal_llm_pretraining_amd import _lib

    with pytest.raises(RuntimeError, match="label_smoothing"):
        _lib.call("mmpt_cross_entropy_smooth", R, 2048, 2000, x.data_ptr(), 2048,
                  labels.data_ptr(), -100, SCALE, bad, loss.data_ptr(), dl.data_ptr(), 2048,
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert loss.eq(7.0).all() and dl.eq(7.0).all() and torch.equal(x, logits)
    from multimodal_llm_pretraining_amd import kernels as K

    with pytest.raises(RuntimeError, match="label_smoothing"):
        K.cross_entropy(x, labels, -100, SCALE, loss, dl, vocab_valid=2000, label_smoothing=bad)
    assert loss.eq(7.0).all() and dl.eq(7.0).all()


# ------------------------------------------------------------------ engine: parity with the oracles
# At near-initial weights softmax is almost uniform, so the smoothed gradient is almost (1 - eps)
# times the unsmoothed one and the two losses almost coincide: a comparison at the families' 3e-2
# bar would nearly pass without any smoothing.  Each family is therefore compared at weights fitted
# to its batch by a few fp32 Adam steps of its own oracle (unsmoothed): the fitted model is
# confident, its unsmoothed gradient small, and the smoothing term eps (onehot - 1 / V) a large
# part of the smoothed gradient.  Every case first asserts, on the oracle alone, that the smoothed
# and the unsmoothed gradients (and losses) differ by at least ten times the bar they are
# compared at (measured on the CPU: flat gradients differ by 0.4 to 1.0, losses by 0.4 to 1.5).
GRAD_BAR = 3e-2  # ||got - ref|| / ||ref||, the gradient bar of every family's parity test


def fit(P, loss_fn, steps, lr):
    params = {k: v.clone().requires_grad_() for k, v in P.items()}
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        loss_fn(params).backward()
        opt.step()
    return {k: v.detach() for k, v in params.items()}


def flat(G, names):
    return torch.cat([G[k].flatten().float() for k in names])


def relerr(a, b):
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def engine_step(cfg, P, batch, eps, checkpointing=False):
    """(loss per item, {name: gradient}, forward-only loss per item) of one smoothed step."""
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.engine import Batch, Engine
    from multimodal_llm_pretraining_amd.params import ParamStore

    store = ParamStore(C.param_shapes(cfg), "cuda")
    store.load(P)
    store.refresh_shadow()
    eng = Engine(cfg, store)
    eng.checkpointing, eng.label_smoothing = checkpointing, eps
    b = Batch(cfg, batch.get("input_ids"), batch["labels"], batch.get("pixel_values"), store.device)
    fwd = eng.forward(b, 1.0 / b.num_items, need_grad=False).item() / b.num_items
    assert eng.cache == {}
    store.zero_grad()
    loss = eng.forward(b, 1.0 / b.num_items).item() / b.num_items
    eng.backward(b)
    torch.cuda.synchronize()
    return loss, {k: store.g(k).cpu() for k in P}, fwd


def _mm_family(name, text_len):
    from oracle import model as O
    from test_parity_gpu import oracle_cfg

    from multimodal_llm_pretraining_amd import config as C

    cfg = C.get_config(name)
    ocfg = oracle_cfg(cfg)
    batch = O.make_batch(ocfg, 3, text_len, seed=1)

    def loss_and_grads(P, precision):
        Pr = {k: v.clone().requires_grad_() for k, v in P.items()}
        loss = O.forward_loss(Pr, ocfg, batch, precision)
        loss.backward()
        return loss.item(), {k: v.grad for k, v in Pr.items()}

    def loss_bar(P):  # test_parity_gpu.test_loss_and_grads: 1e-4 + |bf16 - fp32|
        with torch.no_grad():
            return 1e-4 + abs(O.forward_loss(P, ocfg, batch, "bf16").item() -
                              O.forward_loss(P, ocfg, batch, "fp32").item())

    return dict(cfg=cfg, P=O.init_params(ocfg, seed=0), batch=batch, loss_bar=loss_bar,
                loss_fn=lambda Pr: O.forward_loss(Pr, ocfg, batch, "fp32"),
                loss_and_grads=loss_and_grads)


def _oracle_family(name, mod, make_batch, sigma_args, extra=()):
    from multimodal_llm_pretraining_amd import config as C

    cfg = C.get_config(name)
    batch = make_batch(mod, cfg)
    return dict(cfg=cfg, P=mod.init_params(cfg, seed=0), batch=batch,
                # the families' test_loss_and_grads: 1e-4 + 3 sigma at the batch's shape
                loss_bar=lambda P: 1e-4 + 3 * mod.bf16_sigma(P, cfg, *sigma_args),
                loss_fn=lambda Pr: mod.forward_loss(Pr, cfg, batch, "fp32"),
                loss_and_grads=lambda P, precision: mod.loss_and_grads(P, cfg, batch, precision,
                                                                       *extra))


def family(name):
    if name == "tiny-mm":
        return _mm_family(name, 47)
    if name == "tiny-llama":  # a padded vocabulary: 515 real classes in 520 columns
        return _mm_family(name, 130)
    if name == "tiny-roberta":
        import roberta_oracle as RO
        return _oracle_family(name, RO, lambda m, c: m.make_batch(c, 4, 48, seed=1), (4, 48))
    if name == "tiny-vit-cls":
        import vit_cls_oracle as VO
        return _oracle_family(name, VO, lambda m, c: m.make_batch(c, 8, seed=1), (8,))
    if name == "tiny-convnext":
        import convnext_oracle as CO
        return _oracle_family(name, CO, lambda m, c: m.make_batch(c, 8, seed=1), (8,))
    import mamba_oracle as MO
    return _oracle_family(name, MO, lambda m, c: m.make_batch(c, 3, 70, seed=1), (3, 70), ("fused",))


# (fitting steps, lr) per family, chosen on the CPU from the oracle alone: the flat smoothed and
# unsmoothed gradients differ by >= 0.45 and the bf16 oracle's flat gradient stays within 1.5e-2
# of the fp32 oracle's (so the fit has not reached the point where the smoothed gradient cancels)
FIT = {"tiny-mm": (16, 3e-3), "tiny-llama": (18, 3e-3), "tiny-roberta": (12, 3e-3),
       "tiny-vit-cls": (12, 2e-3), "tiny-convnext": (8, 3e-3), "tiny-mamba": (6, 3e-3)}


_fitted: dict = {}


def fitted(name):
    """(the family, its fitted weights), made once per family and never written."""
    if name not in _fitted:
        f = family(name)
        _fitted[name] = (f, fit(f["P"], f["loss_fn"], *FIT[name]))
    return _fitted[name]


@pytest.mark.parametrize("name", list(FIT))
def test_gradient_parity_with_the_oracle(name):
    """Loss and flat gradient of one smoothed engine step against the family's oracle with
    F.cross_entropy smoothed, at that family's parity bars; the forward-only loss is the same
    smoothed loss.  Fails without smoothing by construction (the discrimination asserts)."""
    f, P = fitted(name)
    cfg, batch = f["cfg"], f["batch"]
    names = list(P)
    loss_u, G_u = f["loss_and_grads"](P, "bf16")
    with LS.smoothed_cross_entropy(EPS):
        loss_s, G_s = f["loss_and_grads"](P, "bf16")
        loss_bar = f["loss_bar"](P)
    gap = relerr(flat(G_u, names), flat(G_s, names))
    print(f"{name}: oracle loss {loss_u:.5f} unsmoothed, {loss_s:.5f} smoothed (bar {loss_bar:.2e}); "
          f"flat gradients differ by {gap:.3f}")
    assert gap >= 10 * GRAD_BAR and abs(loss_s - loss_u) >= 10 * loss_bar  # discrimination
    loss, G, fwd = engine_step(cfg, P, batch, EPS)
    err = relerr(flat(G, names), flat(G_s, names))
    worst = max((relerr(G[k], G_s[k]), k) for k in names)
    print(f"{name}: GPU loss {loss:.7f} (forward only {fwd:.7f}), d {loss - loss_s:+.2e}; flat "
          f"gradient error {err:.2e}; worst tensor {worst[1]} {worst[0]:.2e}")
    assert abs(loss - loss_s) < loss_bar, (loss, loss_s, loss_bar)
    assert abs(fwd - loss_s) < loss_bar and abs(fwd - loss) < 1e-6
    assert err < GRAD_BAR, err


# ------------------------------------------------------------------ trainer and facade (tiny-mm)
def _mm_setup(steps, n=4, text_len=40):
    from oracle import model as O
    from test_parity_gpu import oracle_cfg

    from multimodal_llm_pretraining_amd import config as C

    ocfg = oracle_cfg(C.get_config("tiny-mm"))
    P = O.init_params(ocfg, seed=0)
    g = torch.Generator().manual_seed(7)  # (test_sharding_gpu._setup(perturb=True))
    P = {k: v * (1.0 + 0.25 * torch.randn(v.shape, generator=g)) for k, v in P.items()}
    return ocfg, P, [O.make_batch(ocfg, n, text_len, seed=s) for s in range(1, steps + 1)]


def _trainer(P, eps, sharding="", ac=False):
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    tr = ManualTrainer(StepConfig(model="tiny-mm", sharding=sharding, scheduler="constant",
                                  activation_checkpointing=ac, label_smoothing=eps),
                       AdamConfig(lr=1e-3), "cuda")
    tr.store.load(P)
    tr.store.refresh_shadow()
    return tr


def _run_accumulated(tr, batches):
    """Each 4-sample batch as two accumulated 2-sample micro-batches (test_sharding_gpu)."""
    losses = []
    for bd in batches:
        full = tr.stage(bd)
        mbs = [tr.stage({k: v[sl] for k, v in bd.items()}) for sl in (slice(0, 2), slice(2, 4))]
        losses.append(tr.train_step(mbs, full.num_items).item() / full.num_items)
    torch.cuda.synchronize()
    return losses


def _master(tr):
    if hasattr(tr.opt, "sync_master"):
        tr.opt.sync_master()
    return {k: v.detach().float().cpu() for k, v in tr.store.state_dict().items()}


def test_checkpointing_and_zero3_are_bitwise_with_smoothing():
    """With eps = 0.1: activation checkpointing is bit-identical to stored activations, zero_3 on
    one rank bitwise data parallel — and the step is not the unsmoothed one."""
    _, P, batches = _mm_setup(2)
    ref = _trainer(P, EPS)
    ref_losses = _run_accumulated(ref, batches)
    want = _master(ref)
    ac = _trainer(P, EPS, ac=True)
    assert _run_accumulated(ac, batches) == ref_losses
    assert torch.equal(ac.store.master, ref.store.master)
    assert torch.equal(ac.store.shadow, ref.store.shadow)
    z = _trainer(P, EPS, sharding="zero_3")
    assert _run_accumulated(z, batches) == ref_losses
    got = _master(z)
    for n in want:
        assert torch.equal(got[n], want[n]), n
    plain = _trainer(P, 0.0)
    assert _run_accumulated(plain, batches) != ref_losses
    assert not torch.equal(plain.store.master, ref.store.master)


def _facade(P, overrides):
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.data import DummyMultimodalLanguageModelingDataset
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining
    from multimodal_llm_pretraining_amd.train import TrainingClass

    cfg = C.get_config("tiny-mm")
    m = MMPTForPretraining(cfg)
    m.store.load(P)
    m.store.refresh_shadow()
    tc = TrainingClass(num_training_steps=4, micro_batch_size=2, gradient_accumulation_steps=1,
                       bf16=True, optimizer=torch.optim.AdamW, optimizer_kwargs={"lr": 1e-3},
                       scheduler_type="constant", max_grad_norm=0.0)
    # (the steps below feed the oracle's batches; the trainer only holds the dataset)
    ds = DummyMultimodalLanguageModelingDataset(cfg.text.n_vocab, 64, cfg.vision.image, 8,
                                                image_token_id=cfg.image_token_id,
                                                image_tokens=cfg.vision.num_patches)
    tr = tc.build_trainer(m, ds) if overrides is None else \
        tc.build_trainer(m, ds, hf_training_args_overrides=overrides)
    return m, tr


def _facade_steps(m, tr, batches):
    losses = []
    for bd in batches:
        losses.append(tr.manual_training_step(m, bd).item())
        tr.manual_optimization_step(m)
    torch.cuda.synchronize()
    return losses


def test_two_steps_through_the_facade():
    """build_trainer(hf_training_args_overrides={"label_smoothing_factor": 0.1}): two AdamW steps
    match the oracle's smoothed train_steps at test_parity_gpu's two-step bars (1e-4 and 3e-4,
    each plus |bf16 - fp32| of the oracle); the model's own .loss stays unsmoothed; without the
    key the trainer is bitwise the one built without overrides."""
    from oracle import model as O

    from test_parity_gpu import oracle_cfg

    # the fitted weights of the parity test: at perturbed initial weights the two losses are too
    # close (5e-3 apart) for the two-step bars to tell them apart
    f, P = fitted("tiny-mm")
    ocfg = oracle_cfg(f["cfg"])
    batches = [f["batch"], O.make_batch(ocfg, 3, 47, seed=2)]
    opt, lrs = O.OptimCfg(kind="adamw", lr=1e-3), [1e-3, 1e-3]
    with LS.smoothed_cross_entropy(EPS):
        want, _ = O.train_steps(P, ocfg, batches, opt, lrs, "bf16")
        want32, _ = O.train_steps(P, ocfg, batches, opt, lrs, "fp32")
    plain, _ = O.train_steps(P, ocfg, batches, opt, lrs, "bf16")
    floor = [abs(a - b) for a, b in zip(want, want32)]
    bars = [1e-4 + floor[0], 3e-4 + floor[1]]
    assert all(abs(a - b) >= 10 * bar for a, b, bar in zip(want, plain, bars))  # discrimination
    m, tr = _facade(P, {"label_smoothing_factor": EPS})
    assert tr.core.step_cfg.label_smoothing == EPS and m.engine.label_smoothing == EPS
    with torch.no_grad():
        own = m(**batches[0]).loss.item()  # HF smooths in the Trainer, not in the model
    assert abs(own - plain[0]) < bars[0] and m.engine.label_smoothing == EPS
    got = _facade_steps(m, tr, batches)
    print(f"facade {got}, oracle smoothed {want} (fp32 {want32}), unsmoothed {plain}")
    assert abs(got[0] - want[0]) < bars[0] and abs(got[1] - want[1]) < bars[1], (got, want)
    # no key, the key at 0, and no overrides at all: one and the same step, the parent's
    runs = []
    for overrides in (None, {}, {"label_smoothing_factor": 0.0}):
        m, tr = _facade(P, overrides)
        assert m.engine.label_smoothing == 0.0
        runs.append((_facade_steps(m, tr, batches), m.store.master.clone()))
    for losses, master in runs[1:]:
        assert losses == runs[0][0] and torch.equal(master, runs[0][1])
    assert all(abs(a - b) < bar for a, b, bar in zip(runs[0][0], plain, bars))
    with pytest.raises(ValueError, match="label_smoothing_factor"):
        _facade(P, {"label_smoothing_factor": 1.0})


def test_forward_only_loss_is_smoothed():
    """forward(need_grad=False) returns the smoothed loss (HF smooths in evaluation too) and, at
    the default 0, the unsmoothed one — each against the bf16 oracle at test_parity_gpu's
    1e-4 + |bf16 - fp32|, on the fitted weights, where the two losses are 1.5 apart."""
    from test_parity_gpu import gpu_setup

    from multimodal_llm_pretraining_amd.engine import Batch

    f, P = fitted("tiny-mm")
    bd = f["batch"]
    plain, _ = f["loss_and_grads"](P, "bf16")
    bar0 = f["loss_bar"](P)
    with LS.smoothed_cross_entropy(EPS):
        want, _ = f["loss_and_grads"](P, "bf16")
        bar = f["loss_bar"](P)
    assert abs(want - plain) >= 10 * max(bar, bar0)
    cfg, store, eng = gpu_setup("tiny-mm", P)
    b = Batch(cfg, bd["input_ids"], bd["labels"], bd["pixel_values"], store.device)
    got0 = eng.forward(b, 1.0 / b.num_items, need_grad=False).item() / b.num_items
    eng.label_smoothing = EPS
    got = eng.forward(b, 1.0 / b.num_items, need_grad=False).item() / b.num_items
    assert eng.cache == {}
    print(f"forward only: {got0:.7f} (oracle {plain:.7f}), smoothed {got:.7f} (oracle {want:.7f})")
    assert abs(got0 - plain) < bar0, (got0, plain, bar0)
    assert abs(got - want) < bar, (got, want, bar)
