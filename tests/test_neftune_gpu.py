"""NEFTune on the GPU (TrainingArguments.neftune_noise_alpha; include/mmpt.h K8).

* the kernels: mmpt_embed_noise / mmpt_embed_noise_fwd bitwise against the numpy float32
  restatement (tests/neftune_ref.py); the RoBERTa noise kernels at the bounds test_roberta_gpu.py
  holds the noise-free entries to, on e with the reference noise, and bitwise the existing entries
  at mag = 0;
* the engine against each family's oracle fed the reference noise through a hook on its input
  embedding, at that family's own parity bars (test_parity_gpu.py, test_mamba_gpu.py,
  test_roberta_gpu.py), alpha = 5;
* the semantics on tiny-lm (determinism, counter, checkpointing, ZeRO-3, eval, preview, facade)
  and the default path, which launches what it launched before.
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mamba_oracle as MO  # noqa: E402
import neftune_ref as NR  # noqa: E402
import roberta_oracle as RO  # noqa: E402
from oracle import model as O  # noqa: E402
from test_parity_gpu import gpu_setup, oracle_cfg  # noqa: E402
from test_roberta_gpu import (EPS, embed_case, existing_bwd, gen, ln_bwd64, params, rel, same,  # noqa: E402
                              stats)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
ERR_ARG = "status -1"
ALPHA, SEED = 5.0, 1234
SITE = (7 << 32) | (3 << 16) | 4  # a noise site of some later step and rank (unit 0, k 4)


@pytest.fixture(scope="module")
def K():
    from multimodal_llm_pretraining_amd import kernels

    return kernels


def site0(eng, step=0):
    from multimodal_llm_pretraining_amd.engine import dropout_site

    return dropout_site(step, eng.rank, 0, 4)


def t32(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


# ------------------------------------------------------------------ mmpt_embed_noise(_fwd)
SHAPES = [(7, 64), (5, 2560), (9, 100)]


@pytest.mark.parametrize("rows,h", SHAPES)
def test_embed_noise_is_the_reference(K, rows, h):
    mag = NR.mag_of(ALPHA, 130, h)
    got = K.embed_noise(rows, h, K.EmbedNoise(float(mag), SEED, SITE))
    want = t32(NR.noise(rows, h, SITE, SEED, mag))
    assert same(got, want)
    assert float(got.abs().max()) < float(mag) and int((got == 0).sum()) == 0
    assert same(K.embed_noise(rows, h, K.EmbedNoise(0.0, SEED, SITE)).abs(), torch.zeros(rows, h))


@pytest.mark.parametrize("rows,h", SHAPES)
def test_embed_noise_fwd_is_table_plus_reference(K, rows, h):
    g = torch.Generator().manual_seed(31 * rows + h)
    vocab = 37
    table = torch.randn(vocab, h, generator=g) * 0.02
    ids = torch.randint(0, vocab, (rows,), generator=g)
    ids[0], ids[-1] = 0, vocab - 1
    mag = NR.mag_of(ALPHA, 130, h)
    nz = NR.noise(rows, h, SITE, SEED, mag)
    noise = K.EmbedNoise(float(mag), SEED, SITE)
    out = torch.full((rows, h), float("nan"), device="cuda")
    K.embed_fwd(ids.cuda(), table.cuda(), out, noise=noise)
    want = t32(NR.add(table[ids].numpy(), nz))
    assert same(out, want)
    plain = torch.empty_like(out)
    K.embed_fwd(ids.cuda(), table.cuda(), plain)
    assert same(plain, table[ids]) and not same(plain, out)
    # with an image map: image rows are the features, untouched; text rows keep their own row's
    # noise (the row index counts every row)
    imap = torch.full((rows,), -1, dtype=torch.int32)
    img_rows = [1, 2, rows - 2]
    imap[img_rows] = torch.tensor([2, 0, 1], dtype=torch.int32)
    img = (torch.randn(3, h, generator=g)).to(BF16)
    out2 = torch.full((rows, h), float("nan"), device="cuda")
    K.embed_fwd(ids.cuda(), table.cuda(), out2, imap.cuda(), img.cuda(), noise=noise)
    want2 = want.clone()
    want2[img_rows] = img[[2, 0, 1]].float()
    assert same(out2, want2)


def test_noise_argument_errors(K):
    from multimodal_llm_pretraining_amd import _lib

    out = torch.full((4, 64), float("nan"), device="cuda")
    table = torch.zeros(8, 64, device="cuda")
    ids = torch.zeros(4, dtype=torch.int64, device="cuda")

    def fwd(rows=4, h=64, mag=0.1):
        _lib.call("mmpt_embed_noise_fwd", rows, h, ids.data_ptr(), table.data_ptr(), 0, 0,
                  out.data_ptr(), mag, SEED, SITE, 0)

    def alone(rows=4, h=64, mag=0.1):
        _lib.call("mmpt_embed_noise", rows, h, mag, SEED, SITE, out.data_ptr(), 0)

    for f in (fwd, alone):
        for kw in (dict(h=62), dict(h=0), dict(rows=0), dict(rows=1 << 31), dict(mag=-0.1),
                   dict(mag=float("nan")), dict(mag=float("inf")),
                   dict(rows=(1 << 31) - 1, h=1 << 31)):
            with pytest.raises(RuntimeError, match=ERR_ARG):
                f(**kw)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()  # nothing was launched
    # the RoBERTa noise entries check mag the same way, before any launch
    ids_, pos, word, ptab, typ = embed_case(3, 72, gen(3, 72, 9))
    w, b = params(72, gen(3, 72, 9))
    h32 = torch.full((3, 72), float("nan"), device="cuda")
    h16 = torch.empty(3, 72, dtype=BF16, device="cuda")
    mean, rstd = w.new_empty(3), w.new_empty(3)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match=ERR_ARG):
            K.roberta_embed_fwd(ids_, pos, word, ptab, typ, w, b, EPS, h32, h16, mean, rstd,
                                noise=K.EmbedNoise(bad, SEED, SITE))
        with pytest.raises(RuntimeError, match=ERR_ARG):
            K.roberta_embed_bwd(ids_, pos, word, ptab, typ, mean, rstd, w, h32, h32,
                                noise=K.EmbedNoise(bad, SEED, SITE))
    torch.cuda.synchronize()
    assert torch.isnan(h32).all()


# ------------------------------------------------------------------ the RoBERTa noise kernels
R_ROWS, R_HS = (1, 3, 257), (72, 128, 1024, 1032)
R_MAG = 0.5  # against unit-variance tables: a backward that drew other noise is far outside
R_DSITE = (7 << 32) | (3 << 4) | 1  # the hidden-dropout site of test_roberta_gpu.py


def noisy_e(word, ids, ptab, pos, typ, rows, h, mag):
    """e = ((word[ids] + noise) + type) + pos_table[pos], each add one fp32 rounding."""
    nz = t32(NR.noise(rows, h, SITE, SEED, np.float32(mag))).cuda()
    return (((word[ids] + nz) + typ) + ptab[pos]).contiguous()


@pytest.mark.parametrize("p", (0.0, 0.1))
@pytest.mark.parametrize("h", R_HS)
@pytest.mark.parametrize("rows", R_ROWS)
def test_roberta_embed_noise_fwd(K, rows, h, p):
    """test_roberta_gpu.test_roberta_embed_fwd's bound — the bits of the fp32 LayerNorm and dropout
    kernels over the same e — with e carrying the reference noise; mean and rstd also against the
    fp64 row formulas at the fp32 bound of an h-term sum."""
    g = gen(rows, h, 4)
    ids, pos, word, ptab, typ = embed_case(rows, h, g)
    w, b = params(h, g)
    h32 = torch.empty(rows, h, device="cuda")
    h16 = torch.empty(rows, h, dtype=BF16, device="cuda")
    mean, rstd = w.new_empty(rows), w.new_empty(rows)
    noise = K.EmbedNoise(R_MAG, SEED, SITE)
    K.roberta_embed_fwd(ids, pos, word, ptab, typ, w, b, EPS, h32, h16, mean, rstd, p, SEED,
                        R_DSITE, noise=noise)
    e = noisy_e(word, ids, ptab, pos, typ, rows, h, R_MAG)
    y, rm, rr = stats(K, e, w, b)
    want = torch.empty_like(y)
    K.dropout_f32(y, want, p, SEED, R_DSITE)
    assert same(mean, rm) and same(rstd, rr)
    assert same(h32, want) and same(h16, want.to(BF16))
    e64 = e.double()
    m64, v64 = e64.mean(1), e64.var(1, unbiased=False)
    tol = h * 2.0 ** -24 * e64.abs().max().item()
    assert float((mean.double() - m64).abs().max()) <= tol
    assert float((rstd.double() * torch.sqrt(v64 + EPS) - 1).abs().max()) <= h * 2.0 ** -23
    # and the noise is in it: the noise-free entry gives other statistics
    K.roberta_embed_fwd(ids, pos, word, ptab, typ, w, b, EPS, h32, h16, mean, rstd, p, SEED,
                        R_DSITE)
    assert not same(mean, rm)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("h", R_HS)
@pytest.mark.parametrize("rows", R_ROWS)
def test_roberta_embed_noise_bwd(K, rows, h, both):
    """test_roberta_gpu.test_roberta_embed_bwd's bars (de, dw, db within 2 x the existing
    LayerNorm backward's error against fp64, dtype within the sum of its rows' bounds) on e with
    the reference noise: the backward drew the forward's noise.  Against the noise-free e the
    same outputs are far off."""
    g = gen(rows, h, 5)
    ids, pos, word, ptab, typ = embed_case(rows, h, g)
    w, b = params(h, g)
    e = noisy_e(word, ids, ptab, pos, typ, rows, h, R_MAG)
    _, mean, rstd = stats(K, e, w, b)
    if both:
        dh = (torch.randint(-32, 33, (rows, h), generator=g).float() / 16).cuda()
        dhb = (torch.randint(-32, 33, (rows, h), generator=g).float() / 16).to(BF16).cuda()
        dy = dh + dhb.float()
    else:
        dh, dhb = torch.randn(rows, h, generator=g).to(BF16).float().cuda(), None
        dy = dh.clone()
    start = [torch.randn(h, generator=g).cuda() for _ in range(3)]
    rdx, rdw, rdb = ln_bwd64(e, mean, rstd, w, dy)
    ex = existing_bwd(K, e, mean, rstd, dy.to(BF16), w, start)
    base = dict(dx=rel(ex[0], rdx), dw=rel(ex[2], start[0].double().cpu() + rdw.cpu()),
                db=rel(ex[3], start[1].double().cpu() + rdb.cpu()))
    noise = K.EmbedNoise(R_MAG, SEED, SITE)

    def run(noise=noise, alias=False):
        src = dh.clone()
        de = src if alias else torch.full_like(e, float("nan"))
        dw, db, dt = (t.clone() for t in start)
        K.roberta_embed_bwd(ids, pos, word, ptab, typ, mean, rstd, w, src, de, dhb=dhb, dw=dw,
                            db=db, dtype=dt, p=0.0, seed=SEED, site=R_DSITE, noise=noise)
        return de, dw, db, dt

    de, dw, db, dt = run()
    got = dict(dx=rel(de, rdx), dw=rel(dw, start[0].double().cpu() + rdw.cpu()),
               db=rel(db, start[1].double().cpu() + rdb.cpu()))
    print(f"roberta_embed_noise_bwd rows {rows} h {h} both {both}: new {got}, existing {base}")
    for k in ("dx", "dw", "db"):
        assert got[k] <= 2 * base[k], (k, got[k], base[k])
    want = start[2].double().cpu() + rdx.sum(0).cpu()
    tol = rows * 2 * base["dx"] * rdx.abs().max().item() + \
        rows * 2.0 ** -24 * rdx.abs().sum(0).cpu() + 2.0 ** -22 * want.abs()
    assert bool(((dt.double().cpu() - want).abs() <= tol).all())
    assert all(same(a, c) for a, c in zip(run(), (de, dw, db, dt)))
    assert all(same(a, c) for a, c in zip(run(alias=True), (de, dw, db, dt)))
    # other noise (another site) or none: x-hat is another, far outside the bars
    for other in (None, K.EmbedNoise(R_MAG, SEED, SITE ^ (1 << 32))):
        de2, dw2, _, _ = run(noise=other)
        assert rel(de2, rdx) > 100 * base["dx"]
        assert rel(dw2, start[0].double().cpu() + rdw.cpu()) > 100 * base["dw"]


@pytest.mark.parametrize("p", (0.0, 0.1))
@pytest.mark.parametrize("rows,h", [(3, 72), (257, 128), (3, 1024), (257, 1032)])
def test_roberta_noise_path_at_mag_0_is_the_existing_entries(K, rows, h, p):
    g = gen(rows, h, 6)
    ids, pos, word, ptab, typ = embed_case(rows, h, g)
    w, b = params(h, g)
    dh = torch.randn(rows, h, generator=g).cuda()
    dhb = torch.randn(rows, h, generator=g).to(BF16).cuda()
    start = [torch.randn(h, generator=g).cuda() for _ in range(3)]

    def run(noise):
        h32 = torch.empty(rows, h, device="cuda")
        h16 = torch.empty(rows, h, dtype=BF16, device="cuda")
        mean, rstd = w.new_empty(rows), w.new_empty(rows)
        K.roberta_embed_fwd(ids, pos, word, ptab, typ, w, b, EPS, h32, h16, mean, rstd, p, SEED,
                            R_DSITE, noise=noise)
        de = torch.empty_like(dh)
        dw, db, dt = (t.clone() for t in start)
        K.roberta_embed_bwd(ids, pos, word, ptab, typ, mean, rstd, w, dh.clone(), de, dhb=dhb,
                            dw=dw, db=db, dtype=dt, p=p, seed=SEED, site=R_DSITE, noise=noise)
        return h32, h16, mean, rstd, de, dw, db, dt

    for a, c in zip(run(None), run(K.EmbedNoise(0.0, SEED, SITE))):
        assert same(a, c)


# ------------------------------------------------------------------ engine parity, alpha = 5
def requires_grad(P):
    return {k: v.clone().requires_grad_() for k, v in P.items()}


def grads_of(Pr):
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in Pr.items()}


def engine_step(eng, store, b):
    store.zero_grad()
    s = eng.forward(b, 1.0 / b.num_items)
    eng.backward(b)
    torch.cuda.synchronize()
    assert eng.cache == {}
    return s.item() / b.num_items


def noisy(eng, alpha=ALPHA, seed=SEED):
    eng.neftune_alpha, eng.dropout_seed = alpha, seed
    return eng


def batch_noise(eng, b, step=0):
    """float32 [T, hidden]: what the engine adds to the rows of Batch b at micro-step `step`."""
    h = eng.cfg.text.hidden
    return NR.noise(b.T, h, site0(eng, step), SEED, NR.mag_of(ALPHA, b.S_in, h))


def check_rel_grads(store, G, names=None):
    worst = ("", 0.0)
    for k, r in G.items():
        if names is not None and k not in names:
            continue
        err = ((store.g(k).cpu() - r).norm() / (r.norm() + 1e-20)).item()
        worst = max(worst, (k, err), key=lambda t: t[1])
        assert err < 3e-2, (k, err)
    print(f"worst gradient {worst[0]} {worst[1]:.2e}")


def oracle_with_noise(ocfg, P, bd, nz):
    """(bf16 loss, grads, fp32 loss) of oracle/model.py with nz hooked onto the input embedding."""
    Pr = requires_grad(P)
    with NR.embedding_hook(Pr["text.embed"], nz) as calls:
        ref = O.forward_loss(Pr, ocfg, bd, "bf16")
    assert calls == [1]
    ref.backward()
    with torch.no_grad():
        with NR.embedding_hook(P["text.embed"], nz):
            ref32 = O.forward_loss(P, ocfg, bd, "fp32").item()
    return ref.item(), grads_of(Pr), ref32


def noise_free_loss(eng, b):
    """The same engine's forward with the noise off (no gradients, the counter left alone)."""
    alpha, eng.neftune_alpha = eng.neftune_alpha, None
    loss = eng.forward(b, 1.0 / b.num_items, need_grad=False).item() / b.num_items
    eng.neftune_alpha = alpha
    return loss


@pytest.mark.parametrize("name,text_len,M,padded", [("tiny-lm", 130, 128, False),
                                                    ("tiny-lm", 64, 128, True),
                                                    ("tiny-llama", 130, 128, False),
                                                    ("tiny-mm", 47, 512, False)])
def test_engine_matches_the_noisy_oracle(name, text_len, M, padded):
    """test_parity_gpu.test_loss_and_grads' bars: loss within 1e-4 of the fp32 oracle and within
    1e-4 + |bf16 - fp32| of the bf16 oracle, every gradient within 3e-2 relative.

    The batch sizes come from the oracle's own bf16 error, as test_parity_gpu sizes
    tiny-clip-d80's batch: under alpha = 5 the residual stream carries noise several times the
    embedding scale, and the CPU oracle's |bf16 - fp32| at that test's 3 samples is 1.5e-4
    (tiny-mm) and 1.7e-4 (tiny-llama) — above the 1e-4 bar against fp32, which no bf16
    implementation then meets (measured on the 3-sample batches: GPU within 1.7e-5 of the bf16
    oracle and 2.5e-4 from fp32 for tiny-mm).  The gap falls as 1 / sqrt(samples): 2e-5 to 5e-5 at
    128 samples (tiny-lm, tiny-llama) and at 256 (tiny-mm, whose rows hold 47 text tokens), so
    tiny-mm takes 512."""
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.engine import Batch

    ocfg = oracle_cfg(C.get_config(name))
    P = O.init_params(ocfg, seed=0)
    bd = O.make_batch(ocfg, M, text_len, seed=1)
    cfg, store, eng = gpu_setup(name, P)
    noisy(eng)
    mask = None
    if padded:  # right-padded rows: the oracle runs the padded batch, labels under the pads off
        lens = [text_len if r % 4 == 0 else 9 + (37 * r) % (text_len - 9) for r in range(M)]
        mask = torch.zeros(M, text_len, dtype=torch.int64)
        for r, n in enumerate(lens):
            mask[r, :n] = 1
        bd = {"input_ids": bd["input_ids"], "labels": bd["labels"].masked_fill(mask == 0, -100)}
    b = Batch(cfg, bd["input_ids"], bd["labels"], bd.get("pixel_values"), store.device,
              attention_mask=mask)
    nz = batch_noise(eng, b)
    h = cfg.text.hidden
    if padded:  # the engine numbers the valid tokens; the pads get no noise (nothing reads them)
        assert b.T == sum(lens) and b.S_in == text_len
        full = np.zeros((M * text_len, h), np.float32)
        full[mask.reshape(-1).numpy() != 0] = nz
        nz = full
    ref, G, ref32 = oracle_with_noise(ocfg, P, bd, nz.reshape(M, -1, h))
    floor = abs(ref - ref32)
    plain = noise_free_loss(eng, b)
    loss = engine_step(eng, store, b)
    print(f"{name}: GPU {loss:.7f}, noisy oracle bf16 {ref:.7f} fp32 {ref32:.7f}, GPU noise-free "
          f"{plain:.7f}")
    assert abs(plain - ref) > 2 * (1e-4 + floor)  # an engine that ignored the noise fails the bar
    assert abs(loss - ref32) < 1e-4, (loss, ref32)
    assert abs(loss - ref) < 1e-4 + floor, (loss, ref, floor)
    check_rel_grads(store, G)
    assert eng.dropout_step == 1


def test_frozen_llava_matches_the_noisy_oracle():
    """test_parity_gpu.test_llava_pretrain_freeze's bars: loss within 2e-4 of the bf16 oracle,
    the projector's gradients within 3e-2, nothing else gets a gradient.  HF's hook adds the
    noise whatever is frozen."""
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.engine import Batch
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    cfg = C.get_config("tiny-llava-frozen")
    ocfg = oracle_cfg(cfg)
    P = O.init_params(ocfg, seed=0)
    bd = O.make_batch(ocfg, 3, 47, seed=1)
    tr = ManualTrainer(StepConfig(model="tiny-llava-frozen", scheduler="constant",
                                  neftune_noise_alpha=ALPHA),
                       AdamConfig(lr=1e-3), "cuda", model_cfg=cfg)
    tr.store.load(P)
    tr.store.refresh_shadow()
    eng = tr.engine
    assert eng.neftune_alpha == ALPHA
    eng.dropout_seed = SEED
    b = Batch(cfg, bd["input_ids"], bd["labels"], bd["pixel_values"], tr.store.device)
    nz = batch_noise(eng, b).reshape(3, -1, cfg.text.hidden)
    ref, G, _ = oracle_with_noise(ocfg, P, bd, nz)
    plain = noise_free_loss(eng, b)
    loss = engine_step(eng, tr.store, b)
    print(f"tiny-llava-frozen: GPU {loss:.7f}, noisy oracle {ref:.7f}, GPU noise-free {plain:.7f}")
    assert abs(plain - ref) > 10 * 2e-4
    assert abs(loss - ref) < 2e-4
    for k in P:
        if k.startswith("proj."):
            continue
        assert torch.count_nonzero(tr.store.g(k)) == 0, k
    check_rel_grads(tr.store, G, {k for k in P if k.startswith("proj.")})


def test_mamba_packed_matches_the_noisy_oracle():
    """test_mamba_gpu.test_loss_and_grads' bars (1e-4 + 3 sigma on the loss, 3e-2 on every
    gradient) on a packed batch: 2 rows of 40 holding documents of 22 + 18 and 37 + 3 tokens; the
    oracle runs the documents one by one with their rows of the noise, the magnitude is the
    flattened width's."""
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.engine import Batch, Engine
    from multimodal_llm_pretraining_amd.params import ParamStore

    cfg = C.get_config("tiny-mamba")
    h = cfg.text.hidden
    P = MO.init_params(cfg, seed=0)
    Bn, S, docs = 2, 40, [[22, 18], [37, 3]]
    bd = MO.make_batch(cfg, Bn, S, seed=1)
    pos = torch.stack([torch.cat([torch.arange(n) for n in row]) for row in docs])
    store = ParamStore(C.param_shapes(cfg), "cuda")
    store.load(P)
    store.refresh_shadow()
    eng = noisy(Engine(cfg, store))
    b = Batch(cfg, bd["input_ids"], bd["labels"], None, store.device, position_ids=pos)
    assert b.lens == [22, 18, 37, 3] and b.S_in == S and b.T == Bn * S
    nz = batch_noise(eng, b)
    assert NR.mag_of(ALPHA, S, h) != NR.mag_of(ALPHA, 37, h)
    ids, lab = bd["input_ids"].reshape(-1), bd["labels"].reshape(-1)
    cu = np.concatenate(([0], np.cumsum(b.lens)))

    def oracle(Pq, precision, with_noise=True):
        total = 0.0
        for d in range(len(b.lens)):
            rows = slice(int(cu[d]), int(cu[d + 1]))
            one = {"input_ids": ids[rows][None], "labels": lab[rows][None]}
            z = nz[rows][None] if with_noise else np.zeros_like(nz[rows][None])
            with NR.embedding_hook(Pq["text.embed"], z):
                total = total + MO.forward_loss(Pq, cfg, one, precision, num_items=b.num_items)
        return total

    Pr = requires_grad(P)
    ref = oracle(Pr, "bf16")
    ref.backward()
    G = grads_of(Pr)
    with torch.no_grad():
        ref32 = oracle(P, "fp32").item()
        plain = oracle(P, "bf16", with_noise=False).item()
    sigma = MO.bf16_sigma(P, cfg, Bn, S)
    loss = engine_step(eng, store, b)
    print(f"tiny-mamba packed: GPU {loss:.7f}, noisy oracle bf16 {ref.item():.7f} fp32 "
          f"{ref32:.7f}, noise-free {plain:.7f}, sigma {sigma:.3e}")
    assert abs(ref.item() - plain) > 10 * (1e-4 + 3 * sigma)
    assert abs(loss - ref.item()) < 1e-4 + 3 * sigma, (loss, ref.item(), ref32, sigma)
    check_rel_grads(store, G)


def test_roberta_matches_the_noisy_oracle():
    """test_roberta_gpu.test_loss_and_grads' bars: 1e-4 + 3 sigma on the loss, 3e-2 on every
    gradient — the embedding LayerNorm's and the type row's depend on the noise through x-hat."""
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.engine import Batch, Engine
    from multimodal_llm_pretraining_amd.params import ParamStore

    cfg = C.get_config("tiny-roberta")
    Bn, S, h = 4, 48, cfg.text.hidden
    P = RO.init_params(cfg, seed=0)
    bd = RO.make_batch(cfg, Bn, S, seed=1)
    bd["input_ids"][1, 20] = 1  # a pad id inside a row
    bd["labels"] = bd["input_ids"].clone()
    store = ParamStore(C.param_shapes(cfg), "cuda")
    store.load(P)
    store.refresh_shadow()
    eng = noisy(Engine(cfg, store))
    b = Batch(cfg, bd["input_ids"], bd["labels"], None, store.device)
    nz = batch_noise(eng, b).reshape(Bn, S, h)
    Pr = requires_grad(P)
    with NR.embedding_hook(Pr["text.embed"], nz) as calls:
        ref = RO.forward_loss(Pr, cfg, bd, "bf16")
    assert calls == [1]
    ref.backward()
    G = grads_of(Pr)
    with torch.no_grad():
        plain = RO.forward_loss(P, cfg, bd, "bf16").item()
    sigma = RO.bf16_sigma(P, cfg, Bn, S)
    loss = engine_step(eng, store, b)
    print(f"tiny-roberta: GPU {loss:.7f}, noisy oracle {ref.item():.7f}, noise-free {plain:.7f}, "
          f"sigma {sigma:.3e}")
    assert abs(ref.item() - plain) > 10 * (1e-4 + 3 * sigma)
    assert abs(loss - ref.item()) < 1e-4 + 3 * sigma, (loss, ref.item(), sigma)
    check_rel_grads(store, G)
    # the backward drew the forward's noise: with the noise off only in the backward the
    # embedding LayerNorm's gain gradient leaves the bar
    store.zero_grad()
    eng.forward(b, 1.0 / b.num_items)
    eng._noise = None
    eng.backward(b)
    r = G["text.embed_ln.weight"]
    assert ((store.g("text.embed_ln.weight").cpu() - r).norm() / r.norm()).item() > 3e-2


# ------------------------------------------------------------------ semantics, tiny-lm
@pytest.fixture(scope="module")
def lm():
    from multimodal_llm_pretraining_amd import config as C

    ocfg = oracle_cfg(C.get_config("tiny-lm"))
    P = O.init_params(ocfg, seed=0)
    return P, [O.make_batch(ocfg, 3, 40, seed=s) for s in (1, 2)]


def lm_engine(P, alpha=ALPHA, **attrs):
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg, store, eng = gpu_setup("tiny-lm", P)
    noisy(eng, alpha)
    for k, v in attrs.items():
        setattr(eng, k, v)
    return cfg, store, eng, lambda bd: Batch(cfg, bd["input_ids"], bd["labels"], None, store.device)


def test_same_seed_is_bitwise_and_steps_differ(lm):
    P, (bd, _) = lm
    runs = []
    for _ in range(2):
        _, store, eng, stage = lm_engine(P)
        b = stage(bd)
        l0 = engine_step(eng, store, b)
        g0 = store.grad.clone()
        l1 = engine_step(eng, store, b)
        runs.append((l0, g0, l1, store.grad.clone()))
        assert eng.dropout_step == 2
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2] and torch.equal(runs[0][3], runs[1][3])
    assert runs[0][0] != runs[0][2] and not torch.equal(runs[0][1], runs[0][3])
    _, store, eng, stage = lm_engine(P)
    eng.dropout_seed = SEED + 1
    assert engine_step(eng, store, stage(bd)) != runs[0][0]


def test_eval_and_preview(lm):
    P, (bd, _) = lm
    _, pstore, peng, stage = lm_engine(P, alpha=None)
    plain = engine_step(peng, pstore, stage(bd))
    assert peng.dropout_step == 0
    # eval: dropout_enabled off is the alpha-None step, bit for bit
    _, store, eng, stage = lm_engine(P, dropout_enabled=False)
    b = stage(bd)
    assert engine_step(eng, store, b) == plain and torch.equal(store.grad, pstore.grad)
    assert eng.dropout_step == 0
    # a forward without gradients in train mode previews the next training forward's noise
    eng.dropout_enabled = True
    pre = eng.forward(b, 1.0 / b.num_items, need_grad=False).item() / b.num_items
    assert eng.dropout_step == 0 and eng.cache == {}
    again = eng.forward(b, 1.0 / b.num_items, need_grad=False).item() / b.num_items
    assert again == pre and eng.dropout_step == 0
    got = engine_step(eng, store, b)
    assert got == pre and got != plain and eng.dropout_step == 1


def _trainer(P, alpha, sharding="", ac=False):
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    tr = ManualTrainer(StepConfig(model="tiny-lm", sharding=sharding, scheduler="constant",
                                  activation_checkpointing=ac, neftune_noise_alpha=alpha),
                       AdamConfig(lr=1e-3), "cuda")
    tr.store.load(P)
    tr.store.refresh_shadow()
    tr.engine.dropout_seed = SEED
    return tr


def _steps(tr, batches):
    losses = []
    for bd in batches:
        b = tr.stage(bd)
        losses.append(tr.train_step([b], b.num_items).item() / b.num_items)
    torch.cuda.synchronize()
    return losses


def _master(tr):
    if hasattr(tr.opt, "sync_master"):
        tr.opt.sync_master()
    return {k: v.detach().float().cpu() for k, v in tr.store.state_dict().items()}


def test_checkpointing_and_zero3_are_bitwise(lm):
    P, batches = lm
    ref = _trainer(P, ALPHA)
    assert ref.engine.neftune_alpha == ALPHA
    want = _steps(ref, batches)
    wm = _master(ref)
    for kw in (dict(ac=True), dict(sharding="zero_3")):
        tr = _trainer(P, ALPHA, **kw)
        assert _steps(tr, batches) == want, kw
        got = _master(tr)
        for n in wm:
            assert torch.equal(got[n], wm[n]), (kw, n)
    off = _trainer(P, None)
    assert _steps(off, batches) != want and off.engine.neftune_alpha is None


def _facade(P, overrides):
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.data import DummyTextModelingDataset
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining
    from multimodal_llm_pretraining_amd.train import TrainingClass

    cfg = C.get_config("tiny-lm")
    m = MMPTForPretraining(cfg)
    m.store.load(P)
    m.store.refresh_shadow()
    tc = TrainingClass(num_training_steps=4, micro_batch_size=3, gradient_accumulation_steps=1,
                       bf16=True, optimizer=torch.optim.AdamW, optimizer_kwargs={"lr": 1e-3},
                       scheduler_type="constant", max_grad_norm=0.0)
    ds = DummyTextModelingDataset(cfg.text.n_vocab, 40, 8)
    tr = tc.build_trainer(m, ds) if overrides is None else \
        tc.build_trainer(m, ds, hf_training_args_overrides=overrides)
    return m, tr


def test_two_steps_through_the_facade(lm):
    P, batches = lm

    def two(overrides):
        m, tr = _facade(P, overrides)
        losses = []
        for bd in batches:
            losses.append(tr.manual_training_step(m, bd).item())
            tr.manual_optimization_step(m)
        torch.cuda.synchronize()
        return m, tr, losses, m.store.master.clone()

    m, tr, noisy_losses, noisy_master = two({"neftune_noise_alpha": ALPHA})
    assert tr.core.step_cfg.neftune_noise_alpha == ALPHA and m.engine.neftune_alpha == ALPHA
    assert m.engine.dropout_step == 2
    runs = [two(o) for o in (None, {}, {"neftune_noise_alpha": None}, {"neftune_noise_alpha": 0})]
    for m_, _, losses, master in runs:
        assert m_.engine.neftune_alpha is None and m_.engine.dropout_step == 0
        assert losses == runs[0][2] and torch.equal(master, runs[0][3])
    assert all(a != b for a, b in zip(noisy_losses, runs[0][2]))
    assert not torch.equal(noisy_master, runs[0][3])
    # eval() on the module switches the noise off with the dropout
    m.eval()
    with torch.no_grad():
        a = m(**batches[0]).loss.item()
    m.engine.neftune_alpha = None
    with torch.no_grad():
        assert m(**batches[0]).loss.item() == a
    with pytest.raises(ValueError, match="neftune_noise_alpha"):
        _facade(P, {"neftune_noise_alpha": -1})


# ------------------------------------------------------------------ off by default
def test_default_step_launches_what_it_launched(lm, monkeypatch):
    """With the field absent the step calls mmpt_embed_fwd — no noise entry — and equals, bit
    for bit, the step in which the embedding is gathered by the noise-free call alone."""
    from multimodal_llm_pretraining_amd import _lib
    from multimodal_llm_pretraining_amd import kernels as Kmod
    from multimodal_llm_pretraining_amd.trainer import StepConfig

    P, (bd, _) = lm
    assert StepConfig().neftune_noise_alpha is None
    calls: dict = {}
    orig = _lib.call

    def counting(name, *a):
        calls[name] = calls.get(name, 0) + 1
        return orig(name, *a)

    _, store, eng, stage = lm_engine(P, alpha=None)
    assert eng.neftune_alpha is None
    b = stage(bd)
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "call", counting)
        loss = engine_step(eng, store, b)
    assert calls["mmpt_embed_fwd"] == 1
    assert not any("noise" in n for n in calls), sorted(calls)
    grad = store.grad.clone()
    # the parent's wrapper, restated: the gather without the noise argument
    seen = []

    def parent_embed_fwd(ids, table, out, img_map=None, img=None, noise=None):
        seen.append(noise)
        rows, h = out.shape
        orig("mmpt_embed_fwd", rows, h, ids.data_ptr(), table.data_ptr(), 0, 0, out.data_ptr(),
             Kmod._stream())

    _, store2, eng2, stage2 = lm_engine(P, alpha=None)
    with monkeypatch.context() as mp:
        mp.setattr(Kmod, "embed_fwd", parent_embed_fwd)
        loss2 = engine_step(eng2, store2, stage2(bd))
    assert seen == [None] and loss2 == loss and torch.equal(store2.grad, grad)
    # with the noise on the same step calls the noise entry instead, once
    calls.clear()
    _, store3, eng3, stage3 = lm_engine(P)
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "call", counting)
        loss3 = engine_step(eng3, store3, stage3(bd))
    assert calls.get("mmpt_embed_noise_fwd") == 1 and "mmpt_embed_fwd" not in calls
    assert loss3 != loss
