"""RoBERTa on the GPU: the K20 post-LN kernels (include/mmpt.h) against the existing LayerNorm /
dropout entries and an fp64 torch reference, then the engine, the trainer and the drop-in module
on `tiny-roberta` against the CPU oracle of tests/roberta_oracle.py.

Kernel bars.  Forward: add_layernorm_fwd and roberta_embed_fwd bitwise against the compositions
they replace (the row routine is mmpt_layernorm_f32_fwd's); mlm_ln_fwd, whose row comes from
bf16 loads, under the fp64 bound (2 × mmpt_layernorm_f32_fwd's error on the same row).  Backward fp32 outputs: err = max|out − ref| / max|ref| against an
fp64 reference of the stated arithmetic; the bar is 2 × the err mmpt_layernorm_bwd_ex shows
against the same reference on the same inputs, measured in the same test (both values are
printed).  So that the existing entry can read the same gradient, the gradient inputs are bf16-
representable: bf16 normals, or — where the new kernel adds an fp32 and a bf16 gradient — sixteenths
in [−2, 2], whose sum is exact in fp32 and in bf16.  bf16 outputs: the first rounding point may
differ from the reference's by one ulp, and only where the fp64 value lies within the fp32
outputs' allowed error of the rounding boundary; dropped elements are exactly zero.

Engine bars: test_vit_cls_gpu.py's — every gradient ‖g − g_ref‖/‖g_ref‖ < 3e-2 against the bf16
oracle, the loss within 1e-4 + 3σ of it (second optimizer step 3e-4 + 3σ), σ = the standard
deviation of (bf16 oracle − fp32 oracle) over 8 batch seeds at the test's own shape.
"""

import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roberta_oracle as RO  # noqa: E402
from test_attn_dropout_gpu import MaskedSDPA  # noqa: E402
from test_dropout_gpu import Masks  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ERR_ARG = "status -1"
EPS = 1e-5
SEED, SITE = 0x1234ABCD5, (7 << 32) | (3 << 4) | 1
ROWS, HS, PS = (1, 3, 257), (72, 128, 1024, 1032), (0.0, 0.1)
B, S = 4, 48  # the engine tests' batch (σ is measured at this shape)
# the kernel tests' (rows, h): ROWS x HS, then widths that reach MAXJ = 2, 12, 16 / PT = 2, 4 of the
# row kernels, masked lanes in the last vector (520) and more rows than backward workgroups (1029)
SHAPES = [(r, h) for r in ROWS for h in HS] + [(5, 512), (5, 520), (129, 3072), (5, 4096), (1029, 64)]


@pytest.fixture(scope="module")
def K():
    from multimodal_llm_pretraining_amd import kernels

    return kernels


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same(a, b) -> bool:
    return torch.equal(bits(a), bits(b))


def gen(rows, h, tag=0):
    return torch.Generator().manual_seed(7919 * rows + 31 * h + tag)


def strided(t: torch.Tensor, pad: int = 8) -> torch.Tensor:
    """A copy of the 2-D tensor with a leading dimension of h + pad."""
    buf = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def grid16(shape, g):
    """Sixteenths in [-2, 2]: sums of two are exact in fp32 and in bf16."""
    return torch.randint(-32, 33, shape, generator=g).float() / 16


def bf_ulp(x: torch.Tensor) -> torch.Tensor:
    """One bf16 ulp at |x| (fp64), 2^(e - 7)."""
    e = torch.floor(torch.log2(x.abs().double().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 7)


def ln_bwd64(x, mean, rstd, w, dy):
    """LayerNorm backward in fp64 from the given statistics: dx, dw, db."""
    x, mu, rs = x.double(), mean.double()[:, None], rstd.double()[:, None]
    w, dy = w.double(), dy.double()
    xh = (x - mu) * rs
    g = dy * w
    c1, c2 = (g * xh).mean(1, keepdim=True), g.mean(1, keepdim=True)
    return rs * (g - xh * c1 - c2), (dy * xh).sum(0), dy.sum(0)


def rel(out, ref) -> float:
    ref = ref.double().cpu()
    return ((out.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def first_rounding_ok(out_bf, ref64, allowed_abs):
    """out_bf vs bf16(f32(ref64)): equal, or one ulp apart with ref64 within `allowed_abs` of the
    rounding boundary between the two (the only way a bounded fp32 error changes the rounding)."""
    out = out_bf.double().cpu()
    ref64 = ref64.cpu()
    want = ref64.float().to(BF16).double()
    diff = out != want
    if not bool(diff.any()):
        return 0
    o, r, x = out[diff], want[diff], ref64[diff]
    if torch.is_tensor(allowed_abs):
        allowed_abs = allowed_abs[diff]
    assert bool(((o - r).abs() <= bf_ulp(r) * 1.0000001).all()), "more than one bf16 ulp"
    assert bool(((x - (o + r) / 2).abs() <= allowed_abs).all()), "differs away from a boundary"
    return int(diff.sum())


def colsum_ok(dsum, start, v) -> bool:
    """dsum == start + f32(bf16(Σ_rows f32(v))): the kernel's fp32 sum may sit within the
    standard bound rows · 2^-24 · Σ|v| of the exact one, so its bf16 rounding may be the
    neighbour of the exact sum's; then one fp32 add onto the start value."""
    v64 = v.double().cpu()
    col = v64.sum(0)
    want = start.double().cpu() + col.float().to(BF16).double()
    tol = bf_ulp(col) + v.shape[0] * 2.0 ** -24 * v64.abs().sum(0) + 1e-6 * want.abs()
    return bool(((dsum.double().cpu() - want).abs() <= tol).all())


def stats(K, s, w, b):
    rows, h = s.shape
    y, m, r = torch.empty_like(s), s.new_empty(rows), s.new_empty(rows)
    K.layernorm_f32_fwd(s, w, b, EPS, y, m, r)
    return y, m, r


def params(h, g):
    return (1 + 0.1 * torch.randn(h, generator=g)).cuda(), (0.1 * torch.randn(h, generator=g)).cuda()


# ------------------------------------------------------------------ add_layernorm_fwd
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("rows,h", SHAPES)
def test_add_layernorm_fwd(K, rows, h, p):
    g = gen(rows, h, 1)
    resid = (torch.randn(rows, h, generator=g) * 2 + 0.5).cuda()
    v = strided(torch.randn(rows, h, generator=g).to(BF16).cuda())
    w, b = params(h, g)
    s, y32 = torch.empty_like(resid), torch.empty_like(resid)
    y16 = strided(torch.zeros(rows, h, dtype=BF16, device="cuda"), 16)
    mean, rstd = resid.new_empty(rows), resid.new_empty(rows)
    K.add_layernorm_fwd(resid, v, w, b, EPS, s, y32, y16, mean, rstd, p, SEED, SITE)
    if p == 0:
        want_s = resid + v.float()
    else:
        dv = torch.empty(rows, h, dtype=BF16, device="cuda")
        K.dropout_bf16(v, dv, p, SEED, SITE)
        want_s = resid + dv.float()
        keep = K.dropout_mask(rows * h, p, SEED, SITE).view(rows, h).bool()
        assert same(s[~keep], resid[~keep])
        if rows * h > 1000:
            assert 0.05 < 1 - keep.float().mean().item() < 0.15
    assert same(s, want_s)
    ry, rm, rr = stats(K, s, w, b)
    assert same(y32, ry) and same(mean, rm) and same(rstd, rr)
    assert same(y16, y32.to(BF16))
    # the form that overwrites the residual stream
    r2 = resid.clone()
    y32b, y16b = torch.empty_like(resid), torch.empty(rows, h, dtype=BF16, device="cuda")
    m2, rs2 = resid.new_empty(rows), resid.new_empty(rows)
    K.add_layernorm_fwd(r2, v, w, b, EPS, r2, y32b, y16b, m2, rs2, p, SEED, SITE)
    assert same(r2, s) and same(y32b, y32) and same(y16b, y16) and same(m2, mean) and same(rs2, rstd)


# ------------------------------------------------------------------ add_layernorm_bwd
def existing_bwd(K, x, mean, rstd, dyb, w, start):
    """mmpt_layernorm_bwd_ex on the same inputs: dx, dx_bf16, dw, db, dsum (from `start`)."""
    rows, h = x.shape
    dx = torch.empty_like(x)
    dxb = torch.empty(rows, h, dtype=BF16, device="cuda")
    dw, db, ds = (t.clone() for t in start)
    K.layernorm_bwd(x, mean, rstd, dyb.contiguous(), w, dx, dw, db, dx_bf16=dxb, dsum=ds)
    return dx, dxb, dw, db, ds


@pytest.mark.parametrize("mode", ["dyb", "dy32", "both"])
@pytest.mark.parametrize("rows,h", SHAPES)
def test_add_layernorm_bwd(K, rows, h, mode):
    g = gen(rows, h, 2)
    s = (torch.randn(rows, h, generator=g) * 2 + 0.5).cuda()
    w, b = params(h, g)
    _, mean, rstd = stats(K, s, w, b)
    if mode == "dyb":
        dy32, dyb = None, strided(torch.randn(rows, h, generator=g).to(BF16).cuda())
        dy = dyb.float()
    elif mode == "dy32":
        dy32, dyb = grid16((rows, h), g).cuda(), None
        dy = dy32.clone()
    else:
        dy32, dyb = grid16((rows, h), g).cuda(), strided(grid16((rows, h), g).to(BF16).cuda())
        dy = dy32 + dyb.float()
    assert same(dy, dy.to(BF16).float())  # the existing entry reads the same gradient
    start = [torch.randn(h, generator=g).cuda() for _ in range(3)]
    rdx, rdw, rdb = ln_bwd64(s, mean, rstd, w, dy)
    ex = existing_bwd(K, s, mean, rstd, dy.to(BF16), w, start)
    base = dict(dx=rel(ex[0], rdx), dw=rel(ex[2], start[0].double().cpu() + rdw.cpu()),
                db=rel(ex[3], start[1].double().cpu() + rdb.cpu()))

    def run(p, alias=False):
        ds = dy32.clone() if alias else torch.full_like(s, float("nan"))
        dvb = strided(torch.zeros(rows, h, dtype=BF16, device="cuda"), 24)
        dw, db, dsum, dsum2 = (t.clone() for t in (*start, start[2]))
        K.add_layernorm_bwd(s, mean, rstd, w, ds, dvb, dy32=ds if alias else dy32, dyb=dyb, dw=dw,
                            db=db, dsum=dsum, dsum2=dsum2, p=p, seed=SEED, site=SITE)
        return ds, dvb, dw, db, dsum, dsum2

    ds, dvb, dw, db, dsum, dsum2 = run(0.0)
    got = dict(dx=rel(ds, rdx), dw=rel(dw, start[0].double().cpu() + rdw.cpu()),
               db=rel(db, start[1].double().cpu() + rdb.cpu()))
    print(f"add_layernorm_bwd rows {rows} h {h} {mode}: new {got}, mmpt_layernorm_bwd_ex {base}")
    for k in got:
        assert got[k] <= 2 * base[k], (k, got[k], base[k])
    # bf16 output: the rounding of the kernel's own fp32 value, so it can leave the reference's
    # rounding only where that value differs from the reference
    assert same(dvb, ds.to(BF16))
    allowed = 2 * base["dx"] * rdx.abs().max().item()
    first_rounding_ok(dvb, rdx, allowed)
    assert same(dsum, dsum2)
    assert colsum_ok(dsum, start[2], dvb)
    # two runs are bitwise equal; the in-place form over dy32 too
    again = run(0.0)
    assert all(same(a, c) for a, c in zip(again, (ds, dvb, dw, db, dsum, dsum2)))
    if dy32 is not None:
        al = run(0.0, alias=True)
        assert all(same(a, c) for a, c in zip(al, (ds, dvb, dw, db, dsum, dsum2)))
    # p = 0.1: the same fp32 results, the branch gradient masked by the forward's site
    ds1, dvb1, dw1, db1, dsum1, _ = run(0.1)
    assert same(ds1, ds) and same(dw1, dw) and same(db1, db)
    keep = K.dropout_mask(rows * h, 0.1, SEED, SITE).view(rows, h).bool()
    assert int(dvb1[~keep].count_nonzero()) == 0 and same(dvb1[~keep], torch.zeros_like(dvb1[~keep]))
    want1 = torch.empty(rows, h, dtype=BF16, device="cuda")
    K.dropout_bf16(dvb.contiguous(), want1, 0.1, SEED, SITE)
    assert same(dvb1, want1)
    assert colsum_ok(dsum1, start[2], dvb1)
    assert all(same(a, c) for a, c in zip(run(0.1), (ds1, dvb1, dw1, db1, dsum1)))


# ------------------------------------------------------------------ mlm_ln
def gelu_grad64(x):
    x = x.double()
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-x * x / 2) / math.sqrt(2 * math.pi)


@pytest.mark.parametrize("rows,h", SHAPES)
def test_mlm_ln(K, rows, h):
    g = gen(rows, h, 3)
    gl = strided(torch.randn(rows, h, generator=g).to(BF16).cuda())
    w, b = params(h, g)
    # forward: LayerNorm over f32(g) rounded to bf16.  The row routine is the source of
    # mmpt_layernorm_f32_fwd's, but hipcc fuses the squares differently when the row comes from
    # bf16 loads (rstd may move by an ulp), so this entry is held to the fp64 bound: 2 x the
    # error mmpt_layernorm_f32_fwd shows on the same row
    n16 = strided(torch.zeros(rows, h, dtype=BF16, device="cuda"), 16)
    mean, rstd = w.new_empty(rows), w.new_empty(rows)
    K.mlm_ln_fwd(gl, w, b, EPS, n16, mean, rstd)
    x = gl.float().contiguous()
    ry, rm, rr = stats(K, x, w, b)
    x64 = x.double().cpu()
    m64 = x64.mean(1)
    r64 = 1 / torch.sqrt(((x64 - m64[:, None]) ** 2).mean(1) + EPS)
    y64 = (x64 - m64[:, None]) * r64[:, None] * w.double().cpu() + b.double().cpu()
    fbase = dict(mean=rel(rm, m64), rstd=rel(rr, r64), y=rel(ry, y64))
    fgot = dict(mean=rel(mean, m64), rstd=rel(rstd, r64))
    print(f"mlm_ln_fwd rows {rows} h {h}: new {fgot}, mmpt_layernorm_f32_fwd {fbase}")
    assert fgot["mean"] <= 2 * fbase["mean"] and fgot["rstd"] <= 2 * fbase["rstd"], (fgot, fbase)
    first_rounding_ok(n16, y64, 2 * fbase["y"] * y64.abs().max().item())
    # backward
    dn = strided(torch.randn(rows, h, generator=g).to(BF16).cuda())
    pre = strided((torch.randn(rows, h, generator=g) * 1.5).to(BF16).cuda())
    start = [torch.randn(h, generator=g).cuda() for _ in range(3)]
    rdx, rdw, rdb = ln_bwd64(x, mean, rstd, w, dn.float())
    ex = existing_bwd(K, x, mean, rstd, dn, w, start)
    base = dict(dx=rel(ex[0], rdx), dw=rel(ex[2], start[0].double().cpu() + rdw.cpu()),
                db=rel(ex[3], start[1].double().cpu() + rdb.cpu()))

    def run(pre_):
        dpre = strided(torch.zeros(rows, h, dtype=BF16, device="cuda"), 24)
        dw, db, dsum = (t.clone() for t in start)
        K.mlm_ln_bwd(gl, mean, rstd, w, dn, pre_, dpre, dw=dw, db=db, dsum=dsum)
        return dpre, dw, db, dsum

    # gelu'(20) is exactly 1 in fp32: this call shows the first rounding point dg = bf16(LN'(dn))
    dg, dw, db, _ = run(torch.full((rows, h), 20.0, dtype=BF16, device="cuda"))
    got = dict(dw=rel(dw, start[0].double().cpu() + rdw.cpu()),
               db=rel(db, start[1].double().cpu() + rdb.cpu()))
    allowed = 2 * base["dx"] * rdx.abs().max().item()
    n1 = first_rounding_ok(dg, rdx, allowed)
    print(f"mlm_ln_bwd rows {rows} h {h}: new {got}, mmpt_layernorm_bwd_ex {base}; dg off the "
          f"reference's rounding at {n1} of {rows * h}")
    for k in got:
        assert got[k] <= 2 * base[k], (k, got[k], base[k])
    # the second rounding point over the kernel's own dg: bf16(dg · gelu'(pre)), gelu' to 2e-7
    # absolute (common.h) and one fp32 rounding of the product
    dpre, dw2, db2, dsum = run(pre)
    assert same(dw2, dw) and same(db2, db)
    prod = dg.double().cpu() * gelu_grad64(pre.cpu())
    first_rounding_ok(dpre, prod, dg.double().cpu().abs() * 4e-7 + prod.abs() * 2.0 ** -22)
    assert colsum_ok(dsum, start[2], dpre)
    assert all(same(a, c) for a, c in zip(run(pre), (dpre, dw2, db2, dsum)))


# ------------------------------------------------------------------ roberta_embed
def embed_case(rows, h, g, vocab=40, max_pos=300):
    ids = torch.randint(0, vocab, (rows,), generator=g)
    ids[::3] = 1  # pad ids inside the rows
    pos = torch.randint(0, max_pos, (rows,), generator=g)
    pos[ids == 1] = 1
    word = torch.randn(vocab, h, generator=g)
    ptab = torch.randn(max_pos, h, generator=g)
    word[1] = 0
    ptab[1] = 0
    typ = torch.randn(h, generator=g) * 0.5
    return tuple(t.cuda() for t in (ids, pos, word, ptab, typ))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("rows", ROWS)
def test_roberta_embed_fwd(K, rows, h, p):
    g = gen(rows, h, 4)
    ids, pos, word, ptab, typ = embed_case(rows, h, g)
    w, b = params(h, g)
    h32 = torch.empty(rows, h, device="cuda")
    h16 = torch.empty(rows, h, dtype=BF16, device="cuda")
    mean, rstd = w.new_empty(rows), w.new_empty(rows)
    K.roberta_embed_fwd(ids, pos, word, ptab, typ, w, b, EPS, h32, h16, mean, rstd, p, SEED, SITE)
    e = (word[ids] + typ) + ptab[pos]
    y, rm, rr = stats(K, e, w, b)
    want = torch.empty_like(y)
    K.dropout_f32(y, want, p, SEED, SITE)
    assert same(mean, rm) and same(rstd, rr)
    assert same(h32, want) and same(h16, want.to(BF16))
    if p > 0:
        keep = K.dropout_mask(rows * h, p, SEED, SITE).view(rows, h).bool()
        assert int(h32[~keep].count_nonzero()) == 0


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("rows", ROWS)
def test_roberta_embed_bwd(K, rows, h, both):
    g = gen(rows, h, 5)
    ids, pos, word, ptab, typ = embed_case(rows, h, g)
    w, b = params(h, g)
    e = ((word[ids] + typ) + ptab[pos]).contiguous()
    _, mean, rstd = stats(K, e, w, b)
    if both:
        dh, dhb = grid16((rows, h), g).cuda(), grid16((rows, h), g).to(BF16).cuda()
        dy = dh + dhb.float()
    else:
        dh, dhb = torch.randn(rows, h, generator=g).to(BF16).float().cuda(), None
        dy = dh.clone()
    start = [torch.randn(h, generator=g).cuda() for _ in range(3)]
    rdx, rdw, rdb = ln_bwd64(e, mean, rstd, w, dy)
    ex = existing_bwd(K, e, mean, rstd, dy.to(BF16), w, start)
    base = dict(dx=rel(ex[0], rdx), dw=rel(ex[2], start[0].double().cpu() + rdw.cpu()),
                db=rel(ex[3], start[1].double().cpu() + rdb.cpu()))

    def run(p, src=None, alias=False):
        src = dh.clone() if src is None else src.clone()
        de = src if alias else torch.full_like(e, float("nan"))
        dw, db, dt = (t.clone() for t in start)
        K.roberta_embed_bwd(ids, pos, word, ptab, typ, mean, rstd, w, src, de, dhb=dhb, dw=dw,
                            db=db, dtype=dt, p=p, seed=SEED, site=SITE)
        return de, dw, db, dt

    de, dw, db, dt = run(0.0)
    got = dict(dx=rel(de, rdx), dw=rel(dw, start[0].double().cpu() + rdw.cpu()),
               db=rel(db, start[1].double().cpu() + rdb.cpu()))
    print(f"roberta_embed_bwd rows {rows} h {h} both {both}: new {got}, mmpt_layernorm_bwd_ex {base}")
    for k in ("dx", "dw", "db"):
        assert got[k] <= 2 * base[k], (k, got[k], base[k])
    # Σ_rows de has no counterpart in the existing entry.  It sums the kernel's own de, so its
    # error is at most the rows' de errors added up (each within the bar above: 2 x the existing
    # entry's), the fp32 summation bound rows · 2^-24 · Σ|de|, and the add onto the start value
    want = start[2].double().cpu() + rdx.sum(0).cpu()
    tol = rows * 2 * base["dx"] * rdx.abs().max().item() + \
        rows * 2.0 ** -24 * rdx.abs().sum(0).cpu() + 2.0 ** -22 * want.abs()
    err = (dt.double().cpu() - want).abs()
    print(f"  dtype: worst error {err.max().item():.3e}, bound there {tol[err.argmax()].item():.3e}")
    assert bool((err <= tol).all())
    assert all(same(a, c) for a, c in zip(run(0.0), (de, dw, db, dt)))
    assert all(same(a, c) for a, c in zip(run(0.0, alias=True), (de, dw, db, dt)))
    if not both:  # dropout backward = the forward's map on the gradient, then the same kernel
        dropped = torch.empty_like(dh)
        K.dropout_f32(dh, dropped, 0.1, SEED, SITE)
        assert all(same(a, c) for a, c in zip(run(0.1), run(0.0, src=dropped)))


def test_embed_tables_take_the_long_position_segments(K):
    """B rows share each position id (segments of B rows, longer than the 1024 rows
    mmpt_embed_bwd_split splits at): the two scatter-adds against index_add in fp64."""
    rows, h, S_, vocab = 4 * 1100, 72, 4, 50
    g = gen(rows, h, 6)
    ids = torch.randint(0, vocab, (rows,), generator=g)
    pos = (torch.arange(rows) % S_) + 2
    pos[ids == 1] = 1
    de = torch.randn(rows, h, generator=g).cuda()
    for key, n in ((ids, vocab), (pos, S_ + 2)):
        table = torch.zeros(n, h, device="cuda")
        K.embed_bwd(K.embed_segments(key.cuda(), n, 1), de, table)
        sel = key != 1
        want = torch.zeros(n, h, dtype=F64).index_add_(0, key[sel], de.cpu().double()[sel])
        assert int(table[1].count_nonzero()) == 0
        assert rel(table, want) < 1e-5


# ------------------------------------------------------------------ argument errors
def test_argument_errors(K):
    from multimodal_llm_pretraining_amd import _lib

    rows = 2

    def bufs(h):
        f = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
        hb = lambda n: torch.zeros(n, dtype=BF16, device="cuda")  # noqa: E731
        return dict(x=f(rows * h + 4), s=f(rows * h + 4), y=f(rows * h), w=f(h + 4), b=f(h),
                    m=f(rows), r=f(rows), v=hb(rows * (h + 8) + 8), o=hb(rows * (h + 8) + 8),
                    q=hb(rows * (h + 8) + 8), dw=f(h), db=f(h), ds=f(h),
                    ids=torch.zeros(rows, dtype=torch.int64, device="cuda"),
                    tab=f(4 * h + 4),
                    ws=K.workspace(_lib.query("mmpt_add_layernorm_bwd_workspace_bytes", rows, h), slot=2))

    def p_(t, k, off=0):
        return t[k].data_ptr() + off

    def fwd(h, **kw):
        t = bufs(h)
        a = dict(resid=p_(t, "x"), v=p_(t, "v"), ld_v=h, s=p_(t, "s"), y16=p_(t, "o"), ld_y=h, p=0.0)
        a.update({k: (v(t) if callable(v) else v) for k, v in kw.items()})
        _lib.call("mmpt_add_layernorm_fwd", rows, h, EPS, a["resid"], a["v"], a["ld_v"], p_(t, "w"),
                  p_(t, "b"), a["s"], p_(t, "y"), a["y16"], a["ld_y"], p_(t, "m"), p_(t, "r"),
                  a["p"], 1, 1, 0)

    def bwd(h, **kw):
        t = bufs(h)
        a = dict(s=p_(t, "x"), dy32=p_(t, "s"), dyb=p_(t, "v"), ld_dyb=h, ds=p_(t, "y"),
                 dvb=p_(t, "o"), ld_dvb=h, dsum=None, dsum2=None, p=0.0)
        a.update({k: (v(t) if callable(v) else v) for k, v in kw.items()})
        _lib.call("mmpt_add_layernorm_bwd", rows, h, a["s"], p_(t, "m"), p_(t, "r"), p_(t, "w"),
                  a["dy32"], a["dyb"], a["ld_dyb"], a["ds"], a["dvb"], a["ld_dvb"], p_(t, "dw"),
                  p_(t, "db"), a["dsum"], a["dsum2"], a["p"], 1, 1, p_(t, "ws"), 0)

    def emb_f(h, **kw):
        t = bufs(h)
        a = dict(word=p_(t, "tab"), h16=p_(t, "o"))
        a.update({k: v(t) for k, v in kw.items()})
        _lib.call("mmpt_roberta_embed_fwd", rows, h, EPS, p_(t, "ids"), p_(t, "ids"), a["word"], 4,
                  p_(t, "tab"), 4, p_(t, "w"), p_(t, "w"), p_(t, "b"), p_(t, "y"), a["h16"],
                  p_(t, "m"), p_(t, "r"), 0.0, 1, 1, 0)

    def emb_b(h, **kw):
        t = bufs(h)
        a = dict(dh=p_(t, "s"), p=0.0)
        a.update({k: (v(t) if callable(v) else v) for k, v in kw.items()})
        _lib.call("mmpt_roberta_embed_bwd", rows, h, p_(t, "ids"), p_(t, "ids"), p_(t, "tab"), 4,
                  p_(t, "tab"), 4, p_(t, "w"), p_(t, "m"), p_(t, "r"), p_(t, "w"), a["dh"], None,
                  p_(t, "y"), p_(t, "dw"), p_(t, "db"), p_(t, "ds"), a["p"], 1, 1, p_(t, "ws"), 0)

    def mlm_f(h, **kw):
        t = bufs(h)
        a = dict(g=p_(t, "v"), ld_g=h)
        a.update({k: (v(t) if callable(v) else v) for k, v in kw.items()})
        _lib.call("mmpt_mlm_ln_fwd", rows, h, EPS, a["g"], a["ld_g"], p_(t, "w"), p_(t, "b"),
                  p_(t, "o"), h, p_(t, "m"), p_(t, "r"), 0)

    def mlm_b(h, **kw):
        t = bufs(h)
        a = dict(pre=p_(t, "q"), ld_pre=h)
        a.update({k: (v(t) if callable(v) else v) for k, v in kw.items()})
        _lib.call("mmpt_mlm_ln_bwd", rows, h, p_(t, "v"), h, p_(t, "m"), p_(t, "r"), p_(t, "w"),
                  p_(t, "q"), h, a["pre"], a["ld_pre"], p_(t, "o"), h, p_(t, "dw"), p_(t, "db"),
                  p_(t, "ds"), p_(t, "ws"), 0)

    for ok in (fwd, bwd, emb_f, emb_b, mlm_f, mlm_b):  # the well-formed calls pass
        ok(16)
    bwd(16, dy32=None), bwd(16, dyb=None, ld_dyb=0)
    torch.cuda.synchronize()
    bad = [lambda f=f: f(12) for f in (fwd, bwd, emb_f, emb_b, mlm_f, mlm_b)]      # h % 8 != 0
    bad += [lambda: fwd(16, resid=lambda t: p_(t, "x", 4)),                        # misaligned
            lambda: fwd(16, v=lambda t: p_(t, "v", 2)),
            lambda: fwd(16, y16=lambda t: p_(t, "o", 2)),
            lambda: bwd(16, s=lambda t: p_(t, "x", 4)),
            lambda: bwd(16, dvb=lambda t: p_(t, "o", 2)),
            lambda: bwd(16, dyb=lambda t: p_(t, "v", 2)),
            lambda: emb_f(16, word=lambda t: p_(t, "tab", 4)),
            lambda: emb_f(16, h16=lambda t: p_(t, "o", 2)),
            lambda: emb_b(16, dh=lambda t: p_(t, "s", 4)),
            lambda: mlm_f(16, g=lambda t: p_(t, "v", 2)),
            lambda: mlm_b(16, pre=lambda t: p_(t, "q", 2)),
            lambda: fwd(16, ld_v=8), lambda: fwd(16, ld_y=20),                     # ld < h, % 8
            lambda: bwd(16, ld_dvb=8), lambda: bwd(16, ld_dyb=20),
            lambda: mlm_f(16, ld_g=8), lambda: mlm_b(16, ld_pre=12),
            lambda: bwd(16, dy32=None, dyb=None),                                  # no gradient in
            lambda: bwd(16, dsum2=lambda t: p_(t, "ds")),                          # dsum2 w/o dsum
            lambda: fwd(16, p=1.0), lambda: bwd(16, p=-0.1), lambda: emb_b(16, p=1.5)]
    for call in bad:
        with pytest.raises(RuntimeError, match=ERR_ARG):
            call()
    # the tensor-level wrappers refuse before the library is entered
    z = torch.zeros(2, 16, device="cuda")
    zb = torch.zeros(2, 16, dtype=BF16, device="cuda")
    with pytest.raises(ValueError):
        K.add_layernorm_fwd(z, zb[:1], z[0], z[0], EPS, z, z, zb, z[0], z[0])
    with pytest.raises(TypeError):
        K.mlm_ln_fwd(z, z[0], z[0], EPS, zb, z[0], z[0])


# ------------------------------------------------------------------ engine
def pad_batch(cfg, seed=1):
    """B x S ids with the pad id at position 0, mid-row and twice in a row."""
    b = RO.make_batch(cfg, B, S, seed=seed)
    ids = b["input_ids"]
    ids[0, 0] = 1
    ids[1, 20] = 1
    ids[2, 30] = ids[2, 31] = 1
    b["labels"] = ids.clone()
    return b


@pytest.fixture(scope="module")
def ref():
    from multimodal_llm_pretraining_amd import config as C

    cfg = C.get_config("tiny-roberta")
    P = RO.init_params(cfg, seed=0)
    batch = pad_batch(cfg)
    loss16, G = RO.loss_and_grads(P, cfg, batch, "bf16")
    with torch.no_grad():
        loss32 = RO.forward_loss(P, cfg, batch, "fp32").item()
    sigma = RO.bf16_sigma(P, cfg, B, S)
    print(f"tiny-roberta B={B} S={S}: bf16 {loss16:.7f} fp32 {loss32:.7f} sigma {sigma:.3e}")
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


def run(cfg, P, batch, steps=1, mask=None, **kw):
    """([loss per micro-step], the store with the last step's gradients, the Batch)."""
    from multimodal_llm_pretraining_amd.engine import Batch

    store, eng = engine_for(cfg, P, **kw)
    b = Batch(cfg, batch["input_ids"], batch["labels"], None, store.device, attention_mask=mask)
    losses = []
    for _ in range(steps):
        store.zero_grad()
        s = eng.forward(b, 1.0 / b.num_items)
        eng.backward(b)
        losses.append(s.item() / b.num_items)
    torch.cuda.synchronize()
    assert eng.cache == {}
    return losses, store, b


def check_grads(store, G, cfg, S_=S):
    worst = ("", 0.0)
    for k, r in G.items():
        g = store.g(k).cpu()
        err = ((g - r).norm() / (r.norm() + 1e-20)).item()
        worst = max(worst, (k, err), key=lambda e: e[1])
        assert err < 3e-2, (k, err)
    print(f"worst gradient {worst[0]} {worst[1]:.2e}")
    V = cfg.text.n_vocab
    assert int(store.g("text.embed")[V:].count_nonzero()) == 0
    assert int(store.g("text.mlm.bias")[V:].count_nonzero()) == 0
    gp = store.g("text.pos_embed")
    assert int(gp[1].count_nonzero()) == 0 and int(gp[S_ + 2:].count_nonzero()) == 0
    assert int(gp[0].count_nonzero()) == 0


def test_loss_and_grads(ref):
    (loss,), store, b = run(ref["cfg"], ref["P"], ref["batch"])
    sigma = ref["sigma"]
    print(f"GPU loss {loss:.7f} (bf16 oracle {ref['loss16']:.7f}, fp32 {ref['loss32']:.7f}), "
          f"sigma {sigma:.3e}")
    assert b.num_items == B * S and b.loss_rows is None
    assert abs(loss - ref["loss16"]) < 1e-4 + 3 * sigma, (loss, ref["loss16"], ref["loss32"], sigma)
    check_grads(store, ref["G"], ref["cfg"])


def test_mlm_batch_runs_the_head_on_the_labelled_rows(ref, K):
    cfg, P = ref["cfg"], ref["P"]
    bd = {k: v.clone() for k, v in ref["batch"].items()}
    g = torch.Generator().manual_seed(11)
    bd["labels"][torch.rand(B, S, generator=g) >= 0.15] = -100
    bd["labels"][3] = -100  # a row without any label
    n = int((bd["labels"] != -100).sum())
    assert 0 < n < 0.3 * B * S
    seen = []
    gemm = K.gemm

    def spy(a, b, out, **kw):
        seen.append(tuple(out.shape))
        return gemm(a, b, out, **kw)

    K.gemm = spy
    try:
        (loss,), store, bt = run(cfg, P, bd)
    finally:
        K.gemm = gemm
    V, h = cfg.text.vocab, cfg.text.hidden
    assert bt.num_items == n and bt.loss_rows.numel() == n
    assert (n, V) in seen and (B * S, V) not in seen  # the decoder ran on the compacted rows
    assert seen.count((n, h)) >= 3 and (V, h) in seen  # the head dense, its dX, dn; the tied dW
    want, G = RO.loss_and_grads(P, cfg, bd, "bf16")  # every row, the rest at -100
    print(f"15% labelled ({n} rows): GPU {loss:.7f}, bf16 oracle {want:.7f}")
    # σ was measured on 192 labelled rows; n rows average n/192 as many terms
    assert abs(loss - want) < 1e-4 + 3 * ref["sigma"] * math.sqrt(B * S / n), (loss, want)
    check_grads(store, G, cfg)


def test_right_padded_batch(ref):
    cfg, P, bd = ref["cfg"], ref["P"], ref["batch"]
    lens = (48, 17, 1, 33)
    mask = torch.zeros(B, S, dtype=torch.int64)
    for r, n in enumerate(lens):
        mask[r, :n] = 1
    (loss,), store, bt = run(cfg, P, bd, mask=mask)
    assert bt.T == sum(lens) and bt.num_items == sum(lens) and bt.max_len == 48
    want, G = RO.loss_and_grads(P, cfg, bd, "bf16", lens=list(lens))
    print(f"padded {lens}: GPU {loss:.7f}, bf16 oracle run per sequence {want:.7f}")
    assert abs(loss - want) < 1e-4 + 3 * ref["sigma"] * math.sqrt(B * S / sum(lens)), (loss, want)
    check_grads(store, G, cfg)


def masked_oracle(K, monkeypatch, cfg, P, bd, seed, precision="bf16"):
    """The oracle fed the engine's own masks: hidden dropout through test_dropout_gpu.Masks,
    attention-probability dropout through a patched scaled_dot_product_attention."""
    t = cfg.text
    sdpa = MaskedSDPA(K, seed, 0, [(t.attn_dropout, 1 + i, 0) for i in range(t.layers)])
    with monkeypatch.context() as mp:
        mp.setattr(F, "scaled_dot_product_attention", sdpa)
        loss, G = RO.loss_and_grads(P, cfg, bd, precision, drop=Masks(K, cfg, seed, 0))
    assert sdpa.n == t.layers
    return loss, G


def test_dropout_against_masked_oracle(ref, K, monkeypatch):
    from multimodal_llm_pretraining_amd import config as C

    cfg = C.get_config("tiny-roberta-drop")
    P, bd = ref["P"], ref["batch"]
    want, G = masked_oracle(K, monkeypatch, cfg, P, bd, 1234)
    losses, store, _ = run(cfg, P, bd, steps=2, seed=1234)
    (again,), first, _ = run(cfg, P, bd, seed=1234)
    run_g = first.g
    print(f"dropout: GPU {losses[0]:.7f}, masked bf16 oracle {want:.7f}, p = 0 {ref['loss16']:.7f}")
    assert abs(losses[0] - want) < 1e-4 + 3 * ref["sigma"], (losses[0], want)
    # and the masks did something: against the p = 0 oracle's gradients the same bar fails widely
    unmasked = max(((store_g.cpu() - r).norm() / (r.norm() + 1e-20)).item()
                   for store_g, r in ((run_g(k), ref["G"][k]) for k in G))
    assert unmasked > 0.1 and losses[0] != ref["loss16"], unmasked
    assert losses[1] != losses[0]  # the next micro-step draws other masks
    assert again == losses[0]  # the same seed and step: bitwise
    check_grads(first, G, cfg)
    # eval() is the dropout-free model, bit for bit
    from multimodal_llm_pretraining_amd.engine import Batch

    (plain,), pstore, _ = run(ref["cfg"], P, bd)
    store2, eng = engine_for(cfg, P)
    eng.dropout_enabled = False
    bt = Batch(cfg, bd["input_ids"], bd["labels"], None, store2.device)
    ev = eng.forward(bt, 1.0 / bt.num_items).item() / bt.num_items
    eng.backward(bt)
    assert ev == plain and same(store2.grad, pstore.grad) and eng.dropout_step == 0


@pytest.mark.parametrize("name", ["tiny-roberta", "tiny-roberta-drop"])
def test_checkpointing_is_bitwise(ref, name):
    from multimodal_llm_pretraining_amd import config as C

    cfg = C.get_config(name)
    la, a, _ = run(cfg, ref["P"], ref["batch"], steps=2, seed=1234)
    lb, b, _ = run(cfg, ref["P"], ref["batch"], steps=2, seed=1234, checkpointing=True)
    assert la == lb and same(a.grad, b.grad)


@pytest.mark.parametrize("sharding", ["", "zero_1"])
def test_two_adam_steps(ref, sharding):
    """The recipe's optimizer (Adam β (0.9, 0.98), linear schedule; HF Trainer's effective weight
    decay 0) through trainer.ManualTrainer, data parallel (world 1) and ZeRO-1."""
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    cfg, P, sigma = ref["cfg"], ref["P"], ref["sigma"]
    batches = [ref["batch"], pad_batch(cfg, seed=2)]
    lrs = [4e-4, 3e-4]  # linear, no warmup, 4 steps
    want, _ = RO.train_steps(P, cfg, batches, lrs, "bf16")
    tr = ManualTrainer(StepConfig(model="tiny-roberta", scheduler="linear", num_warmup_steps=0,
                                  num_training_steps=4, sharding=sharding),
                       AdamConfig(lr=4e-4, betas=(0.9, 0.98), weight_decay=0.0, adamw=False), "cuda")
    tr.store.load(P)
    tr.store.refresh_shadow()
    got = []
    for bd in batches:
        b = tr.stage(bd)
        got.append(tr.train_step([b], b.num_items).item() / b.num_items)
    print(f"two Adam steps ({sharding or 'ddp'}): GPU {got}, bf16 oracle {want}, sigma {sigma:.3e}")
    assert abs(got[0] - want[0]) < 1e-4 + 3 * sigma, (got, want, sigma)
    assert abs(got[1] - want[1]) < 3e-4 + 3 * sigma, (got, want, sigma)
    assert got[1] != got[0]
    V = cfg.text.n_vocab  # the padding rows stay exactly zero through the update
    assert int(tr.store.p("text.embed")[V:].count_nonzero()) == 0
    assert int(tr.store.p("text.mlm.bias")[V:].count_nonzero()) == 0
    assert int(tr.store.p("text.pos_embed")[1].count_nonzero()) == 0


@pytest.mark.parametrize("sharding", ["", "zero_1"])
def test_offloaded_optimizer_matches_device_adam(ref, sharding):
    """Optimizer offload touches the flat buffers and gates each unit's first forward on its host
    update (the MLM head is a unit of its own): first-step losses equal, later ones within the
    project's 1e-4 (tests/test_sharding_gpu.py's offload bar)."""
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig
    from multimodal_llm_pretraining_amd.zero3 import unit_of

    assert unit_of("text.mlm.dense.weight") == unit_of("text.mlm.bias") == "text.mlm"
    assert unit_of("text.mlm.ln.weight") is None and unit_of("text.pos_embed") is None
    cfg, P = ref["cfg"], ref["P"]
    batches = [ref["batch"], pad_batch(cfg, seed=2), pad_batch(cfg, seed=3)]
    got = {}
    for offload in (False, True):
        tr = ManualTrainer(StepConfig(model="tiny-roberta", scheduler="constant", offload=offload,
                                      sharding=sharding),
                           AdamConfig(lr=4e-4, betas=(0.9, 0.98), adamw=False), "cuda")
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


@pytest.mark.parametrize("sharding", ["zero_2", "zero_3"])
def test_unit_sharding_is_refused(sharding):
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    with pytest.raises(NotImplementedError, match="roberta"):
        ManualTrainer(StepConfig(model="tiny-roberta", sharding=sharding), AdamConfig(), "cuda")


def test_dropin_module(ref):
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining

    cfg, P, bd = ref["cfg"], ref["P"], ref["batch"]
    (loss,), eng_store, _ = run(cfg, P, bd)
    m = MMPTForPretraining(cfg)
    assert (m.config.hidden_size, m.config.vocab_size, m.config.model_type) == (128, 515, "mmpt")
    assert m.config.text_config.model_type == "roberta"
    assert set(m.state_dict()) == set(C.param_shapes(cfg))  # the store's names
    m.store.load(P)
    m.store.refresh_shadow()
    out = m(input_ids=bd["input_ids"], labels=bd["labels"], attention_mask=bd["attention_mask"])
    assert out.loss.item() == pytest.approx(loss, abs=1e-6)
    out.loss.backward()
    assert m.engine.cache == {}
    for name, p in m.named_parameters():
        assert p.grad is not None and p.grad.data_ptr() == m.store.g(name).data_ptr(), name
        assert same(p.grad, eng_store.g(name)), name
    with torch.no_grad():
        ev = m(input_ids=bd["input_ids"], labels=bd["labels"])
    assert m.engine.cache == {} and ev.loss.item() == pytest.approx(loss, abs=1e-6)
    with pytest.raises(ValueError, match="max_positions"):
        m(input_ids=torch.zeros(2, 65, dtype=torch.int64),
          labels=torch.zeros(2, 65, dtype=torch.int64))


def test_harness_trains_two_steps(ref):
    """TrainingClass.build_trainer → benchmarking.ManualTrainer → estimate_step_time, the path
    scripts/benchmark.py drives, over the dummy text dataset."""
    from multimodal_llm_pretraining_amd.benchmarking import estimate_step_time
    from multimodal_llm_pretraining_amd.data import DummyTextModelingDataset
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining
    from multimodal_llm_pretraining_amd.train import TrainingClass

    cfg = ref["cfg"]
    ds = DummyTextModelingDataset(cfg.text.n_vocab, S, 32)
    kw = dict(num_training_steps=4, micro_batch_size=4, gradient_accumulation_steps=1, bf16=True,
              optimizer=torch.optim.Adam,
              optimizer_kwargs={"lr": 4e-4, "betas": (0.9, 0.98), "weight_decay": 0.01},
              scheduler_type="linear", scheduler_kwargs={"num_warmup_steps": 1}, max_grad_norm=0.0)
    m = MMPTForPretraining(cfg)
    tr = TrainingClass(**kw).build_trainer(m, ds)
    before = m.store.w("text.mlm.dense.weight").clone()
    assert estimate_step_time(tr, 4, 8, 1) > 0
    torch.cuda.synchronize()
    assert not torch.equal(m.store.w("text.mlm.dense.weight"), before)
    m = MMPTForPretraining(cfg)
    with pytest.raises(NotImplementedError, match="roberta"):
        TrainingClass(**kw, zero_stage="2").build_trainer(m, ds)
