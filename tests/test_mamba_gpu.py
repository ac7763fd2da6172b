"""Mamba on the GPU: the K22 kernels (include/mmpt.h) against fp64 references, then the engine, the
trainer and the drop-in module on `tiny-mamba` against the "fused" CPU oracle of
tests/mamba_oracle.py.

Kernel bars.  Operands are bf16-exact where the kernel reads bf16; the reference is fp64 on the CPU
from the same rounded operands, u = 2^-24, A = the same expression over absolute values.

Causal conv.  |got − ref| <= 2^-8 |ref| + 16 u A for the forward and dx, 2^-8 |ref| + N u A with
N = B·L for dw and db (the backward's du is the fp32 sum of its two gradient inputs, one more
rounding inside the 16 u).  The op rounds to bf16 twice (c, then silu(c); dc, then dx), so the
reference applies the first rounding too, and where the fp64 value of the first result lies within
the kernel's fp32 evaluation error of a bf16 tie (16 u A_c for c; 16 u |du| σ(1 + |c|(1 − σ)) for
dc, which covers the cancellation in silu' near c = −1.28) either neighbour is a correct first
rounding: there, and only there, the bar grows by the effect of that one-ulp choice on the output.
`+=` is checked bitwise against start + (the result from zero), a second run gives the same bits,
and sequence b alone has the bits of sequence b in the batch.

Selective scan, y.  |got − ref| <= 2^-8 |ref| + n u A, n = (6 + 2 max|δ a|) L + 16, computed from
the operands: per step one exp (library expf, 1 ulp; its argument δ a carries the roundings of
softplus — expf 1 ulp, log1pf 2 ulp — and of the product, about 3 |x| u), one multiply and one add.
The kernel joins chunks with exp(a Σδ), Σδ summed in fp64 and rounded once, so a chunk of c steps
costs two roundings of an argument of at most c max|δ a|: within the c steps' allowance.

Scan backward.  Each term of a gradient is a product of a recomputed state h (error n u A_h, as in
the forward), an adjoint μ that runs the same recurrence backwards (n u A_μ) and a few more
factors (softplus' and silu', 16 u in all), summed over S terms: n_b = 2 n + S + 16 with S = N for
du, dz and ddt_raw, I for dB and dC, B·L for dA_log, dD and ddt_bias.  bf16 outputs are held to
2^-8 |ref| + n_b u A, fp32 outputs (summed from unrounded values) to n_b u A alone.  A uses
σ(1 + |z|(1 − σ)) for silu'(z).  Bitwise: batch independence, a second run, and the prefix
property — the chunk length does not depend on L, so the first L' outputs of a longer run have the
bits of a length-L' run for L' a multiple of the chunk.
"""

import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ERR_ARG = "status -1"
U = 2.0 ** -24
CONV_SHAPES = [(1, 1, 8), (2, 3, 8), (3, 4, 24), (2, 5, 40), (2, 65, 192), (3, 130, 64), (1, 257, 8)]


@pytest.fixture(scope="module")
def K():
    from multimodal_llm_pretraining_amd import kernels

    return kernels


def sid(s):
    return "x".join(map(str, s))


def same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def rb(t):
    """fp64 -> the nearest bf16, back in fp64"""
    return t.to(F32).to(BF16).double()


def worst(got, ref, a, n, r=2.0 ** -8, extra=None):
    err = (got.double().cpu() - ref).abs()
    bound = r * ref.abs() + n * U * a
    if extra is not None:
        bound = bound + extra
    return (err / bound.clamp_min(1e-300)).max().item()


def nan16(*shape):
    return torch.full(shape, float("nan"), dtype=BF16, device="cuda")


# ------------------------------------------------------------------ causal conv
_conv = {}


def sig64(c):
    return torch.sigmoid(c)


def conv_case(shape):
    """Seeded operands of one shape and their fp64 results, computed once and shared."""
    if shape in _conv:
        return _conv[shape]
    B, L, C = shape
    g = torch.Generator().manual_seed(7919 * B + 104729 * L + C)
    xz = torch.randn(B * L, 2 * C, generator=g).to(BF16)  # x is the first half of [x | z]
    w = (torch.randn(4, C, generator=g) * 0.4).to(BF16)
    bias = (torch.randn(C, generator=g) * 0.3).to(BF16)
    du = torch.randn(B * L, C, generator=g).to(BF16)
    du2 = torch.randn(B * L, C, generator=g).to(BF16)  # u's second gradient (x_proj's)
    x = xz[:, :C].double().view(B, L, C)
    w64, b64, du64 = w.double(), bias.double(), (du.double() + du2.double()).view(B, L, C)
    xp = F.pad(x, (0, 0, 3, 0))
    taps = [xp[:, k:k + L] for k in range(4)]  # taps[k][:, t] = x[:, t-3+k]
    c64 = sum(w64[k] * taps[k] for k in range(4)) + b64
    a_c = sum(w64[k].abs() * taps[k].abs() for k in range(4)) + b64.abs()
    cb, clo, chi = rb(c64), rb(c64 - 16 * U * a_c), rb(c64 + 16 * U * a_c)
    silu = lambda c: c * sig64(c)  # noqa: E731
    fwd = silu(cb)
    amb_fwd = (silu(chi) - silu(clo)).abs()

    def dsilu(c):
        s = sig64(c)
        return s * (1 + c * (1 - s))

    def dsilu_abs(c):
        s = sig64(c)
        return s * (1 + c.abs() * (1 - s))

    cands = []
    for c in (cb, clo, chi):
        v, e = du64 * dsilu(c), 16 * U * du64.abs() * dsilu_abs(c)
        cands += [rb(v - e), rb(v + e)]
    dcb = rb(du64 * dsilu(cb))
    amb_dc = torch.stack(cands).amax(0) - torch.stack(cands).amin(0)
    dcp, ambp = F.pad(dcb, (0, 0, 0, 3)), F.pad(amb_dc, (0, 0, 0, 3))
    back = [(dcp[:, 3 - k:3 - k + L], ambp[:, 3 - k:3 - k + L]) for k in range(4)]  # dc[:, t+3-k]
    dx = sum(w64[k] * back[k][0] for k in range(4))
    a_dx = sum(w64[k].abs() * back[k][0].abs() for k in range(4))
    amb_dx = sum(w64[k].abs() * back[k][1] for k in range(4))
    dw = torch.stack([(dcb * taps[k]).sum((0, 1)) for k in range(4)])
    a_dw = torch.stack([(dcb.abs() * taps[k].abs()).sum((0, 1)) for k in range(4)])
    amb_dw = torch.stack([(amb_dc * taps[k].abs()).sum((0, 1)) for k in range(4)])
    case = dict(xz=xz, w=w, bias=bias, du=du, du2=du2, fwd=fwd.view(B * L, C), a_fwd=a_c.view(B * L, C),
                amb_fwd=amb_fwd.view(B * L, C), dx=dx.view(B * L, C), a_dx=a_dx.view(B * L, C),
                amb_dx=amb_dx.view(B * L, C), dw=dw, a_dw=a_dw, amb_dw=amb_dw, db=dcb.sum((0, 1)),
                a_db=dcb.abs().sum((0, 1)), amb_db=amb_dc.sum((0, 1)))
    _conv[shape] = case
    return case


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=sid)
def test_causal_conv1d_fwd(K, shape):
    B, L, C = shape
    t = conv_case(shape)
    xz, w, bias = t["xz"].cuda(), t["w"].cuda(), t["bias"].cuda()
    x = xz[:, :C]
    u = nan16(B * L, C)
    K.causal_conv1d_fwd(x, w, bias, u, L)
    wr = worst(u, t["fwd"], t["a_fwd"], 16, extra=t["amb_fwd"])
    print(f"causal_conv1d_fwd {shape}: worst err / bound {wr:.3f}")
    assert wr <= 1.0
    again = nan16(B * L, C)
    K.causal_conv1d_fwd(x, w, bias, again, L)
    assert same(again, u)
    for b in range(B):  # a read across a sequence boundary shows here
        one = nan16(L, C)
        K.causal_conv1d_fwd(x[b * L:(b + 1) * L], w, bias, one, L)
        assert same(one, u[b * L:(b + 1) * L]), b


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=sid)
def test_causal_conv1d_bwd(K, shape):
    B, L, C = shape
    t = conv_case(shape)
    xz, w, bias, du = t["xz"].cuda(), t["w"].cuda(), t["bias"].cuda(), t["du"].cuda()
    du2 = t["du2"].cuda()
    x = xz[:, :C]
    dxz = nan16(B * L, 2 * C)  # dx lands in the first half of d[x | z]
    dx = dxz[:, :C]
    dw0, db0 = torch.zeros(4, C, device="cuda"), torch.zeros(C, device="cuda")
    K.causal_conv1d_bwd(x, w, bias, du, dx, dw0, db0, L, du2=du2)
    n = B * L
    wx = worst(dx, t["dx"], t["a_dx"], 16, extra=t["amb_dx"])
    ww = worst(dw0, t["dw"], t["a_dw"], n, extra=t["amb_dw"])
    wb = worst(db0, t["db"], t["a_db"], n, extra=t["amb_db"])
    print(f"causal_conv1d_bwd {shape}: worst err / bound dx {wx:.3f} dw {ww:.3f} db {wb:.3f}")
    assert wx <= 1.0 and ww <= 1.0 and wb <= 1.0
    assert torch.isnan(dxz[:, C:].float()).all()  # nothing written past ld's first C columns
    assert same(dw0, dw0.to(BF16).float()) and same(db0, db0.to(BF16).float())
    g = torch.Generator().manual_seed(6)
    sw, sb = torch.randn(4, C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
    dw1, db1 = sw.clone(), sb.clone()
    dx1 = nan16(B * L, C)
    K.causal_conv1d_bwd(x, w, bias, du, dx1, dw1, db1, L, du2=du2)
    assert same(dw1, sw + dw0) and same(db1, sb + db0)  # += of the bf16-rounded sums
    assert same(dx1, dx)  # and a second run gives the same bits
    for b in range(B):
        one = nan16(L, C)
        K.causal_conv1d_bwd(x[b * L:(b + 1) * L], w, bias, du[b * L:(b + 1) * L], one,
                            torch.zeros(4, C, device="cuda"), torch.zeros(C, device="cuda"), L,
                            du2=du2[b * L:(b + 1) * L])
        assert same(one, dx[b * L:(b + 1) * L]), b
    # no second gradient is a second gradient of zeros
    outs = []
    for second in (None, torch.zeros_like(du2)):
        o = [nan16(B * L, C), torch.zeros(4, C, device="cuda"), torch.zeros(C, device="cuda")]
        K.causal_conv1d_bwd(x, w, bias, du, *o, L, du2=second)
        outs.append(o)
    assert all(same(p, q) for p, q in zip(*outs))


def test_causal_conv1d_argument_errors(K):
    C, L = 16, 4
    x, u = torch.zeros(2 * L, C, dtype=BF16, device="cuda"), nan16(2 * L, C)
    w, bias = torch.zeros(4, C, dtype=BF16, device="cuda"), torch.zeros(C, dtype=BF16, device="cuda")
    dw, db = torch.zeros(4, C, device="cuda"), torch.zeros(C, device="cuda")
    wide = torch.zeros(2 * L, C + 8, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError, match=ERR_ARG):  # a pointer 8 bytes off a 16-byte boundary
        K.causal_conv1d_fwd(wide[:, 4:4 + C], w, bias, u, L)
    with pytest.raises(RuntimeError, match=ERR_ARG):
        K.causal_conv1d_bwd(x, w, bias, x, wide[:, 4:4 + C], dw, db, L)
    odd = torch.zeros(2 * L, C + 4, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError, match=ERR_ARG):  # a leading dimension that is no multiple of 8
        K.causal_conv1d_fwd(odd[:, :C], w, bias, u, L)
    with pytest.raises(RuntimeError, match=ERR_ARG):
        K.causal_conv1d_bwd(x, w, bias, odd[:, :C], u, dw, db, L)
    x12, w12 = torch.zeros(2 * L, 12, dtype=BF16, device="cuda"), torch.zeros(4, 12, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError, match=ERR_ARG):  # C % 8
        K.causal_conv1d_fwd(x12, w12, torch.zeros(12, dtype=BF16, device="cuda"), nan16(2 * L, 12), L)
    with pytest.raises(RuntimeError, match="GPU"):
        K.causal_conv1d_fwd(x.cpu(), w, bias, u, L)
    with pytest.raises(RuntimeError, match="GPU"):
        K.causal_conv1d_bwd(x, w, bias, x, u, dw.cpu(), db, L)
    with pytest.raises(ValueError):  # rows that are no whole number of sequences
        K.causal_conv1d_fwd(x, w, bias, u, 3)
    assert torch.isnan(u.float()).all()  # nothing was launched


# ------------------------------------------------------------------ selective scan
R = 8  # dt_rank columns in front of B and C in the x_proj output


def scan_cases(c):
    return [((1, 1, 8, 16), "plain"), ((2, c - 1, 40, 16), "plain"), ((1, c, 8, 16), "plain"),
            ((3, c + 1, 64, 16), "threshold"), ((2, 2 * c + 3, 192, 16), "plain"),
            ((2, 2 * c + 3, 192, 16), "carry"), ((1, 5 * c, 72, 8), "plain")]


_scan = {}


def scan_ops(shape, kind):
    """bf16 / fp32 operands as the kernels read them.  δ spans [1e-3, 1.5] (log-uniform over the
    channels, so states both persist and die within a few tokens), a spans [-16, -0.5]."""
    B, L, I, N = shape
    g = torch.Generator().manual_seed(31 * B + 1009 * L + 17 * I + N + len(kind))
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    T = B * L
    delta = torch.exp(torch.empty(I).uniform_(math.log(1e-3), math.log(1.5), generator=g).double())
    o = dict(xz=torch.cat([rnd(T, I), 1.5 * rnd(T, I)], 1).to(BF16),  # [u | z]
             proj=rnd(T, R + 2 * N).to(BF16),                           # [dt low-rank | B | C]
             dt=(0.3 * rnd(T, I)).to(BF16),
             dt_bias=torch.log(torch.expm1(delta)).float(),
             A_log=torch.empty(I, N).uniform_(math.log(0.5), math.log(16.0), generator=g),
             D=1 + 0.5 * rnd(I), dy=rnd(T, I).to(BF16), du_in=rnd(T, I).to(BF16))
    if kind == "threshold":  # dt_raw + bias > 20: softplus is the identity there
        o["dt"].view(B, L, I)[:, ::5, ::3] = 24.0
    if kind == "carry":  # a near 0, one non-zero u at t = 0: the last chunk's output is pure carry
        o["A_log"] = torch.empty(I, N).uniform_(math.log(1e-3), math.log(1e-2), generator=g)
        uu = o["xz"][:, :I].view(B, L, I).clone()
        uu[:, 1:] = 0
        o["xz"][:, :I] = uu.view(T, I)
    return o


def scan_ref(o, shape, absmode=False):
    """fp64 forward and backward of the scan; absmode: the same expressions over absolute values."""
    B, L, I, N = shape
    ab = (lambda t: t.abs()) if absmode else (lambda t: t)
    v3 = lambda t, n: t.double().view(B, L, n)  # noqa: E731
    u, z = ab(v3(o["xz"][:, :I], I)), v3(o["xz"][:, I:], I)
    Bm, Cm = ab(v3(o["proj"][:, R:R + N], N)), ab(v3(o["proj"][:, R + N:], N))
    x = v3(o["dt"], I) + o["dt_bias"].double()
    delta = torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20))))
    sg = torch.where(x > 20, torch.ones_like(x), torch.sigmoid(x))
    a = -torch.exp(o["A_log"].double())
    aa = ab(a)
    D, dy, du_in = ab(o["D"].double()), ab(v3(o["dy"], I)), ab(v3(o["du_in"], I))
    sz = torch.sigmoid(z)
    gate = ab(z * sz)
    gp = sz * (1 + ab(z) * (1 - sz))
    dlu = delta * u
    h = torch.zeros(B, I, N, dtype=F64)
    hs = []
    for t in range(L):
        h = torch.exp(delta[:, t, :, None] * a) * h + dlu[:, t, :, None] * Bm[:, t, None, :]
        hs.append(h)
    p = torch.stack([(Cm[:, t, None, :] * hs[t]).sum(-1) for t in range(L)], 1) + D * u
    dp = dy * gate
    out = dict(y=p * gate, dz=dy * p * gp, dD=(dp * u).sum((0, 1)))
    lam = torch.zeros(B, I, N, dtype=F64)
    dA = torch.zeros(I, N, dtype=F64)
    dB, dC, dd, du = [None] * L, [None] * L, [None] * L, [None] * L
    for t in reversed(range(L)):
        al = torch.exp(delta[:, t, :, None] * a)
        mu = dp[:, t, :, None] * Cm[:, t, None, :] + lam
        hp = hs[t - 1] if t else torch.zeros_like(h)
        dC[t] = (dp[:, t, :, None] * hs[t]).sum(1)
        dB[t] = (mu * dlu[:, t, :, None]).sum(1)
        q = (mu * Bm[:, t, None, :]).sum(-1)
        wv = mu * al * hp
        dA += (wv * delta[:, t, :, None]).sum(0)
        dd[t] = (wv * aa).sum(-1) + q * u[:, t]
        du[t] = q * delta[:, t] + dp[:, t] * D + du_in[:, t]
        lam = mu * al
    ddt = torch.stack(dd, 1) * sg
    out.update(dB=torch.stack(dB, 1), dC=torch.stack(dC, 1), du=torch.stack(du, 1), ddt=ddt,
               dA_log=dA * aa, dbias=ddt.sum((0, 1)))
    out = {k: (v.reshape(B * L, -1) if v.dim() == 3 else v) for k, v in out.items()}
    out["n"] = (6 + 2 * (delta[..., None] * a).abs().max().item()) * L + 16
    return out


def scan_case(shape, kind):
    key = (shape, kind)
    if key not in _scan:
        o = scan_ops(shape, kind)
        _scan[key] = (o, scan_ref(o, shape), scan_ref(o, shape, absmode=True))
    return _scan[key]


def run_scan_fwd(K, o, shape, rows=None):
    B, L, I, N = shape
    sl = slice(None) if rows is None else rows
    xz, proj, dt = o["xz"].cuda()[sl], o["proj"].cuda()[sl], o["dt"].cuda()[sl]
    T = xz.shape[0]
    y = nan16(T, I)
    states = K.scan_states(T // L, L, I, N, "cuda")
    K.selective_scan_fwd(xz[:, :I], dt, o["dt_bias"].cuda(), o["A_log"].cuda(), proj[:, R:R + N],
                         proj[:, R + N:], o["D"].cuda(), xz[:, I:], y, L, states=states)
    return y, states


def run_scan_bwd(K, o, shape, states, rows=None, start=None):
    B, L, I, N = shape
    sl = slice(None) if rows is None else rows
    xz, proj, dt = o["xz"].cuda()[sl], o["proj"].cuda()[sl], o["dt"].cuda()[sl]
    dy, du_in = o["dy"].cuda()[sl], o["du_in"].cuda()[sl]
    T = xz.shape[0]
    dxz, dproj, ddt = nan16(T, 2 * I), nan16(T, R + 2 * N), nan16(T, I)
    if start is None:
        acc = [torch.zeros(I, N, device="cuda"), torch.zeros(I, device="cuda"),
               torch.zeros(I, device="cuda")]
    else:
        acc = [s.clone() for s in start]
    K.selective_scan_bwd(xz[:, :I], dt, o["dt_bias"].cuda(), o["A_log"].cuda(), proj[:, R:R + N],
                         proj[:, R + N:], o["D"].cuda(), xz[:, I:], dy, dxz[:, :I], dxz[:, I:],
                         ddt, dproj[:, R:R + N], dproj[:, R + N:], acc[0], acc[1], acc[2], L,
                         states=states, du_in=du_in)
    assert torch.isnan(dproj[:, :R].float()).all()  # the dt columns belong to another kernel
    return dict(du=dxz[:, :I], dz=dxz[:, I:], ddt=ddt, dB=dproj[:, R:R + N], dC=dproj[:, R + N:],
                dA_log=acc[0], dD=acc[1], dbias=acc[2])


@pytest.fixture(scope="module")
def cases(K):
    return scan_cases(K.scan_chunk())


@pytest.mark.parametrize("idx", range(7))
def test_selective_scan_fwd(K, cases, idx):
    shape, kind = cases[idx]
    B, L, I, N = shape
    c = K.scan_chunk()
    o, ref, ra = scan_case(shape, kind)
    y, states = run_scan_fwd(K, o, shape)
    wr = worst(y, ref["y"], ra["y"], ref["n"])
    print(f"selective_scan_fwd {shape} {kind}: n {ref['n']:.0f}, worst err / bound {wr:.3f}")
    assert wr <= 1.0
    if kind == "carry":  # the last chunk sees u only through the carried state, and it is not zero
        assert (ref["y"].view(B, L, I)[:, -1].abs() > 0).any() and (y.view(B, L, I)[:, -1] != 0).any()
    y2, states2 = run_scan_fwd(K, o, shape)
    assert same(y2, y)
    if L > c:
        assert same(states2[:, 1:], states[:, 1:])
    for b in range(B):
        yb, _ = run_scan_fwd(K, o, shape, rows=slice(b * L, (b + 1) * L))
        assert same(yb, y[b * L:(b + 1) * L]), b
    for Lp in range(c, L, c):  # the prefix property, sequence 0
        yp, _ = run_scan_fwd(K, o, (1, Lp, I, N), rows=slice(0, Lp))
        assert same(yp, y[:Lp]), Lp


@pytest.mark.parametrize("idx", range(7))
def test_selective_scan_bwd(K, cases, idx):
    shape, kind = cases[idx]
    B, L, I, N = shape
    o, ref, ra = scan_case(shape, kind)
    _, states = run_scan_fwd(K, o, shape)
    got = run_scan_bwd(K, o, shape, states)
    nb = lambda s: 2 * ref["n"] + s + 16  # noqa: E731
    terms = dict(du=N, dz=N, ddt=N, dB=I, dC=I, dA_log=B * L, dD=B * L, dbias=B * L)
    ratios = {}
    for k, s in terms.items():
        r = 0.0 if k in ("dA_log", "dD", "dbias") else 2.0 ** -8
        ratios[k] = worst(got[k], ref[k], ra[k], nb(s), r=r)
    print(f"selective_scan_bwd {shape} {kind}: worst err / bound "
          + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    g = torch.Generator().manual_seed(9)
    start = [torch.randn(I, N, generator=g).cuda(), torch.randn(I, generator=g).cuda(),
             torch.randn(I, generator=g).cuda()]
    again = run_scan_bwd(K, o, shape, states, start=start)
    for k in ("du", "dz", "ddt", "dB", "dC"):
        assert same(again[k], got[k]), k  # a second run gives the same bits
    for k, s in zip(("dA_log", "dD", "dbias"), start):
        assert same(again[k], s + got[k]), k  # += of the fp32 sums
    for b in range(B):
        rows = slice(b * L, (b + 1) * L)
        _, sb = run_scan_fwd(K, o, shape, rows=rows)
        one = run_scan_bwd(K, o, shape, sb, rows=rows)
        for k in ("du", "dz", "ddt", "dB", "dC"):
            assert same(one[k], got[k][rows]), (k, b)


def test_selective_scan_eval_forward_needs_no_states(K, cases):
    shape, kind = cases[4]
    B, L, I, N = shape
    o, _, _ = scan_case(shape, kind)
    y, _ = run_scan_fwd(K, o, shape)
    xz, proj = o["xz"].cuda(), o["proj"].cuda()
    y2 = nan16(B * L, I)
    K.selective_scan_fwd(xz[:, :I], o["dt"].cuda(), o["dt_bias"].cuda(), o["A_log"].cuda(),
                         proj[:, R:R + N], proj[:, R + N:], o["D"].cuda(), xz[:, I:], y2, L)
    assert same(y2, y)


def test_selective_scan_argument_errors(K):
    L, I, N = 4, 16, 16
    T = 2 * L
    z16 = lambda *s: torch.zeros(*s, dtype=BF16, device="cuda")  # noqa: E731
    u, dt, z, y = z16(T, I), z16(T, I), z16(T, I), nan16(T, I)
    proj = z16(T, R + 2 * N)
    Bm, Cm = proj[:, R:R + N], proj[:, R + N:]
    bias, A, D = torch.zeros(I, device="cuda"), torch.zeros(I, N, device="cuda"), torch.zeros(I, device="cuda")
    ok = lambda **kw: K.selective_scan_fwd(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("u", u), ("dt", dt), ("bias", bias), ("A", A), ("Bm", Bm), ("Cm", Cm), ("D", D), ("z", z),
        ("y", y))], kw.get("L", L))
    shifted = z16(T, R + 8 + 2 * N)
    with pytest.raises(RuntimeError, match=ERR_ARG):  # B and C 8 bytes off a 16-byte boundary
        ok(Bm=shifted[:, R + 4:R + 4 + N], Cm=shifted[:, R + 4 + N:R + 4 + 2 * N])
    odd = z16(T, R + 2 * N + 4)
    with pytest.raises(RuntimeError, match=ERR_ARG):  # a leading dimension that is no multiple of 8
        ok(Bm=odd[:, R:R + N], Cm=odd[:, R + N:R + 2 * N])
    with pytest.raises(RuntimeError, match=ERR_ARG):  # I % 8
        K.selective_scan_fwd(z16(T, 12), z16(T, 12), torch.zeros(12, device="cuda"),
                             torch.zeros(12, N, device="cuda"), Bm, Cm, torch.zeros(12, device="cuda"),
                             z16(T, 12), nan16(T, 12), L)
    p4 = z16(T, 8)
    with pytest.raises(RuntimeError, match=ERR_ARG):  # N is 8 or 16
        K.selective_scan_fwd(u, dt, bias, torch.zeros(I, 4, device="cuda"), p4[:, :4], p4[:, 4:], D,
                             z, y, L)
    with pytest.raises(RuntimeError, match="GPU"):
        ok(u=u.cpu())
    with pytest.raises(RuntimeError, match="GPU"):
        ok(A=A.cpu())
    with pytest.raises(ValueError):
        ok(L=3)
    acc = [torch.zeros(I, N, device="cuda"), torch.zeros(I, device="cuda"), torch.zeros(I, device="cuda")]
    c = K.scan_chunk()
    Tl = c + 1
    with pytest.raises(ValueError, match="states"):  # two chunks and no states from the forward
        K.selective_scan_bwd(z16(Tl, I), z16(Tl, I), bias, A, z16(Tl, N), z16(Tl, N), D, z16(Tl, I),
                             z16(Tl, I), nan16(Tl, I), nan16(Tl, I), nan16(Tl, I), nan16(Tl, N),
                             nan16(Tl, N), *acc, Tl)
    with pytest.raises(RuntimeError, match="GPU"):
        K.selective_scan_bwd(u, dt, bias, A, Bm, Cm, D, z, u, nan16(T, I), nan16(T, I), nan16(T, I),
                             nan16(T, N), nan16(T, N), acc[0].cpu(), acc[1], acc[2], L)
    assert torch.isnan(y.float()).all()  # nothing was launched


# ------------------------------------------------------------------ engine
import mamba_oracle as MO  # noqa: E402

EB, EL = 3, 70  # sequences and length of the parity batches (σ is measured at this shape)


def fbits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def ref():
    """The oracle side, computed once: seed-0 weights (mamba_oracle.init_params), one 3 x 70
    batch, the bf16 "fused"-policy loss and gradients, the fp32 loss and σ at this shape."""
    from multimodal_llm_pretraining_amd import config as C

    cfg = C.get_config("tiny-mamba")
    P = MO.init_params(cfg, seed=0)
    batch = MO.make_batch(cfg, EB, EL, seed=1)
    loss16, G = MO.loss_and_grads(P, cfg, batch, "bf16", "fused")
    with torch.no_grad():
        loss32 = MO.forward_loss(P, cfg, batch, "fp32").item()
    sigma = MO.bf16_sigma(P, cfg, EB, EL)
    print(f"tiny-mamba {EB}x{EL}: bf16 {loss16:.7f} fp32 {loss32:.7f} sigma {sigma:.3e}")
    return dict(cfg=cfg, P=P, batch=batch, loss16=loss16, loss32=loss32, G=G, sigma=sigma)


def engine_for(cfg, P, checkpointing=False):
    from multimodal_llm_pretraining_amd import config as C
    from multimodal_llm_pretraining_amd.engine import Engine
    from multimodal_llm_pretraining_amd.params import ParamStore

    store = ParamStore(C.param_shapes(cfg), "cuda")
    store.load(P)
    store.refresh_shadow()
    eng = Engine(cfg, store)
    eng.checkpointing = checkpointing
    return store, eng


def run(cfg, P, batch, steps=1, **kw):
    """([loss per micro-step], the store with the flat grads of the last one)."""
    from multimodal_llm_pretraining_amd.engine import Batch

    store, eng = engine_for(cfg, P, **kw)
    b = Batch(cfg, batch["input_ids"], batch["labels"], None, store.device)
    losses = []
    for _ in range(steps):
        store.zero_grad()
        s = eng.forward(b, 1.0 / b.num_items)
        eng.backward(b)
        losses.append(s.item() / b.num_items)
    assert eng.cache == {}
    return losses, store


def test_loss_and_grads(ref):
    """Every parameter, the tied embedding (gather + decoder) and A_log included."""
    (loss,), store = run(ref["cfg"], ref["P"], ref["batch"])
    sigma = ref["sigma"]
    print(f"GPU loss {loss:.7f} (bf16 oracle {ref['loss16']:.7f}, fp32 {ref['loss32']:.7f}), "
          f"sigma {sigma:.3e}")
    errs = {k: ((store.g(k).cpu() - r).norm() / (r.norm() + 1e-20)).item()
            for k, r in ref["G"].items()}
    print(f"worst gradient error {max((v, k) for k, v in errs.items())}")
    assert abs(loss - ref["loss16"]) < 1e-4 + 3 * sigma, (loss, ref["loss16"], ref["loss32"], sigma)
    for k, e in errs.items():
        assert e < 3e-2, (k, e)
    assert {"text.embed", "text.layers.0.A_log", "text.layers.1.D", "text.layers.0.dt_proj.bias",
            "text.layers.1.conv.weight"} <= set(errs)
    assert all(float(r.norm()) > 0 for r in ref["G"].values())
    t = ref["cfg"].text
    assert int(store.g("text.embed")[t.n_vocab:].count_nonzero()) == 0


def test_two_adamw_steps(ref):
    """The reference recipe's optimizer (AdamW β (0.9, 0.95), weight decay 0.1, clip 1.0,
    cosine_with_min_lr with an absolute min_lr) through trainer.ManualTrainer against
    torch.optim.AdamW."""
    from multimodal_llm_pretraining_amd.optim import AdamConfig, min_lr_rate_of
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    cfg, P, sigma = ref["cfg"], ref["P"], ref["sigma"]
    batches = [ref["batch"], MO.make_batch(cfg, EB, EL, seed=2)]
    lrs = MO.cosine_min_lr(1e-3, 1e-5, 0, 4, 2)
    want, _ = MO.train_steps(P, cfg, batches, lrs, "bf16")
    tr = ManualTrainer(StepConfig(model="tiny-mamba", scheduler="cosine_with_min_lr",
                                  num_warmup_steps=0, num_training_steps=4,
                                  min_lr_rate=min_lr_rate_of({"min_lr": 1e-5}, 1e-3)),
                       AdamConfig(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.1, adamw=True,
                                  max_grad_norm=1.0), "cuda")
    tr.store.load(P)
    tr.store.refresh_shadow()
    got = []
    for bd in batches:
        b = tr.stage(bd)
        assert b.num_items == EB * (EL - 1)
        got.append(tr.train_step([b], b.num_items).item() / b.num_items)
    print(f"two AdamW steps: GPU {got}, bf16 oracle {want}, sigma {sigma:.3e}")
    assert abs(got[0] - want[0]) < 1e-4 + 3 * sigma, (got, want, sigma)
    assert abs(got[1] - want[1]) < 3e-4 + 3 * sigma, (got, want, sigma)
    assert got[1] != got[0]
    assert int(tr.store.p("text.embed")[cfg.text.n_vocab:].count_nonzero()) == 0


def test_grad_accumulation_equals_big_batch(ref):
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg, bd = ref["cfg"], ref["batch"]
    _, full = run(cfg, ref["P"], bd)
    store, eng = engine_for(cfg, ref["P"])
    n = EB * (EL - 1)
    total = 0.0
    for sl in (slice(0, 1), slice(1, 3)):
        b = Batch(cfg, bd["input_ids"][sl], bd["labels"][sl], None, store.device)
        total += eng.forward(b, 1.0 / n).item()
        eng.backward(b)
    err = ((store.grad - full.grad).norm() / full.grad.norm()).item()
    assert err < 1e-2, err
    assert abs(total / n - ref["loss16"]) < 1e-4 + 3 * ref["sigma"]


def test_block_checkpointing_is_bitwise(ref):
    cfg, P, bd = ref["cfg"], ref["P"], ref["batch"]
    la, a = run(cfg, P, bd, steps=2)
    lb, b = run(cfg, P, bd, steps=2, checkpointing=True)
    assert la == lb and torch.equal(fbits(a.grad), fbits(b.grad))
    assert la[0] == la[1]  # no dropout: the same micro-batch gives the same loss


def test_reset_and_eval_forward(ref):
    """need_grad = False keeps nothing: no cache, no scan states (K.scan_states is not called)."""
    from multimodal_llm_pretraining_amd import kernels as K
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg, bd = ref["cfg"], ref["batch"]
    n = EB * (EL - 1)
    (loss,), full = run(cfg, ref["P"], bd)
    store, eng = engine_for(cfg, ref["P"])
    b = Batch(cfg, bd["input_ids"], bd["labels"], None, store.device)
    eng.forward(b, 1.0 / n)
    assert eng.cache
    eng.reset()
    assert eng.cache == {}
    calls, orig = [], K.scan_states
    K.scan_states = lambda *a, **k: calls.append(a) or orig(*a, **k)
    try:
        ev = eng.forward(b, 1.0 / n, need_grad=False).item() / n
        assert calls == []
        eng.forward(b, 1.0 / n)
        assert len(calls) == cfg.text.layers
    finally:
        K.scan_states = orig
    assert ev == pytest.approx(loss, abs=1e-6)
    eng.backward(b)
    assert eng.cache == {} and torch.equal(fbits(store.grad), fbits(full.grad))


def test_padded_batch_is_refused(ref):
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg, bd = ref["cfg"], ref["batch"]
    mask = torch.ones(EB, EL, dtype=torch.int64)
    Batch(cfg, bd["input_ids"], bd["labels"], None, torch.device("cuda"), attention_mask=mask)
    mask[1, -5:] = 0
    with pytest.raises(ValueError, match="padded"):
        Batch(cfg, bd["input_ids"], bd["labels"], None, torch.device("cuda"), attention_mask=mask)


def test_dropin_module(ref):
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining

    cfg, P, bd = ref["cfg"], ref["P"], ref["batch"]
    (loss,), eng_store = run(cfg, P, bd)
    m = MMPTForPretraining(cfg)
    assert (m.config.hidden_size, m.config.vocab_size, m.config.state_size) == (128, 515, 16)
    assert (m.config.intermediate_size, m.config.time_step_rank) == (256, 8)
    A0 = m.store.p("text.layers.0.A_log")  # HF's initialisation: log(1..N) in every row, D = 1
    assert torch.allclose(A0[5].cpu(), torch.log(torch.arange(1, 17.0)))
    assert float(m.store.p("text.layers.1.D").min()) == 1.0
    m.store.load(P)
    m.store.refresh_shadow()
    out = m(input_ids=bd["input_ids"], labels=bd["labels"])
    assert out.loss.item() == pytest.approx(loss, abs=1e-6)
    out.loss.backward()
    assert m.engine.cache == {}
    for name, p in m.named_parameters():
        assert p.grad is not None and p.grad.data_ptr() == m.store.g(name).data_ptr(), name
        assert torch.equal(fbits(p.grad), fbits(eng_store.g(name))), name
    n = EB * (EL - 1)
    half = m(input_ids=bd["input_ids"], labels=bd["labels"], num_items_in_batch=2 * n)
    assert half.loss.item() == pytest.approx(loss / 2, rel=1e-6)
    m.engine.reset()
    with torch.no_grad():
        ev = m(input_ids=bd["input_ids"], labels=bd["labels"])
    assert m.engine.cache == {} and ev.loss.item() == pytest.approx(loss, abs=1e-6)
    m.gradient_checkpointing_enable()
    assert m.engine.checkpointing
    mask = torch.ones(EB, EL, dtype=torch.int64)
    mask[0, -1] = 0
    with pytest.raises(ValueError, match="padded"):
        m(input_ids=bd["input_ids"], labels=bd["labels"], attention_mask=mask)


def test_grad_ready_hook_covers_every_parameter_once(ref):
    from multimodal_llm_pretraining_amd.engine import Batch

    cfg, bd = ref["cfg"], ref["batch"]
    store, eng = engine_for(cfg, ref["P"])
    seen = []
    eng.grad_ready_hook = lambda lo, hi: seen.append((lo, hi))
    b = Batch(cfg, bd["input_ids"], bd["labels"], None, store.device)
    eng.forward(b, 1.0 / b.num_items)
    eng.backward(b)
    torch.cuda.synchronize()
    assert seen
    seen.sort()
    for (_, hi), (lo, _) in zip(seen, seen[1:]):
        assert hi <= lo, seen  # no element announced twice
    for name, off in store.offsets.items():
        n = store.g(name).numel()
        assert any(lo <= off and off + n <= hi for lo, hi in seen), name


def test_offloaded_optimizer_matches_device_adam(ref):
    """Optimizer offload gates each unit's first forward on its host update (each MambaBlock is
    a unit): first-step losses equal, later ones within the project's 1e-4."""
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    cfg, P = ref["cfg"], ref["P"]
    batches = [ref["batch"], MO.make_batch(cfg, EB, EL, seed=2), MO.make_batch(cfg, EB, EL, seed=3)]
    got = {}
    for offload in (False, True):
        tr = ManualTrainer(StepConfig(model="tiny-mamba", scheduler="constant", offload=offload),
                           AdamConfig(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.1, adamw=True,
                                      max_grad_norm=1.0), "cuda")
        tr.store.load(P)
        tr.store.refresh_shadow()
        got[offload] = []
        for bd in batches:
            b = tr.stage(bd)
            got[offload].append(tr.train_step([b], b.num_items).item() / b.num_items)
        tr.flush()
    print(f"offload {got[True]} device {got[False]}")
    assert got[True][0] == got[False][0], got
    for a, b in zip(got[True][1:], got[False][1:]):
        assert abs(a - b) < 1e-4, got


def test_harness_runs_the_text_batches(ref):
    """TrainingClass.build_trainer → benchmarking.ManualTrainer → estimate_step_time over the
    dummy text dataset (plain and zero_1 with optimizer offload), with the recipe's scheduler
    arguments (an absolute min_lr); ZeRO-2 is refused by name before the module's storage is
    touched."""
    from multimodal_llm_pretraining_amd.benchmarking import estimate_step_time
    from multimodal_llm_pretraining_amd.data import DummyTextModelingDataset
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining
    from multimodal_llm_pretraining_amd.train import TrainingClass

    cfg = ref["cfg"]
    ds = DummyTextModelingDataset(cfg.text.n_vocab, EL, 32)
    kw = dict(num_training_steps=4, micro_batch_size=4, gradient_accumulation_steps=1, bf16=True,
              optimizer=torch.optim.AdamW,
              optimizer_kwargs={"lr": 8e-4, "betas": (0.9, 0.95), "weight_decay": 0.1},
              scheduler_type="cosine_with_min_lr", max_grad_norm=1.0)
    for extra in ({}, {"zero_stage": "1", "zero_offload_optimizer": True}):
        m = MMPTForPretraining(cfg)
        m.store.load(ref["P"])
        m.store.refresh_shadow()
        tr = TrainingClass(**kw, scheduler_kwargs={"num_warmup_steps": 1, "min_lr": 1e-5},
                           **extra).build_trainer(m, ds)
        before = m.store.w("text.layers.1.x_proj.weight").clone()
        assert estimate_step_time(tr, 4, 8, 1) > 0
        torch.cuda.synchronize()
        assert not torch.equal(m.store.w("text.layers.1.x_proj.weight"), before)
    m = MMPTForPretraining(cfg)
    with pytest.raises(NotImplementedError, match="zero_2"):
        TrainingClass(**kw, scheduler_kwargs={"num_warmup_steps": 1, "min_lr": 1e-5},
                      zero_stage="2").build_trainer(m, ds)
    assert not m.partitioned and m.store.master.numel() == m.store.padded
