"""The K22 varlen entries (include/mmpt.h: mmpt_causal_conv1d_varlen_*, mmpt_selective_scan_varlen_*)
on packed rows: T tokens of several sequences laid end to end.

Per-token outputs are held BITWISE to the dense entries run on each sequence alone (B = 1, L = its
length): u and dx of the conv; y, the chunk-entry states, du, dz, ddt_raw, dB and dC of the scan.
The varlen kernels are the dense kernels' code with another index computation, so a difference is
a read or a carry across a sequence boundary, not a tolerance question.  With equal lengths (V4)
they also have the bits of the dense call over the whole batch.

The sums over tokens (dw, db; dA_log, dD, ddt_bias) add the same per-workgroup partials in another
fixed order, so they are held to the fp64 bars of tests/test_mamba_gpu.py (u = 2^-24, A the same
expression over absolute values), the fp64 reference computed per sequence and summed:
  dw, db:                 2^-8 |ref| + T u A, with that file's allowance for a first rounding (dc to
                          bf16) that lies within the kernel's evaluation error of a tie;
  dA_log, dD, ddt_bias:   n_b u A,  n_b = 2 n + T + 16,  n = (6 + 2 max|δ a|) L_max + 16 taken at
                          the longest sequence.
`+=` is checked bitwise against start + (the result from zero) and a repeat gives the same bits.

Length sets (c = scan_chunk()): V1 conv windows that span several boundaries and one-token
sequences; V2 chunk edges with a one-token sequence between multi-chunk ones; V3 a long carry
between short neighbours; V4 equal lengths.  Channels 8, 40 (a partial lane group of the scan) and
192 (more than one 128-channel scan workgroup); N 16 and 8.  Operands are drawn as
tests/test_mamba_gpu.py draws them (scan_ops / conv_case)."""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ERR_ARG = "status -1"
U = 2.0 ** -24
R = 8  # dt_rank columns in front of B and C in the x_proj output
PAD = 5  # poisoned rows past T in every output buffer
SETS = ["V1", "V2", "V3", "V4"]


@pytest.fixture(scope="module")
def K():
    from multimodal_llm_pretraining_amd import kernels

    return kernels


def lens_of(name, c):
    return {"V1": [1, 1, 2, 3, 4, 5], "V2": [c + 1, 1, c, c - 1, 2 * c + 1],
            "V3": [3, 4 * c + 2, 2], "V4": [c + 1] * 3}[name]


def same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def rb(t):
    return t.to(F32).to(BF16).double()


def worst(got, ref, a, n, r=2.0 ** -8, extra=None):
    err = (got.double().cpu() - ref).abs()
    bound = r * ref.abs() + n * U * a
    if extra is not None:
        bound = bound + extra
    return (err / bound.clamp_min(1e-300)).max().item()


def nan16(*shape):
    return torch.full(shape, float("nan"), dtype=BF16, device="cuda")


def offsets(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


def pos_of(lens):
    return torch.cat([torch.arange(n, dtype=torch.int32) for n in lens]).cuda()


# ------------------------------------------------------------------ causal conv
def conv_ops(T, C):
    g = torch.Generator().manual_seed(7919 + 104729 * T + C)
    return dict(xz=torch.randn(T, 2 * C, generator=g).to(BF16),  # x is the first half of [x | z]
                w=(torch.randn(4, C, generator=g) * 0.4).to(BF16),
                bias=(torch.randn(C, generator=g) * 0.3).to(BF16),
                du=torch.randn(T, C, generator=g).to(BF16),
                du2=torch.randn(T, C, generator=g).to(BF16))


def conv_sums_ref(o, rows, C):
    """fp64 dw / db of one sequence (rows of the packed operands), their A and the tie allowance:
    the expressions of conv_case in tests/test_mamba_gpu.py with B = 1."""
    L = rows.stop - rows.start
    x = o["xz"][rows, :C].double().view(1, L, C)
    w64, b64 = o["w"].double(), o["bias"].double()
    du64 = (o["du"][rows].double() + o["du2"][rows].double()).view(1, L, C)
    xp = F.pad(x, (0, 0, 3, 0))
    taps = [xp[:, k:k + L] for k in range(4)]
    c64 = sum(w64[k] * taps[k] for k in range(4)) + b64
    a_c = sum(w64[k].abs() * taps[k].abs() for k in range(4)) + b64.abs()
    cb, clo, chi = rb(c64), rb(c64 - 16 * U * a_c), rb(c64 + 16 * U * a_c)

    def dsilu(c, ab=False):
        s = torch.sigmoid(c)
        return s * (1 + (c.abs() if ab else c) * (1 - s))

    cands = []
    for c in (cb, clo, chi):
        v, e = du64 * dsilu(c), 16 * U * du64.abs() * dsilu(c, True)
        cands += [rb(v - e), rb(v + e)]
    dcb = rb(du64 * dsilu(cb))
    amb = torch.stack(cands).amax(0) - torch.stack(cands).amin(0)
    return dict(dw=torch.stack([(dcb * taps[k]).sum((0, 1)) for k in range(4)]),
                a_dw=torch.stack([(dcb.abs() * taps[k].abs()).sum((0, 1)) for k in range(4)]),
                amb_dw=torch.stack([(amb * taps[k].abs()).sum((0, 1)) for k in range(4)]),
                db=dcb.sum((0, 1)), a_db=dcb.abs().sum((0, 1)), amb_db=amb.sum((0, 1)))


def run_conv(K, o, C, lens, start=None):
    T = sum(lens)
    xz, w, bias = o["xz"].cuda(), o["w"].cuda(), o["bias"].cuda()
    du, du2, pos = o["du"].cuda(), o["du2"].cuda(), pos_of(lens)
    u, dxz = nan16(T + PAD, C), nan16(T + PAD, 2 * C)
    K.causal_conv1d_varlen_fwd(xz[:, :C], w, bias, u[:T], pos)
    if start is None:
        dw, db = torch.zeros(4, C, device="cuda"), torch.zeros(C, device="cuda")
    else:
        dw, db = start[0].clone(), start[1].clone()
    K.causal_conv1d_varlen_bwd(xz[:, :C], w, bias, du, dxz[:T, :C], dw, db, pos, du2=du2)
    assert torch.isnan(u[T:].float()).all() and torch.isnan(dxz[T:].float()).all()  # the poison
    assert torch.isnan(dxz[:, C:].float()).all()
    return u[:T], dxz[:T, :C], dw, db


@pytest.mark.parametrize("C", [8, 40, 192])
@pytest.mark.parametrize("name", SETS)
def test_causal_conv1d_varlen(K, name, C):
    lens = lens_of(name, K.scan_chunk())
    T, cu = sum(lens), offsets(lens)
    o = conv_ops(T, C)
    u, dx, dw, db = run_conv(K, o, C, lens)
    xz, w, bias = o["xz"].cuda(), o["w"].cuda(), o["bias"].cuda()
    du, du2 = o["du"].cuda(), o["du2"].cuda()
    zeros = lambda: (torch.zeros(4, C, device="cuda"), torch.zeros(C, device="cuda"))  # noqa: E731
    for s, n in enumerate(lens):  # each sequence alone through the dense entries: the same bits
        rows = slice(cu[s], cu[s + 1])
        one_u, one_dx = nan16(n, C), nan16(n, C)
        K.causal_conv1d_fwd(xz[rows, :C], w, bias, one_u, n)
        K.causal_conv1d_bwd(xz[rows, :C], w, bias, du[rows], one_dx, *zeros(), n, du2=du2[rows])
        assert same(one_u, u[rows]), (s, n)
        assert same(one_dx, dx[rows]), (s, n)
    if name == "V4":  # equal lengths: also the dense call over the batch
        all_u, all_dx = nan16(T, C), nan16(T, C)
        K.causal_conv1d_fwd(xz[:, :C], w, bias, all_u, lens[0])
        K.causal_conv1d_bwd(xz[:, :C], w, bias, du, all_dx, *zeros(), lens[0], du2=du2)
        assert same(all_u, u) and same(all_dx, dx)
    refs = [conv_sums_ref(o, slice(cu[s], cu[s + 1]), C) for s in range(len(lens))]
    ref = {k: sum(r[k] for r in refs) for k in refs[0]}
    ww = worst(dw, ref["dw"], ref["a_dw"], T, extra=ref["amb_dw"])
    wb = worst(db, ref["db"], ref["a_db"], T, extra=ref["amb_db"])
    print(f"causal_conv1d_varlen {name} C {C}: worst err / bound dw {ww:.3f} db {wb:.3f}")
    assert ww <= 1.0 and wb <= 1.0
    assert same(dw, dw.to(BF16).float()) and same(db, db.to(BF16).float())
    g = torch.Generator().manual_seed(6)
    start = [torch.randn(4, C, generator=g).cuda(), torch.randn(C, generator=g).cuda()]
    u1, dx1, dw1, db1 = run_conv(K, o, C, lens, start=start)
    assert same(dw1, start[0] + dw) and same(db1, start[1] + db)  # += of the bf16-rounded sums
    assert same(u1, u) and same(dx1, dx)  # a repeat gives the same bits


# ------------------------------------------------------------------ selective scan
def scan_ops(T, I, N):
    """scan_ops of tests/test_mamba_gpu.py, kind "plain", over T packed rows."""
    g = torch.Generator().manual_seed(31 + 1009 * T + 17 * I + N)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    delta = torch.exp(torch.empty(I).uniform_(math.log(1e-3), math.log(1.5), generator=g).double())
    return dict(xz=torch.cat([rnd(T, I), 1.5 * rnd(T, I)], 1).to(BF16),  # [u | z]
                proj=rnd(T, R + 2 * N).to(BF16),                           # [dt low-rank | B | C]
                dt=(0.3 * rnd(T, I)).to(BF16),
                dt_bias=torch.log(torch.expm1(delta)).float(),
                A_log=torch.empty(I, N).uniform_(math.log(0.5), math.log(16.0), generator=g),
                D=1 + 0.5 * rnd(I), dy=rnd(T, I).to(BF16), du_in=rnd(T, I).to(BF16))


def scan_sums_ref(o, rows, I, N, absmode=False):
    """fp64 dA_log, dD, ddt_bias of one sequence and n: scan_ref of tests/test_mamba_gpu.py, B = 1."""
    L = rows.stop - rows.start
    ab = (lambda t: t.abs()) if absmode else (lambda t: t)
    u, z = ab(o["xz"][rows, :I].double()), o["xz"][rows, I:].double()
    Bm, Cm = ab(o["proj"][rows, R:R + N].double()), ab(o["proj"][rows, R + N:].double())
    x = o["dt"][rows].double() + o["dt_bias"].double()
    delta = torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20))))
    sg = torch.where(x > 20, torch.ones_like(x), torch.sigmoid(x))
    a = -torch.exp(o["A_log"].double())
    aa = ab(a)
    D, dy = ab(o["D"].double()), ab(o["dy"][rows].double())
    sz = torch.sigmoid(z)
    gate = ab(z * sz)
    dlu = delta * u
    h = torch.zeros(I, N, dtype=F64)
    hs = []
    for t in range(L):
        h = torch.exp(delta[t, :, None] * a) * h + dlu[t, :, None] * Bm[t, None, :]
        hs.append(h)
    dp = dy * gate
    lam = torch.zeros(I, N, dtype=F64)
    dA = torch.zeros(I, N, dtype=F64)
    dbias = torch.zeros(I, dtype=F64)
    for t in reversed(range(L)):
        al = torch.exp(delta[t, :, None] * a)
        mu = dp[t, :, None] * Cm[t, None, :] + lam
        hp = hs[t - 1] if t else torch.zeros_like(h)
        q = (mu * Bm[t, None, :]).sum(-1)
        wv = mu * al * hp
        dA += wv * delta[t, :, None]
        dbias += ((wv * aa).sum(-1) + q * u[t]) * sg[t]
        lam = mu * al
    n = (6 + 2 * (delta[..., None] * a).abs().max().item()) * L + 16
    return dict(dA_log=dA * aa, dD=(dp * u).sum(0), dbias=dbias), n


def scan_args(o, I, N, rows=slice(None)):
    xz, proj = o["xz"].cuda()[rows], o["proj"].cuda()[rows]
    return (xz[:, :I], o["dt"].cuda()[rows], o["dt_bias"].cuda(), o["A_log"].cuda(),
            proj[:, R:R + N], proj[:, R + N:], o["D"].cuda(), xz[:, I:])


def fresh_acc(I, N, start=None):
    if start is not None:
        return [s.clone() for s in start]
    return [torch.zeros(I, N, device="cuda"), torch.zeros(I, device="cuda"),
            torch.zeros(I, device="cuda")]


def bwd_buffers(T, I, N):
    dxz, dproj, ddt = nan16(T + PAD, 2 * I), nan16(T + PAD, R + 2 * N), nan16(T + PAD, I)
    outs = dict(du=dxz[:T, :I], dz=dxz[:T, I:], ddt=ddt[:T], dB=dproj[:T, R:R + N],
                dC=dproj[:T, R + N:])
    return (dxz, dproj, ddt), outs


def run_scan_varlen(K, o, I, N, tables, start=None):
    T = tables.T
    y = nan16(T + PAD, I)
    states = K.scan_varlen_states(tables, I, N, "cuda")
    K.selective_scan_varlen_fwd(*scan_args(o, I, N), y[:T], tables, states=states)
    raw, outs = bwd_buffers(T, I, N)
    acc = fresh_acc(I, N, start)
    K.selective_scan_varlen_bwd(*scan_args(o, I, N), o["dy"].cuda(), outs["du"], outs["dz"],
                                outs["ddt"], outs["dB"], outs["dC"], *acc, tables, states=states,
                                du_in=o["du_in"].cuda())
    assert torch.isnan(y[T:].float()).all()  # the poison past T, and the dt columns of dproj
    assert all(torch.isnan(b[T:].float()).all() for b in raw)
    assert torch.isnan(raw[1][:, :R].float()).all()
    outs.update(y=y[:T], states=states, dA_log=acc[0], dD=acc[1], dbias=acc[2])
    return outs


def run_scan_dense(K, o, I, N, rows, L):
    T = rows.stop - rows.start
    y = nan16(T, I)
    states = K.scan_states(T // L, L, I, N, "cuda")
    K.selective_scan_fwd(*scan_args(o, I, N, rows), y, L, states=states)
    _, outs = bwd_buffers(T, I, N)
    K.selective_scan_bwd(*scan_args(o, I, N, rows), o["dy"].cuda()[rows], outs["du"], outs["dz"],
                         outs["ddt"], outs["dB"], outs["dC"], *fresh_acc(I, N), L, states=states,
                         du_in=o["du_in"].cuda()[rows])
    outs.update(y=y, states=states)
    return outs


PER_TOKEN = ("y", "du", "dz", "ddt", "dB", "dC")


@pytest.mark.parametrize("N", [16, 8])
@pytest.mark.parametrize("I", [8, 40, 192])
@pytest.mark.parametrize("name", SETS)
def test_selective_scan_varlen(K, name, I, N):
    c = K.scan_chunk()
    lens = lens_of(name, c)
    T, cu = sum(lens), offsets(lens)
    o = scan_ops(T, I, N)
    tables = K.scan_tables(lens, "cuda")
    cc = offsets([(n + c - 1) // c for n in lens])
    assert tables.total_chunks == cc[-1] and tables.cu_chunks.tolist() == cc
    assert tables.cu_seqlens.tolist() == cu
    got = run_scan_varlen(K, o, I, N, tables)
    for s, n in enumerate(lens):  # each sequence alone through the dense entries: the same bits
        rows = slice(cu[s], cu[s + 1])
        one = run_scan_dense(K, o, I, N, rows, n)
        for k in PER_TOKEN:
            assert same(one[k], got[k][rows]), (k, s, n)
        if n > c:  # (a single chunk has no entry state to keep)
            assert same(one["states"][0], got["states"][cc[s]:cc[s + 1]]), (s, n)
    if name == "V4":  # equal lengths: also the dense call over the batch
        whole = run_scan_dense(K, o, I, N, slice(0, T), lens[0])
        for k in PER_TOKEN:
            assert same(whole[k], got[k]), k
        assert same(whole["states"].view(-1, I, N), got["states"])
    refs = [scan_sums_ref(o, slice(cu[s], cu[s + 1]), I, N) for s in range(len(lens))]
    abss = [scan_sums_ref(o, slice(cu[s], cu[s + 1]), I, N, absmode=True) for s in range(len(lens))]
    n_b = 2 * max(n for _, n in refs) + T + 16  # n at the longest sequence
    ratios = {}
    for k in ("dA_log", "dD", "dbias"):
        ratios[k] = worst(got[k], sum(r[k] for r, _ in refs), sum(r[k] for r, _ in abss), n_b, r=0.0)
    print(f"selective_scan_varlen {name} I {I} N {N}: n_b {n_b:.0f}, worst err / bound "
          + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    g = torch.Generator().manual_seed(9)
    start = [torch.randn(I, N, generator=g).cuda(), torch.randn(I, generator=g).cuda(),
             torch.randn(I, generator=g).cuda()]
    again = run_scan_varlen(K, o, I, N, tables, start=start)
    for k in PER_TOKEN:
        assert same(again[k], got[k]), k  # a repeat gives the same bits
    for s, n in enumerate(lens):
        if n > c:
            assert same(again["states"][cc[s]:cc[s + 1]], got["states"][cc[s]:cc[s + 1]]), s
    for k, s in zip(("dA_log", "dD", "dbias"), start):
        assert same(again[k], s + got[k]), k  # += of the fp32 sums


def test_eval_forward_needs_no_states(K):
    c = K.scan_chunk()
    lens, I, N = lens_of("V2", c), 40, 16
    o, tables = scan_ops(sum(lens), I, N), K.scan_tables(lens_of("V2", c), "cuda")
    y, y2 = nan16(tables.T, I), nan16(tables.T, I)
    K.selective_scan_varlen_fwd(*scan_args(o, I, N), y, tables,
                                states=K.scan_varlen_states(tables, I, N, "cuda"))
    K.selective_scan_varlen_fwd(*scan_args(o, I, N), y2, tables)
    assert same(y, y2)


# ------------------------------------------------------------------ argument errors
def test_argument_errors(K):
    from multimodal_llm_pretraining_amd import _lib

    C = I = N = 16
    lens = [3, 5]
    T = sum(lens)
    z16 = lambda *s: torch.zeros(*s, dtype=BF16, device="cuda")  # noqa: E731
    x, u, w, bias = z16(T, C), nan16(T, C), z16(4, C), z16(C)
    pos = pos_of(lens)
    stream = torch.cuda.current_stream().cuda_stream
    conv = lambda p, rows=T: _lib.call(  # noqa: E731
        "mmpt_causal_conv1d_varlen_fwd", rows, C, 4, p, x.data_ptr(), C, w.data_ptr(),
        bias.data_ptr(), u.data_ptr(), C, stream)
    with pytest.raises(RuntimeError, match=ERR_ARG):  # a table pointer 2 bytes off
        conv(pos.data_ptr() + 2)
    with pytest.raises(RuntimeError, match=ERR_ARG):
        conv(None)
    with pytest.raises(RuntimeError, match=ERR_ARG):  # no rows
        conv(pos.data_ptr(), 0)
    with pytest.raises(RuntimeError, match="GPU"):
        K.causal_conv1d_varlen_fwd(x, w, bias, u, pos.cpu())
    with pytest.raises(RuntimeError, match="GPU"):
        K.causal_conv1d_varlen_fwd(x.cpu(), w, bias, u, pos)
    with pytest.raises(ValueError):  # a position per row
        K.causal_conv1d_varlen_fwd(x, w, bias, u, pos[:-1])
    with pytest.raises(TypeError):
        K.causal_conv1d_varlen_fwd(x, w, bias, u, pos.long())
    assert torch.isnan(u.float()).all()  # nothing was launched

    tables = K.scan_tables(lens, "cuda")
    proj, y = z16(T, R + 2 * N), nan16(T, I)
    ops = (z16(T, I), z16(T, I), torch.zeros(I, device="cuda"), torch.zeros(I, N, device="cuda"),
           proj[:, R:R + N], proj[:, R + N:], torch.zeros(I, device="cuda"), z16(T, I))
    ws = K.workspace(_lib.query("mmpt_selective_scan_varlen_fwd_workspace_bytes",
                                tables.total_chunks, I, N), slot=2)

    def scan(n_seq=2, total=tables.total_chunks, cs=tables.cu_seqlens.data_ptr(),
             ck=tables.cu_chunks.data_ptr()):
        _lib.call("mmpt_selective_scan_varlen_fwd", T, n_seq, total, cs, ck, I, N,
                  ops[0].data_ptr(), I, ops[1].data_ptr(), I, ops[2].data_ptr(), ops[3].data_ptr(),
                  ops[4].data_ptr(), ops[5].data_ptr(), R + 2 * N, ops[6].data_ptr(),
                  ops[7].data_ptr(), I, y.data_ptr(), I, None, ws.data_ptr(), stream)

    with pytest.raises(RuntimeError, match=ERR_ARG):  # table pointers 2 bytes off
        scan(cs=tables.cu_seqlens.data_ptr() + 2)
    with pytest.raises(RuntimeError, match=ERR_ARG):
        scan(ck=tables.cu_chunks.data_ptr() + 2)
    with pytest.raises(RuntimeError, match=ERR_ARG):  # no sequence
        scan(n_seq=0)
    with pytest.raises(RuntimeError, match=ERR_ARG):  # fewer chunks than sequences
        scan(total=1)
    with pytest.raises(RuntimeError, match=ERR_ARG):  # more chunks than T / chunk + n_seq
        scan(total=3)
    with pytest.raises(ValueError, match="cu_seqlens"):  # tables that do not end at T
        K.selective_scan_varlen_fwd(*ops, y, K.scan_tables([3, 4], "cuda"))
    with pytest.raises(ValueError):
        K.scan_tables([], "cuda")
    with pytest.raises(ValueError):
        K.scan_tables([3, 0], "cuda")
    with pytest.raises(ValueError, match="65535"):
        K.scan_tables([1] * 65536, "cuda")
    with pytest.raises(RuntimeError, match="GPU"):
        K.selective_scan_varlen_fwd(ops[0].cpu(), *ops[1:], y, tables)
    cpu_tables = K.scan_tables(lens, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        K.selective_scan_varlen_fwd(*ops, y, cpu_tables)
    c = K.scan_chunk()
    long = K.scan_tables([c + 1], "cuda")
    Tl = c + 1
    acc = fresh_acc(I, N)
    with pytest.raises(ValueError, match="states"):  # two chunks and no states from the forward
        K.selective_scan_varlen_bwd(z16(Tl, I), z16(Tl, I), ops[2], ops[3], z16(Tl, N), z16(Tl, N),
                                    ops[6], z16(Tl, I), z16(Tl, I), nan16(Tl, I), nan16(Tl, I),
                                    nan16(Tl, I), nan16(Tl, N), nan16(Tl, N), *acc, long)
    with pytest.raises(RuntimeError, match="GPU"):
        K.selective_scan_varlen_bwd(*ops, ops[0], nan16(T, I), nan16(T, I), nan16(T, I),
                                    nan16(T, N), nan16(T, N), acc[0].cpu(), acc[1], acc[2], tables)
    assert torch.isnan(y.float()).all()  # nothing was launched
