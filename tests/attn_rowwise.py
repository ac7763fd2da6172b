"""Per-row error bounds for attention against an fp64 reference (test infrastructure only).

A whole-tensor Frobenius norm cannot see the rows where attention kernels go wrong: under a
causal mask the row norm of dK falls by orders of magnitude from the first key to the last, so
the last query rows, the last partial key block and a short sequence of a packed batch weigh
nothing in it.  Here every output row of every (batch, head) is compared with the fp64 result
on a scale of its own:

    ratio = ||got_row - ref_row|| / (2^-8 * row_scale)

`row_scale` is a first-order root-sum-square model of the kernels' rounding points (P -> bf16
before P.V and P^T.dO, O -> bf16 before delta = rowsum(dO * O), dS -> bf16 before dS.K and
dS^T.Q, every output -> bf16); 2^-8 is the bf16 half-ulp bound.  tests/test_attn_rowwise_cpu.py
pins the model with two differently rounded torch implementations (every row <= 1.5) and shows
that it flags the corruptions the whole-tensor norm lets through.  FACTOR = 2.5 is a little
over twice the worst ratio of those torch models; it is not fitted to the HIP kernels.

Shapes: q, dout, O, dQ are [B, H, S, D]; k, v, dK, dV are [B, Hk, S, D] with H = Hk * G (query
head h reads kv head h // G); lse and delta are [B, H, S]; P and dP are [B, H, S, S].
"""

import math
from types import SimpleNamespace

import torch

FACTOR = 2.5
EPS_BF16 = 2.0 ** -8  # round-to-nearest bf16: |x - bf16(x)| <= 2^-8 |x|
BF16 = torch.bfloat16


def _causal_mask(S, device):
    return torch.triu(torch.ones(S, S, device=device, dtype=torch.bool), 1)


def _group_sum(x, G):
    """[B, H, S, D] per query head -> [B, H // G, S, D] summed over each GQA group."""
    B, H, S, D = x.shape
    return x.view(B, H // G, G, S, D).sum(2)


def reference(q, k, v, dout, causal, scale, G=1):
    """fp64 attention forward and backward on the device of the inputs.  Returns O, lse, dQ, dK,
    dV (dK / dV summed over each GQA group) and the intermediates row_scales needs: P,
    dP = dO.V^T, delta = rowsum(dO * O)."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    kr, vr = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    s = (q @ kr.transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(_causal_mask(s.shape[-1], s.device), -math.inf)
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    O = P @ vr
    dP = dout @ vr.transpose(-1, -2)
    delta = (dout * O).sum(-1)
    dS = P * (dP - delta[..., None])
    dQ = scale * (dS @ kr)
    dK = _group_sum(scale * (dS.transpose(-1, -2) @ q), G)
    dV = _group_sum(P.transpose(-1, -2) @ dout, G)
    return SimpleNamespace(O=O, lse=lse, dQ=dQ, dK=dK, dV=dV, P=P, dP=dP, delta=delta)


def lse_fp32(q, k, causal, scale, G=1):
    """The log-sum-exp rows in plain fp32 torch: the reference side's own error, which sets the
    lse tolerance (check_lse)."""
    q, k = q.float(), k.float().repeat_interleave(G, 1)
    s = (q @ k.transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(_causal_mask(s.shape[-1], s.device), -math.inf)
    return torch.logsumexp(s, -1)


def row_scales(ref, q, k, v, dout, scale, G=1):
    """One number per output row: the root-sum-square of the row itself (its final bf16
    rounding) and the first-order effect of each rounding point upstream of it.  ||.|| is the
    2-norm over the head dim; i runs over queries, j over keys of one (batch, head):

        w_ij = scale * P_ij * (|dP_ij| + |delta_i|)   dS_ij rounded to bf16; P_ij inside it
        e_i^2 = sum_d (dO_id * O_id)^2                the rounding of O inside delta_i

        O_i :  sqrt(||O_i||^2  + sum_j P_ij^2 ||V_j||^2)
        dV_j:  sqrt(||dV_j||^2 + sum_i P_ij^2 ||dO_i||^2)
        dQ_i:  sqrt(||dQ_i||^2 + sum_j w_ij^2 ||K_j||^2 + e_i^2 ||scale * sum_j P_ij K_j||^2)
        dK_j:  sqrt(||dK_j||^2 + sum_i (w_ij^2 + (scale * P_ij)^2 e_i^2) ||Q_i||^2)

    For GQA the dK / dV sums run over the query heads of the group as well."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    kr = k.repeat_interleave(G, 1)
    P, dP, delta = ref.P, ref.dP, ref.delta
    n2 = lambda x: (x * x).sum(-1)  # noqa: E731  squared row norms
    P2 = P * P
    w2 = (scale * P * (dP.abs() + delta.abs()[..., None])) ** 2
    e2 = n2(dout * ref.O)
    kn, vn = n2(kr), n2(v.repeat_interleave(G, 1))
    qn, don = n2(q), n2(dout)

    def keys(x):  # [B, H, S_q, S_k] weighted by a per-query [B, H, S_q] -> per key, per group
        B, H, S, _ = x.shape
        return x.view(B, H // G, G, S, S).sum((2, 3))

    o = n2(ref.O) + (P2 * vn[..., None, :]).sum(-1)
    dv = n2(ref.dV) + keys(P2 * don[..., None])
    pk = scale * (P @ kr)
    dq = n2(ref.dQ) + (w2 * kn[..., None, :]).sum(-1) + e2 * n2(pk)
    dk = n2(ref.dK) + keys((w2 + (scale * scale) * P2 * e2[..., None]) * qn[..., None])
    return SimpleNamespace(O=o.sqrt(), dQ=dq.sqrt(), dK=dk.sqrt(), dV=dv.sqrt())


def row_ratios(got, ref, row_scale):
    """||got - ref|| / (2^-8 row_scale) per row ([..., S, D] -> [..., S]); a row whose scale is
    exactly 0 has ratio 0 if it is exactly 0 in `got` and inf otherwise; a NaN counts as inf.
    (dQ of query 0 and dQ / dK of a one-token sequence are exactly 0 in fp64 under a causal
    mask, but their scale is not: w_00 = scale * 2 |delta_0| bounds what a kernel may leave
    there when its dP_00 and delta_0, summed in different orders, do not cancel to the bit.)"""
    err = (got.double() - ref.double()).norm(dim=-1)
    ratio = err / (EPS_BF16 * row_scale)
    zero = row_scale == 0
    exact = (got == 0).all(-1)
    ratio = torch.where(zero, torch.where(exact, 0.0, math.inf).to(ratio.dtype), ratio)
    return torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf)


def check_rows(got, ref, row_scale, factor=FACTOR, what="rows"):
    """Every row of every (batch, head) of got [B, H, S, D] within factor * 2^-8 * row_scale of
    ref; no row is left out.  Raises AssertionError naming the worst (b, h, row, ratio);
    returns the maximum ratio."""
    assert got.shape == ref.shape and row_scale.shape == got.shape[:-1], \
        (what, got.shape, ref.shape, row_scale.shape)
    ratio = row_ratios(got, ref, row_scale)
    worst = float(ratio.max())
    if not worst <= factor:
        b, h, i = (int(x) for x in torch.unravel_index(ratio.argmax(), ratio.shape))
        bad = int((ratio > factor).sum())
        raise AssertionError(
            f"{what}: (b={b}, h={h}, row={i}) has ratio {worst:.3f} > {factor} "
            f"(row scale {float(row_scale[b, h, i]):.3e}; {bad} of {ratio.numel()} rows over)")
    return worst


def lse_tolerance(ref_lse, fp32_lse):
    """Per row: 16 x the largest error of the plain-fp32 rows against fp64 (the 16 allows for the
    MFMA accumulation order and the hardware exp2), floored at 2^-20 (1 + |ref|)."""
    measured = 16.0 * float((fp32_lse.double() - ref_lse).abs().max())
    return torch.clamp(2.0 ** -20 * (1.0 + ref_lse.abs()), min=measured)


def check_lse(got, ref_lse, fp32_lse, what="lse"):
    """Every lse row of got [B, H, S] against the fp64 logsumexp.  Raises AssertionError naming
    the worst row; returns the largest error / tolerance."""
    assert got.shape == ref_lse.shape == fp32_lse.shape, (what, got.shape, ref_lse.shape)
    ratio = (got.double() - ref_lse).abs() / lse_tolerance(ref_lse, fp32_lse)
    ratio = torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf)
    worst = float(ratio.max())
    if not worst <= 1.0:
        b, h, i = (int(x) for x in torch.unravel_index(ratio.argmax(), ratio.shape))
        raise AssertionError(
            f"{what}: (b={b}, h={h}, row={i}) is {float(got[b, h, i])!r}, fp64 "
            f"{float(ref_lse[b, h, i])!r}: {worst:.2f} x its tolerance")
    return worst


# ------------------------------------------------------------------ torch rounding models
def _bf(x):
    return x.to(BF16).float()


def _backward_model(q, kr, vr, dout, O, lse, s, scale, G, fold_scale):
    """The backward of both models: P from lse, P -> bf16 into dV, delta from the bf16 O,
    dS -> bf16 into dQ / dK, outputs bf16.  fold_scale: round scale * dS instead of dS."""
    P = torch.exp(s - lse[..., None])
    Pb = _bf(P)
    dV = _bf(_group_sum(Pb.transpose(-1, -2) @ dout, G))
    delta = (dout * O).sum(-1)
    dS = P * (dout @ vr.transpose(-1, -2) - delta[..., None])
    if fold_scale:
        dS = _bf(dS * scale)
        dQ, dK = dS @ kr, _group_sum(dS.transpose(-1, -2) @ q, G)
    else:
        dS = _bf(dS)
        dQ, dK = scale * (dS @ kr), _group_sum(scale * (dS.transpose(-1, -2) @ q), G)
    return _bf(dQ), _bf(dK), dV


def model_plain(q, k, v, dout, causal, scale, G=1):
    """fp32 torch attention that rounds where the kernels round: one softmax over the whole
    row, exp(s - max) -> bf16 into P.V, the row sum from the unrounded values, O -> bf16."""
    q, k, v, dout = (t.float() for t in (q, k, v, dout))
    kr, vr = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    s = (q @ kr.transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(_causal_mask(s.shape[-1], s.device), -math.inf)
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    O = _bf((_bf(p) @ vr) / l)
    lse = (m + torch.log(l))[..., 0]
    dQ, dK, dV = _backward_model(q, kr, vr, dout, O, lse, s, scale, G, fold_scale=False)
    return SimpleNamespace(O=O, lse=lse, dQ=dQ, dK=dK, dV=dV)


def model_blocked(q, k, v, dout, causal, scale, G=1, block=64):
    """The same operation as a flash sweep: online softmax over key blocks of 64 in the exp2
    domain, the accumulator rescaled at every block, exp2(s - running max) -> bf16 into P.V;
    the backward rounds scale * dS.  A second, differently rounded witness for row_scales."""
    q, k, v, dout = (t.float() for t in (q, k, v, dout))
    kr, vr = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    S = q.shape[-2]
    log2e = 1.4426950408889634
    s = (q @ kr.transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(_causal_mask(S, s.device), -math.inf)
    m = torch.full(s.shape[:-1] + (1,), -math.inf, device=s.device)
    l = torch.zeros_like(m)
    acc = torch.zeros_like(q)
    for j0 in range(0, S, block):
        sb = s[..., j0:j0 + block] * log2e
        m_new = torch.maximum(m, sb.max(-1, keepdim=True).values)
        alive = torch.isfinite(m_new)  # (no key yet under the causal mask: cannot happen for
        # block 0, kept so that the sweep is the general one)
        corr = torch.where(alive, torch.exp2(m - m_new), torch.ones_like(m))
        p = torch.where(alive, torch.exp2(sb - m_new), torch.zeros_like(sb))
        l = l * corr + p.sum(-1, keepdim=True)
        acc = acc * corr + _bf(p) @ vr[..., j0:j0 + block, :]
        m = m_new
    O = _bf(acc / l)
    lse = ((m + torch.log2(l)) / log2e)[..., 0]
    dQ, dK, dV = _backward_model(q, kr, vr, dout, O, lse, s, scale, G, fold_scale=True)
    return SimpleNamespace(O=O, lse=lse, dQ=dQ, dK=dK, dV=dV)
