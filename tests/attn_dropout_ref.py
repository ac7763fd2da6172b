"""Attention-probability dropout: the numpy restatement of the mask (include/mmpt.h "K19"), an
fp64 reference that takes a keep mask, its row scales, and the two torch rounding models of
tests/attn_rowwise.py extended by the mask (test infrastructure only).

The mask of (batch b, query head h, query q, key k), positions inside their sequence:

    W    = philox4x32_10(ctr = {(q>>2) | ((k>>2) << 16), b*heads + h, lo32(site), hi32(site)},
                         key = {lo32(seed), hi32(seed)})
    byte = (W.w[q & 3] >> (8 * (k & 3))) & 0xFF;  keep iff byte >= t8 = floor(p * 256)
    p_eff = t8 / 256;  s = float(1 / (1 - p_eff))

The arithmetic (P the undropped softmax, lse unchanged, s = 1 / (1 - p_eff)):

    O = s * sum_k keep*P*V;  dV = s * (keep*P)^T dO;  dS = P * (s*keep*dP - delta);
    delta = rowsum(dO * O) with the dropped O;  dQ = scale * dS K;  dK = scale * dS^T Q.

Row scales: tests/attn_rowwise.row_scales with P replaced by s*keep*P in the O and dV terms and
dP replaced by s*keep*dP in w (the rounding of dS).  The remaining P (the factor of dS, the
delta terms) stays the undropped one: that is the P the kernels multiply by.

The rounding order the HIP kernels ship (include/mmpt.h), which the torch models follow: the
dropped P is zeroed before the bf16 pack, s is folded into the fp32 epilogues of O and dV, and
s*keep is applied to dP in fp32 before the subtraction.

FACTOR: the worst per-row ratio of the two torch models over S in {5, 65, 130}, D = 64,
p in {0.1, 0.5}, causal and not (tests/test_attn_dropout_cpu.py::test_rounding_models_pin) is
1.08 (S = 5, causal, p = 0.5) <= 1.25, so FACTOR stays attn_rowwise.FACTOR = 2.5.  It is derived from the torch models,
never from the HIP kernels.
"""

import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_rowwise as AR  # noqa: E402
from test_dropout_cpu import philox4x32_10  # noqa: E402

FACTOR = AR.FACTOR
MAX_SEQ = 262144


def t8_of(p: float) -> int:
    return int(np.floor(np.float64(p) * 256.0))


def p_eff(p: float) -> float:
    return t8_of(p) / 256.0


def scale_of(p: float) -> np.float32:
    return np.float32(1.0 / (1.0 - np.float64(p_eff(p))))


def keep_mask(batch, heads, seq_q, seq_k, p, seed, site, b0=0) -> np.ndarray:
    """bool [batch, heads, seq_q, seq_k]; batch element i is batch index b0 + i."""
    q = np.arange(seq_q, dtype=np.uint64)[:, None]
    k = np.arange(seq_k, dtype=np.uint64)[None, :]
    c0 = np.broadcast_to((q >> np.uint64(2)) | ((k >> np.uint64(2)) << np.uint64(16)), (seq_q, seq_k))
    out = np.empty((batch, heads, seq_q, seq_k), dtype=bool)
    t8 = t8_of(p)
    for b in range(batch):
        for h in range(heads):
            w = philox4x32_10((c0, (b0 + b) * heads + h, site & 0xFFFFFFFF, (site >> 32) & 0xFFFFFFFF),
                              (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
            w = np.stack(np.broadcast_arrays(*w), 0).astype(np.uint32)  # [4, Sq, Sk]
            word = np.take_along_axis(w, np.broadcast_to((q & np.uint64(3)).astype(np.int64),
                                                         (seq_q, seq_k))[None], 0)[0]
            byte = (word >> ((k & np.uint64(3)) * np.uint64(8)).astype(np.uint32)) & np.uint32(0xFF)
            out[b, h] = byte >= t8
    return out


# ------------------------------------------------------------------ fp64 reference
def reference(q, k, v, dout, causal, scale, keep, s, G=1):
    """tests/attn_rowwise.reference with a keep mask [B, H, S, S] (bool) and the factor s.
    P, dP stay the undropped softmax and dO.V^T; Pd = s*keep*P and dPd = s*keep*dP beside them."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    kr, vr = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    sc = (q @ kr.transpose(-1, -2)) * scale
    if causal:
        sc = sc.masked_fill(AR._causal_mask(sc.shape[-1], sc.device), -math.inf)
    lse = torch.logsumexp(sc, -1)
    P = torch.exp(sc - lse[..., None])
    m = keep.to(P.device).double() * float(s)
    Pd = P * m
    O = Pd @ vr
    dP = dout @ vr.transpose(-1, -2)
    dPd = dP * m
    delta = (dout * O).sum(-1)
    dS = P * (dPd - delta[..., None])
    dQ = scale * (dS @ kr)
    dK = AR._group_sum(scale * (dS.transpose(-1, -2) @ q), G)
    dV = AR._group_sum(Pd.transpose(-1, -2) @ dout, G)
    return SimpleNamespace(O=O, lse=lse, dQ=dQ, dK=dK, dV=dV, P=P, dP=dP, delta=delta, Pd=Pd, dPd=dPd)


def row_scales(ref, q, k, v, dout, scale, G=1):
    """attn_rowwise.row_scales with P -> s*keep*P in the O and dV terms and dP -> s*keep*dP in w."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    kr = k.repeat_interleave(G, 1)
    P, delta = ref.P, ref.delta
    n2 = lambda x: (x * x).sum(-1)  # noqa: E731
    P2, Pd2 = P * P, ref.Pd * ref.Pd
    w2 = (scale * P * (ref.dPd.abs() + delta.abs()[..., None])) ** 2
    e2 = n2(dout * ref.O)
    kn, vn = n2(kr), n2(v.repeat_interleave(G, 1))
    qn, don = n2(q), n2(dout)

    def keys(x):
        B, H, S, _ = x.shape
        return x.view(B, H // G, G, S, S).sum((2, 3))

    o = n2(ref.O) + (Pd2 * vn[..., None, :]).sum(-1)
    dv = n2(ref.dV) + keys(Pd2 * don[..., None])
    pk = scale * (P @ kr)
    dq = n2(ref.dQ) + (w2 * kn[..., None, :]).sum(-1) + e2 * n2(pk)
    dk = n2(ref.dK) + keys((w2 + (scale * scale) * P2 * e2[..., None]) * qn[..., None])
    return SimpleNamespace(O=o.sqrt(), dQ=dq.sqrt(), dK=dk.sqrt(), dV=dv.sqrt())


# ------------------------------------------------------------------ torch rounding models
_bf = AR._bf


def _backward_model(q, kr, vr, dout, O, lse, sc, scale, G, fold_scale, keep, s):
    P = torch.exp(sc - lse[..., None])
    Pb = _bf(torch.where(keep, P, torch.zeros_like(P)))  # zeroed before the bf16 pack
    dV = _bf(AR._group_sum(Pb.transpose(-1, -2) @ dout, G) * s)  # s in the fp32 epilogue
    delta = (dout * O).sum(-1)
    dP = dout @ vr.transpose(-1, -2)
    dS = P * (torch.where(keep, dP * s, torch.zeros_like(dP)) - delta[..., None])
    if fold_scale:
        dS = _bf(dS * scale)
        dQ, dK = dS @ kr, AR._group_sum(dS.transpose(-1, -2) @ q, G)
    else:
        dS = _bf(dS)
        dQ, dK = scale * (dS @ kr), AR._group_sum(scale * (dS.transpose(-1, -2) @ q), G)
    return _bf(dQ), _bf(dK), dV


def model_plain(q, k, v, dout, causal, scale, keep, s, G=1):
    q, k, v, dout = (t.float() for t in (q, k, v, dout))
    s = float(s)
    kr, vr = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    sc = (q @ kr.transpose(-1, -2)) * scale
    if causal:
        sc = sc.masked_fill(AR._causal_mask(sc.shape[-1], sc.device), -math.inf)
    m = sc.max(-1, keepdim=True).values
    p = torch.exp(sc - m)
    l = p.sum(-1, keepdim=True)  # the undropped row sum
    O = _bf((_bf(torch.where(keep, p, torch.zeros_like(p))) @ vr) * ((1.0 / l) * s))
    lse = (m + torch.log(l))[..., 0]
    dQ, dK, dV = _backward_model(q, kr, vr, dout, O, lse, sc, scale, G, False, keep, s)
    return SimpleNamespace(O=O, lse=lse, dQ=dQ, dK=dK, dV=dV)


def model_blocked(q, k, v, dout, causal, scale, keep, s, G=1, block=64):
    q, k, v, dout = (t.float() for t in (q, k, v, dout))
    s = float(s)
    kr, vr = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    S = q.shape[-2]
    log2e = 1.4426950408889634
    sc = (q @ kr.transpose(-1, -2)) * scale
    if causal:
        sc = sc.masked_fill(AR._causal_mask(S, sc.device), -math.inf)
    m = torch.full(sc.shape[:-1] + (1,), -math.inf, device=sc.device)
    l = torch.zeros_like(m)
    acc = torch.zeros_like(q)
    for j0 in range(0, S, block):
        sb = sc[..., j0:j0 + block] * log2e
        m_new = torch.maximum(m, sb.max(-1, keepdim=True).values)
        alive = torch.isfinite(m_new)
        corr = torch.where(alive, torch.exp2(m - m_new), torch.ones_like(m))
        p = torch.where(alive, torch.exp2(sb - m_new), torch.zeros_like(sb))
        l = l * corr + p.sum(-1, keepdim=True)
        pk = torch.where(keep[..., j0:j0 + block], p, torch.zeros_like(p))
        acc = acc * corr + _bf(pk) @ vr[..., j0:j0 + block, :]
        m = m_new
    O = _bf(acc * ((1.0 / l) * s))
    lse = ((m + torch.log2(l)) / log2e)[..., 0]
    dQ, dK, dV = _backward_model(q, kr, vr, dout, O, lse, sc, scale, G, True, keep, s)
    return SimpleNamespace(O=O, lse=lse, dQ=dQ, dK=dK, dV=dV)
