"""Label-smoothed cross entropy (include/mmpt.h K12, mmpt_cross_entropy_smooth): the fp64 row
formulas the kernels implement, as plain torch, and the patch the oracle comparisons use.

With eps the factor and V = vocab_valid, a scored row with logits x and label y has

    loss      = (1 - eps) (lse - x_y) + eps (lse - sum_{v<V} x_v / V)
    dlogits_v = grad_scale (softmax_v - (1 - eps) [v = y] - eps / V)     for v < V, 0 past V

an ignored row has loss 0 and gradient 0, and a label outside [0, V) that is not ignore_index
gives a NaN loss row and a zero gradient.  This is F.cross_entropy(label_smoothing=eps) and HF's
LabelSmoother (tests/test_label_smoothing_cpu.py checks both).
"""

from contextlib import contextmanager

import torch
import torch.nn.functional as F


def ce_rows(logits, labels, eps, vocab_valid=None, ignore_index=-100, grad_scale=1.0):
    """(loss rows [R], dlogits [R, vocab], softmax [R, vocab]) in fp64 from logits [R, vocab] of
    any float dtype; columns past vocab_valid are padding (softmax and gradient 0 there)."""
    x = logits.double()
    R, V = x.shape
    vv = V if vocab_valid is None else int(vocab_valid)
    xv = x[:, :vv]
    ign = labels == ignore_index
    bad = ~ign & ((labels < 0) | (labels >= vv))
    scored = ~(ign | bad)
    lab = labels.clamp(0, vv - 1)[:, None]
    lse = torch.logsumexp(xv, -1)
    nll = lse - xv.gather(1, lab)[:, 0]
    uni = lse - xv.sum(-1) / vv
    loss = torch.where(scored, (1 - eps) * nll + eps * uni, torch.zeros_like(lse))
    loss[bad] = float("nan")
    p = torch.zeros_like(x)
    p[:, :vv] = torch.softmax(xv, -1)
    g = p[:, :vv] - eps / vv
    g.scatter_add_(1, lab, torch.full_like(nll, -(1 - eps))[:, None])
    d = torch.zeros_like(x)
    d[:, :vv] = grad_scale * g * scored[:, None]
    return loss, d, p


@contextmanager
def smoothed_cross_entropy(eps):
    """Inside the block torch.nn.functional.cross_entropy smooths with `eps` (the oracles call
    it through `F.`): the family's oracle, unchanged, computes the smoothed loss."""
    orig = F.cross_entropy

    def smoothed(*args, **kwargs):
        kwargs.setdefault("label_smoothing", eps)
        return orig(*args, **kwargs)

    F.cross_entropy = smoothed
    try:
        yield
    finally:
        F.cross_entropy = orig
