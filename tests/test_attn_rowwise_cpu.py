"""tests/attn_rowwise.py off the GPU: its row-scale model against two differently rounded torch
attention implementations (validity: every row of every output within 1.5 row scales), and the
corruptions that the whole-tensor relative error of test_attention_fwd_bwd lets through, which
check_rows at FACTOR must flag (sensitivity)."""

import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_rowwise as AR  # noqa: E402

VALIDITY = 1.5  # the bound on the torch models; worst ratio over the cases below: 1.22
OLD_O, OLD_GRAD = 1e-2, 2e-2  # test_attention_fwd_bwd's whole-tensor bounds


def relerr(a, b):
    """The whole-tensor measure of tests/test_kernels_gpu.py."""
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@functools.lru_cache(maxsize=None)
def case(S, D, causal, seed, B=2, H=3, G=1):
    """bf16 randn inputs, the fp64 reference, its row scales and both model outputs."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).to(AR.BF16)  # noqa: E731
    q, dout = rnd(B, H, S, D), rnd(B, H, S, D)
    k, v = rnd(B, H // G, S, D), rnd(B, H // G, S, D)
    scale = D ** -0.5
    ref = AR.reference(q, k, v, dout, causal, scale, G)
    rs = AR.row_scales(ref, q, k, v, dout, scale, G)
    models = {"plain": AR.model_plain(q, k, v, dout, causal, scale, G),
              "blocked": AR.model_blocked(q, k, v, dout, causal, scale, G)}
    return dict(q=q, k=k, v=v, dout=dout, scale=scale, ref=ref, rs=rs, models=models,
                lse32=AR.lse_fp32(q, k, causal, scale, G))


CASES = [(S, D, causal, seed) for S in (65, 130, 257) for D in (64, 128)
         for causal in (True, False) for seed in (0, 1)] + [(641, 256, True, 0)]


@pytest.mark.parametrize("S,D,causal,seed", CASES)
def test_row_scale_model_is_valid(S, D, causal, seed):
    """Every row of O, dQ, dK, dV of both torch models within 1.5 row scales of fp64, and their
    fp32 lse within check_lse's tolerance."""
    c = case(S, D, causal, seed)
    for name, m in c["models"].items():
        for what in ("O", "dQ", "dK", "dV"):
            r = AR.check_rows(getattr(m, what), getattr(c["ref"], what), getattr(c["rs"], what),
                              VALIDITY, f"{name} {what}")
            print(f"S={S} D={D} causal={causal} seed={seed} {name} {what}: {r:.3f}")
        AR.check_lse(m.lse, c["ref"].lse, c["lse32"], f"{name} lse")


def test_row_scale_model_gqa_is_valid():
    """G = 2: the dK / dV scales sum over the group's query heads."""
    c = case(130, 64, True, 0, B=1, H=4, G=2)
    for name, m in c["models"].items():
        for what in ("O", "dQ", "dK", "dV"):
            AR.check_rows(getattr(m, what), getattr(c["ref"], what), getattr(c["rs"], what),
                          VALIDITY, f"{name} {what}")


def test_zero_scale_rows_must_be_exactly_zero():
    """A row whose scale is exactly 0 passes only if it is exactly 0.  Causal: dQ of query 0
    (P one-hot, dP = delta) and dQ / dK of a one-token sequence are exactly 0 in fp64 and in the
    models; the row-scale formulas leave them the bound scale * 2 |delta_0| ||K_0||, not 0."""
    c = case(65, 64, True, 0)
    assert (c["ref"].dQ[:, :, 0] == 0).all() and (c["rs"].dQ > 0).all()
    rs = c["rs"].dQ.clone()
    rs[1, 2, 0] = 0
    got = c["models"]["plain"].dQ.clone()
    got[1, 2, 0] = 0  # (the fp32 model's dP_00 - delta_0 does not cancel to the bit either)
    assert AR.check_rows(got, c["ref"].dQ, rs) <= VALIDITY
    got[1, 2, 0, 5] = 1e-30
    with pytest.raises(AssertionError, match=r"b=1, h=2, row=0\)"):
        AR.check_rows(got, c["ref"].dQ, rs)
    one = case(1, 64, True, 0)
    assert (one["ref"].dQ == 0).all() and (one["ref"].dK == 0).all()
    for what in ("O", "dQ", "dK", "dV"):
        AR.check_rows(getattr(one["models"]["plain"], what), getattr(one["ref"], what),
                      getattr(one["rs"], what), VALIDITY)


def test_nan_row_is_flagged():
    c = case(65, 64, False, 0)
    got = c["models"]["plain"].O.clone()
    got[0, 1, 64, 3] = float("nan")
    with pytest.raises(AssertionError, match=r"b=0, h=1, row=64"):
        AR.check_rows(got, c["ref"].O, c["rs"].O)


# ------------------------------------------------------------------ sensitivity
def flagged(c, what, got, old_bound, where):
    """`got` (a corrupted copy of the plain model's output) passes the old whole-tensor bound
    and fails check_rows at FACTOR, in the row that was corrupted."""
    ref = getattr(c["ref"], what)
    clean = getattr(c["models"]["plain"], what)
    assert AR.check_rows(clean, ref, getattr(c["rs"], what)) <= VALIDITY
    old = relerr(got, ref)
    print(f"{what}: whole-tensor relerr {relerr(clean, ref):.2e} -> {old:.2e} corrupted")
    assert old < old_bound, (what, old)
    with pytest.raises(AssertionError, match=where):
        AR.check_rows(got, ref, getattr(c["rs"], what))


@pytest.mark.parametrize("S,D", [(257, 64), (641, 256)])
def test_last_output_row_scaled_is_flagged(S, D):
    c = case(S, D, True, 0)
    got = c["models"]["plain"].O.clone()
    got[:, :, -1] = AR._bf(got[:, :, -1] * 1.1)
    flagged(c, "O", got, OLD_O, rf"row={S - 1}\)")


@pytest.mark.parametrize("S,D", [(257, 64), (641, 256)])
@pytest.mark.parametrize("what", ["dK", "dV"])
def test_last_key_block_zeroed_is_flagged(S, D, what):
    """S % 64 = 1: the last key block is one row, the smallest of all under a causal mask."""
    c = case(S, D, True, 0)
    got = getattr(c["models"]["plain"], what).clone()
    got[:, :, (S - 1) // 64 * 64:] = 0
    flagged(c, what, got, OLD_GRAD, rf"row={S - 1}\)")


def test_last_output_row_from_the_row_above_is_flagged():
    c = case(641, 256, True, 0)
    got = c["models"]["plain"].O.clone()
    got[1, 2, -1] = got[1, 2, -2]
    flagged(c, "O", got, OLD_O, r"b=1, h=2, row=640\)")


def test_dq_rows_from_the_neighbouring_head_are_flagged():
    """16 wrong rows of one head are 4.9e-2 of the whole tensor at B * H = 6 (S = 641, D = 256):
    the old bound does see them there.  It stops seeing them in a batch of the size the
    training step runs (B * H = 512 here, S = 130): about 1.3e-2."""
    c = case(130, 64, True, 0, B=16, H=32)
    got = c["models"]["plain"].dQ.clone()
    got[3, 1, -16:] = got[3, 2, -16:]
    flagged(c, "dQ", got, OLD_GRAD, r"b=3, h=1, row=1(1[4-9]|2[0-9])\)")


def test_lse_row_off_is_flagged():
    """The lse check: the fp32 models pass, one row off by 1e-2 does not."""
    c = case(257, 64, True, 0)
    ref = c["ref"].lse
    for m in c["models"].values():
        assert AR.check_lse(m.lse, ref, c["lse32"]) <= 1.0
    got = c["models"]["blocked"].lse.clone()
    got[1, 0, 200] += 1e-2
    with pytest.raises(AssertionError, match=r"b=1, h=0, row=200\)"):
        AR.check_lse(got, ref, c["lse32"])
