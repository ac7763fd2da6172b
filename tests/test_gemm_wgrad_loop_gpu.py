"""The K loop of the K_ROWS x K_ROWS gemm4p kernels (the weight gradients): K-tiles in pairs with
the buffer a compile-time constant, the start buffer taken from the K-tile count, transposed
reads off per-lane bases + immediates, the [A0 A1 B0 B1] image order.

Operands are bf16 integers in [-3, 3] and the initial fp32 dw small integers, so every product
and partial sum is exact in fp32 in any order (|Σ| <= 9·K < 2^24): the accumulators hold the fp64
matmul exactly, and the result must match bit for bit what the epilogues are defined to store
(include/mmpt.h: F32_STORE C = f32(bf16(acc)), F32_ACC C += f32(bf16(acc)), split-K slabs summed
in fp32 first) — the fp64 matmul, rounded once to bf16, plus the initial dw.  A wrong fragment
address, buffer or parity is a wrong integer (sums below 256, most of them at these K, are not
rounded at all).  Every case also asserts that a gemm4p K_ROWS x K_ROWS kernel ran.

(Against the unrounded fp64 matmul the parent kernels and these differ alike, by the bf16
rounding alone: 23 of 9.4 M elements at K = 192, 2.3% at K = 1024, each by one bf16 step.)

Shapes: the launch schedule (csrc/gemm_plan.h) gives few tiles to gemm128 — 256-row tiles win
unsplit from 129 tiles on (more than 512 tiles of 128), and with K splits where tiles x splits
fill the CUs — so the small cases run at M = N = 3072 (144 tiles), the split-K ones at 2048
(64 tiles), the edge tiles at 3080 x 2824 and the fused row sums at M = 11008 / 12040."""

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"


@pytest.fixture(scope="module")
def K():
    from multimodal_llm_pretraining_amd import kernels

    return kernels


def _ints(shape, seed, lo=-3, hi=3):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, device=dev, generator=g)


def _plan(K, M, N, Kd, epi):
    from multimodal_llm_pretraining_amd import _lib

    ws = _lib.query("mmpt_gemm_workspace_bytes", M, N, Kd, epi)
    tile, splits = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("mmpt_gemm_plan", M, N, Kd, epi, ws, ctypes.byref(tile), ctypes.byref(splits))
    return tile.value, splits.value


def _check_gemm(K, M, N, Kd, epi, kernel):
    """dw (+)= aᵀ·b on [Kd][M] x [Kd][N] integer operands, against fp64, bit for bit."""
    a = _ints((Kd, M), 3 * Kd + M).to(torch.bfloat16)
    b = _ints((Kd, N), 5 * Kd + N + 1).to(torch.bfloat16)
    dw0 = _ints((M, N), 7 * Kd + 2, -8, 8).float()
    dw = dw0.clone()
    K.gemm(a, b, dw, layout_a=K.K_ROWS, layout_b=K.K_ROWS, epilogue=epi)
    name = K.gemm_last_kernel()
    assert name.startswith(kernel + "<1, 1, "), name
    ref = a.double().t() @ b.double()
    assert ref.abs().max().item() < 2 ** 24
    ref = ref.float().to(torch.bfloat16).double()  # exact in fp32, then the epilogue's bf16(acc)
    if epi == K.EPI_F32_ACC:
        ref += dw0.double()
    bad = dw.double() != ref
    assert not bad.any(), (name, int(bad.sum()), bad.nonzero()[:4].tolist(), dw[bad][:4].tolist(),
                           ref[bad][:4].tolist())
    return name


@pytest.mark.parametrize("epi", ["acc", "store"])
@pytest.mark.parametrize("Kd", [64, 128, 192, 256, 320, 384, 448, 1024])
def test_k_tile_counts(K, Kd, epi):
    """1..7 and 16 K-tiles: odd and even counts (both start buffers), the peeled last two
    K-tiles, fewer than 3 K-tiles (no main loop)."""
    _check_gemm(K, 3072, 3072, Kd, K.EPI_F32_ACC if epi == "acc" else K.EPI_F32_STORE,
                "gemm4p_kernel")


@pytest.mark.parametrize("Kd", [72, 200, 1000])
def test_k_tail_kernel(K, Kd):
    """K % 64 != 0 (K % 8 == 0): the K-tail form, whose last K-tile's pieces past K read zeros."""
    _check_gemm(K, 3072, 3072, Kd, K.EPI_F32_ACC, "gemm4p_kt_kernel")


@pytest.mark.parametrize("Kd", [64 * 101, 64 * 100])
def test_split_k(K, Kd):
    """Split-K as the plan chooses it (4 splits: 26 + 26 + 26 + 23 K-tiles of 101, 25 each of
    100): even and odd K-tile counts per split."""
    tile, splits = _plan(K, 2048, 2048, Kd, K.EPI_F32_ACC)
    assert tile == 256 and splits > 1, (tile, splits)
    name = _check_gemm(K, 2048, 2048, Kd, K.EPI_F32_ACC, "gemm4p_kernel")
    assert name == "gemm4p_kernel<1, 1, 100>", name


@pytest.mark.parametrize("Kd", [192, 320])
def test_more_tiles_than_cus(K, Kd):
    """272 tiles: a workgroup walks a second tile, which starts over in the buffer its own
    K-tile count gives."""
    _check_gemm(K, 4352, 4096, Kd, K.EPI_F32_ACC, "gemm4p_kernel")


def test_edge_tiles(K):
    """8 rows in the last tile row, 8 columns in the last tile column."""
    _check_gemm(K, 3080, 2824, 320, K.EPI_F32_ACC, "gemm4p_kernel")


@pytest.mark.parametrize("T,M,N", [(64 * 37, 11008, 768), (64 * 38, 11008, 768),
                                   (64 * 37, 12040, 768), (64 * 38, 12040, 768),
                                   (64 * 101, 2048, 2048)])  # (the split-K form, 4 splits)
def test_fused_row_sums(K, T, M, N):
    """gemm_wgrad_colsum: the row-sum K-tile ranges [cs_lo, cs_hi) of the tile columns and the
    last column's two weighted K-tiles.  dw exact; dbias the fp64 row sum (an exact integer in
    the fp32 partial sums too) with the same final rounding to bf16."""
    dy = _ints((T, M), T + M).to(torch.bfloat16)
    x = _ints((T, N), T + M + 1).to(torch.bfloat16)
    dw0 = _ints((M, N), T + M + 2, -8, 8).float()
    dw, db = dw0.clone(), torch.zeros(M, device=dev)
    assert K.gemm_wgrad_colsum(dy, x, dw, db), "the fused form did not take the shape"
    name = K.gemm_last_kernel()
    assert name in ("gemm4p_kernel<1, 1, 12>", "gemm4p_kernel<1, 1, 102>"), name
    ref = (dy.double().t() @ x.double()).float().to(torch.bfloat16).double() + dw0.double()
    bad = dw.double() != ref
    assert not bad.any(), (name, int(bad.sum()), bad.nonzero()[:4].tolist())
    sums = dy.double().sum(0)
    assert sums.abs().max().item() < 2 ** 24
    want = sums.float().to(torch.bfloat16).float()
    assert torch.equal(db, want), (name, (db - want).abs().max().item())


@pytest.mark.parametrize("Kd", [320, 384])
def test_reversed_k_walk(K, Kd):
    """MMPT_GEMM_KREV = 1 at 272 tiles: a workgroup's second tile walks its K-tiles last to
    first (a negative step of the running resource bases), at an odd and an even count."""
    from multimodal_llm_pretraining_amd import _lib

    prev = _lib.set_switch("MMPT_GEMM_KREV", 1)
    try:
        _check_gemm(K, 4352, 4096, Kd, K.EPI_F32_ACC, "gemm4p_kernel")
    finally:
        _lib.set_switch("MMPT_GEMM_KREV", prev)


@pytest.mark.parametrize("Kd", [192, 320])
def test_fast_epilogue_staging(K, Kd):
    """The bf16 epilogue of the K_ROWS x K_ROWS form (gemm4p_kernel<1, 1, 0>) at 272 tiles: its
    rows are staged in the A image of the next tile's K-tile 1, which the start buffer moves."""
    M, N = 4352, 4096
    a = _ints((Kd, M), 11 * Kd + 1).to(torch.bfloat16)
    b = _ints((Kd, N), 13 * Kd + 2).to(torch.bfloat16)
    out = torch.full((M, N), 7.0, device=dev, dtype=torch.bfloat16)
    K.gemm(a, b, out, layout_a=K.K_ROWS, layout_b=K.K_ROWS, epilogue=K.EPI_BF16)
    name = K.gemm_last_kernel()
    assert name == "gemm4p_kernel<1, 1, 0>", name
    ref = (a.double().t() @ b.double()).float().to(torch.bfloat16)
    bad = out != ref
    assert not bad.any(), (name, int(bad.sum()), bad.nonzero()[:4].tolist())
