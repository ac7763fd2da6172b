"""Thin tensor-level wrappers over the libmmpt C-ABI (include/mmpt.h).

PyTorch is used only as plumbing here: device memory (the caching allocator),
the current HIP stream and shape bookkeeping.  Every arithmetic operation is a
call into the hand-written HIP library; nothing falls back to ATen.
"""

from __future__ import annotations

import math
import struct
from typing import NamedTuple

import torch

from . import _lib

ROWS_K, K_ROWS = 0, 1
EPI_BF16, EPI_BF16_GELU, EPI_BF16_DGELU, EPI_F32_ACC, EPI_F32_STORE, EPI_F32_RESID, EPI_BF16_DGELU_COLSUM = range(7)
# quick-GELU (CLIP) forms of the GELU epilogues
EPI_BF16_QGELU, EPI_BF16_DQGELU, EPI_BF16_DQGELU_COLSUM = 7, 8, 9
# SwiGLU (Llama MLP) with the gate|up projection in 128-column blocks (include/mmpt.h)
EPI_BF16_SWIGLU, EPI_BF16_DSWIGLU = 10, 11
EPI_F32_ACC_COLSUM = 12

_ws_cache: dict[tuple[int, int, int], torch.Tensor] = {}

# Optional live instrumentation (bench.py roofline): when set, every GEMM launch is
# bracketed by HIP events on its own stream and its algorithmic FLOPs recorded.
_gemm_probe: list | None = None


def start_gemm_probe() -> None:
    global _gemm_probe
    _gemm_probe = []


def stop_gemm_probe() -> list:
    """Returns [(kernel_name, flops, algorithmic_bytes, start_event, end_event, shape,
    stream), ...] (end_event = end of the main GEMM kernel; shape = (M, N, K, epilogue);
    stream = the HIP stream the launch went to); caller synchronizes."""
    global _gemm_probe
    out, _gemm_probe = _gemm_probe or [], None
    return out


def gemm_kernel_name(M: int, N: int, K: int, layout_a: int, layout_b: int, epilogue: int,
                     workspace_bytes: int) -> str:
    """The exact kernel (as rocprofv3 names it) mmpt_gemm_bf16 launches for this problem."""
    import ctypes

    buf = ctypes.create_string_buffer(64)
    _lib.call("mmpt_gemm_kernel_name", layout_a, layout_b, epilogue, M, N, K, workspace_bytes,
              buf, 64)
    return buf.value.decode()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def workspace(nbytes: int, slot: int = 0, device: torch.device | None = None) -> torch.Tensor:
    """Persistent scratch per (device, slot, stream): kernels running concurrently on
    different streams (Engine's weight-gradient stream) never share a workspace."""
    dev = torch.cuda.current_device() if device is None else device.index
    key = (dev, slot, torch.cuda.current_stream(dev).cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=f"cuda:{dev}")
        _ws_cache[key] = ws
    return ws


def _check(t: torch.Tensor, dtype: torch.dtype, name: str) -> None:
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor must live on the GPU (no CPU fallback)")


def _ld(t: torch.Tensor) -> int:
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("expected a 2-D tensor with unit inner stride")
    return t.stride(0)


# ----------------------------------------------------------------------------- GEMM
def gemm(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, *, layout_a: int = ROWS_K,
         layout_b: int = ROWS_K, epilogue: int = EPI_BF16, bias: torch.Tensor | None = None,
         aux: torch.Tensor | None = None, out2: torch.Tensor | None = None) -> torch.Tensor:
    """out = op(a) @ op(b) with a fused epilogue (see include/mmpt.h mmpt_epilogue).

    layout ROWS_K: operand stored [rows][K]; K_ROWS: stored [K][rows].
    """
    _check(a, torch.bfloat16, "gemm.a")
    _check(b, torch.bfloat16, "gemm.b")
    if layout_a == ROWS_K:
        M, K = a.shape
    else:
        K, M = a.shape
    if layout_b == ROWS_K:
        N, Kb = b.shape
    else:
        Kb, N = b.shape
    if K != Kb:
        raise ValueError(f"gemm: K mismatch {K} vs {Kb}")
    want = (M, 2 * N) if epilogue == EPI_BF16_DSWIGLU else (M, N)  # dgate|dup, blocked
    if tuple(out.shape) != want:
        raise ValueError(f"gemm: out shape {tuple(out.shape)} != {want}")
    if epilogue == EPI_BF16_SWIGLU and (out2 is None or tuple(out2.shape) != (M, N // 2)):
        raise ValueError("gemm: SWIGLU needs out2 [M, N/2] (the activation)")
    if epilogue == EPI_BF16_DSWIGLU and (aux is None or tuple(aux.shape) != (M, 2 * N)):
        raise ValueError("gemm: DSWIGLU needs aux [M, 2N] (the forward's gate|up)")
    wsb = _lib.query("mmpt_gemm_workspace_bytes", M, N, K, epilogue)
    ws = workspace(wsb, slot=5) if wsb > 0 else None
    probe = _gemm_probe
    if probe is not None:
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()  # materialise the hipEvent; re-recorded by the library after the main kernel
        ev0.record()
        _lib.load().mmpt_gemm_probe_event(ev1.cuda_event)
    _lib.call(
        "mmpt_gemm_bf16", layout_a, layout_b, epilogue, M, N, K,
        a.data_ptr(), _ld(a), b.data_ptr(), _ld(b), out.data_ptr(), _ld(out),
        _p(bias), _p(aux), 0 if aux is None else _ld(aux),
        _p(out2), 0 if out2 is None else _ld(out2), _p(ws), wsb, _stream(),
    )
    if probe is not None:
        out_b = {EPI_BF16: 2, EPI_BF16_GELU: 4, EPI_BF16_DGELU: 4, EPI_F32_ACC: 8,
                 EPI_F32_STORE: 4, EPI_F32_RESID: 10, EPI_BF16_DGELU_COLSUM: 4,
                 EPI_BF16_QGELU: 4, EPI_BF16_DQGELU: 4, EPI_BF16_DQGELU_COLSUM: 4,
                 EPI_BF16_SWIGLU: 3, EPI_BF16_DSWIGLU: 8, EPI_F32_ACC_COLSUM: 8}[epilogue]
        import ctypes

        name = ctypes.create_string_buffer(64)  # the launch's own choice (alignment included)
        _lib.call("mmpt_gemm_last_kernel_name", name, 64)
        mt = _lib.query("mmpt_gemm_last_tail_rows")  # rows computed by the tail split (if any)
        mm = M - mt
        st = _stream()
        probe.append((name.value.decode(),
                      2.0 * mm * N * K, 2.0 * (mm + N) * K + out_b * mm * N, ev0, ev1,
                      (mm, N, K, epilogue), st))
        if mt > 0:  # the tail: split-K launch + epilogue kernel, from the main launch's end
            ev2 = torch.cuda.Event(enable_timing=True)
            ev2.record()
            probe.append((f"gemm4p_kernel<{layout_a}, {layout_b}, 100>+tail_epi_kernel",
                          2.0 * mt * N * K, 2.0 * (mt + N) * K + out_b * mt * N, ev1, ev2,
                          (mt, N, K, epilogue), st))
    return out


def gemm_last_kernel() -> str:
    """The kernel (with its template arguments) this thread's last `gemm` launched."""
    import ctypes

    name = ctypes.create_string_buffer(64)
    _lib.call("mmpt_gemm_last_kernel_name", name, 64)
    return name.value.decode()


def gemm_dgelu_colsum(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, pre: torch.Tensor,
                      dbias: torch.Tensor, quick: bool = False) -> torch.Tensor:
    """out = bf16(bf16(a @ b^T) * gelu'(pre)) and dbias += bf16(Σ_rows out) — the fc1 input
    gradient and fc1 bias gradient in one GEMM pass (per-tile column sums in the epilogue,
    then a fixed-order reduce)."""
    M, N = out.shape
    rows = _lib.query("mmpt_gemm_colsum_rows", M, N, a.shape[1])
    part = workspace(rows * N * 4, slot=6).view(torch.float32)[: rows * N]
    gemm(a, b, out, epilogue=EPI_BF16_DQGELU_COLSUM if quick else EPI_BF16_DGELU_COLSUM, aux=pre,
         out2=part.view(rows, N))
    _lib.call("mmpt_colsum_f32", rows, N, part.data_ptr(), dbias.data_ptr(), None, 1, _stream())
    return out


def gemm_wgrad_colsum(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, dbias: torch.Tensor,
                      dbias2: torch.Tensor | None = None) -> bool:
    """dw += dyᵀ·x (fp32) and dbias (and dbias2) += bf16(Σ_rows dy) in one GEMM pass
    (EPI_F32_ACC_COLSUM: the weight-gradient GEMM sums the dy fragments its MFMAs read, one
    partial row per K split, then a fixed-order reduce) — addmm backward's grad_weight and
    grad_bias without a second read of dy.  Returns False, having done nothing, when the fused
    form does not take the problem (mmpt_gemm_acc_colsum_rows == 0): use gemm + colsum."""
    T, M = dy.shape
    N = x.shape[1]
    rows = _lib.query("mmpt_gemm_acc_colsum_rows", M, N, T)
    if rows <= 0:
        return False
    part = workspace(rows * M * 4, slot=8).view(torch.float32)[: rows * M].view(rows, M)
    gemm(dy, x, dw, layout_a=K_ROWS, layout_b=K_ROWS, epilogue=EPI_F32_ACC_COLSUM, out2=part)
    _lib.call("mmpt_colsum_f32", rows, M, part.data_ptr(), dbias.data_ptr(), _p(dbias2), 1,
              _stream())
    return True


def colsum(dy: torch.Tensor, dbias: torch.Tensor, accumulate: bool = True,
           dbias2: torch.Tensor | None = None) -> None:
    rows, cols = dy.shape
    ws = workspace(_lib.query("mmpt_colsum_workspace_bytes", rows, cols), slot=1)
    _lib.call("mmpt_colsum_bf16", rows, cols, dy.data_ptr(), _ld(dy), dbias.data_ptr(),
              _p(dbias2), int(accumulate), ws.data_ptr(), _stream())


# ----------------------------------------------------------------------------- LayerNorm
def layernorm_fwd(x: torch.Tensor, w1, b1, eps: float, y1: torch.Tensor, mean: torch.Tensor,
                  rstd: torch.Tensor, w2=None, b2=None, y2: torch.Tensor | None = None) -> None:
    _check(x, torch.float32, "layernorm.x")
    rows, h = x.shape
    _lib.call("mmpt_layernorm_fwd", rows, h, float(eps), x.data_ptr(), _ld(x), w1.data_ptr(),
              b1.data_ptr(), y1.data_ptr(), _p(w2), _p(b2), _p(y2), mean.data_ptr(),
              rstd.data_ptr(), _stream())


def layernorm_bwd(x, mean, rstd, dy1, w1, dx, dw1, db1, dy2=None, w2=None, dw2=None, db2=None,
                  dresid=None, dx_bf16=None, dsum=None, dsum2=None) -> None:
    """dx = dresid + LN'(dy1) (+ LN'(dy2)); dγ/dβ += ...; optionally dx_bf16 = bf16(dx) and
    dsum (+ dsum2) += bf16(Σ_rows bf16(dx)) (fused cast + bias-gradient column sum)."""
    rows, h = x.shape
    ws = workspace(_lib.query("mmpt_layernorm_bwd_ex_workspace_bytes", rows, h), slot=2)
    _lib.call("mmpt_layernorm_bwd_ex", rows, h, x.data_ptr(), _ld(x), mean.data_ptr(),
              rstd.data_ptr(), dy1.data_ptr(), w1.data_ptr(), _p(dy2), _p(w2), _p(dresid),
              dx.data_ptr(), _p(dx_bf16), _p(dw1), _p(db1), _p(dw2), _p(db2), _p(dsum),
              _p(dsum2), ws.data_ptr(), _stream())


def cls_ln_fwd(x: torch.Tensor, batch: int, tokens: int, w, b, eps: float, y: torch.Tensor,
               mean: torch.Tensor, rstd: torch.Tensor) -> None:
    """K18: y[b] = bf16(LN(x[b*tokens]; w, b)) — the final LayerNorm of a classification head on
    the CLS row of each sample.  x fp32 dense [batch*tokens, h]; y bf16 [batch, h] (any row
    stride); mean, rstd fp32 [batch]."""
    _check(x, torch.float32, "cls_ln.x")
    _check(y, torch.bfloat16, "cls_ln.y")
    h = x.shape[1]
    if tuple(x.shape) != (batch * tokens, h) or not x.is_contiguous():
        raise ValueError(f"cls_ln_fwd: x must be dense [{batch * tokens}, h]")
    if tuple(y.shape) != (batch, h) or mean.numel() != batch or rstd.numel() != batch:
        raise ValueError("cls_ln_fwd: y [batch, h], mean / rstd [batch] expected")
    _lib.call("mmpt_cls_ln_fwd", batch, tokens, h, float(eps), x.data_ptr(), w.data_ptr(),
              b.data_ptr(), y.data_ptr(), _ld(y), mean.data_ptr(), rstd.data_ptr(), _stream())


def cls_ln_bwd(x, batch: int, tokens: int, mean, rstd, dy, w, dx, dx_bf16=None, dw=None, db=None,
               dsum=None) -> None:
    """K18 backward in one pass over dx (fp32 dense [batch*tokens, h]) and, if given, dx_bf16:
    row b*tokens = LN'(dy[b]; w), every other row +0; dw / db += the LayerNorm's parameter
    gradients; dsum += bf16(Σ_b bf16(dx[b*tokens])) (needs dx_bf16)."""
    _check(x, torch.float32, "cls_ln.x")
    _check(dy, torch.bfloat16, "cls_ln.dy")
    _check(dx, torch.float32, "cls_ln.dx")
    h = x.shape[1]
    for t, name in ((x, "x"), (dx, "dx"), (dx_bf16, "dx_bf16")):
        if t is not None and (tuple(t.shape) != (batch * tokens, h) or not t.is_contiguous()):
            raise ValueError(f"cls_ln_bwd: {name} must be dense [{batch * tokens}, {h}]")
    if dx_bf16 is not None:
        _check(dx_bf16, torch.bfloat16, "cls_ln.dx_bf16")
    if tuple(dy.shape) != (batch, h) or mean.numel() != batch or rstd.numel() != batch:
        raise ValueError("cls_ln_bwd: dy [batch, h], mean / rstd [batch] expected")
    ws = workspace(_lib.query("mmpt_cls_ln_bwd_workspace_bytes", batch, h), slot=2)
    _lib.call("mmpt_cls_ln_bwd", batch, tokens, h, x.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
              dy.data_ptr(), _ld(dy), w.data_ptr(), dx.data_ptr(), _p(dx_bf16), _p(dw), _p(db),
              _p(dsum), ws.data_ptr(), _stream())


def layernorm_f32_fwd(x, w, b, eps: float, y, mean, rstd) -> None:
    _check(x, torch.float32, "layernorm_f32.x")
    rows, h = x.shape
    _lib.call("mmpt_layernorm_f32_fwd", rows, h, float(eps), x.data_ptr(), w.data_ptr(),
              b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _stream())


def layernorm_f32_bwd(x, mean, rstd, dy, w, dx, dw, db) -> None:
    rows, h = x.shape
    ws = workspace(_lib.query("mmpt_layernorm_bwd_workspace_bytes", rows, h), slot=2)
    _lib.call("mmpt_layernorm_f32_bwd", rows, h, x.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
              dy.data_ptr(), w.data_ptr(), dx.data_ptr(), _p(dw), _p(db), ws.data_ptr(),
              _stream())


# ----------------------------------------------------------------------------- attention
def rope_inplace(qkv: torch.Tensor, seq: int, heads: int, head_dim: int, rot_dims: int,
                 head_stride: int, part_stride: int, cos: torch.Tensor, sin: torch.Tensor,
                 inverse: bool = False, parts: int = 2, offset: int = 0,
                 pos: torch.Tensor | None = None) -> None:
    """Rotate `parts` (2: q and k at part_stride apart; 1: one of them) of `heads` heads
    starting `offset` elements into each qkv row.  pos (device int32 [tokens], each in
    [0, cos.shape[0])): the table row of every token instead of t % seq (unpadded batches;
    `seq` is then unused)."""
    tokens = qkv.shape[0]
    if pos is not None:
        _check(pos, torch.int32, "rope.pos")
        if pos.dim() != 1 or pos.numel() != tokens or not pos.is_contiguous():
            raise ValueError(f"rope: pos must be a contiguous [tokens = {tokens}] vector")
        _lib.call("mmpt_rope_inplace_pos", tokens, heads, head_dim, rot_dims,
                  qkv.data_ptr() + offset * qkv.element_size(), _ld(qkv), head_stride,
                  part_stride, parts, cos.data_ptr(), sin.data_ptr(), cos.shape[0],
                  pos.data_ptr(), int(inverse), _stream())
        return
    _lib.call("mmpt_rope_inplace", tokens, seq, heads, head_dim, rot_dims,
              qkv.data_ptr() + offset * qkv.element_size(), _ld(qkv), head_stride, part_stride,
              parts, cos.data_ptr(), sin.data_ptr(), int(inverse), _stream())


def rmsnorm_fwd(x: torch.Tensor, w, eps: float, y: torch.Tensor, rstd: torch.Tensor) -> None:
    _check(x, torch.float32, "rmsnorm.x")
    rows, h = x.shape
    _lib.call("mmpt_rmsnorm_fwd", rows, h, float(eps), x.data_ptr(), _ld(x), w.data_ptr(),
              y.data_ptr(), rstd.data_ptr(), _stream())


def rmsnorm_bwd(x, rstd, dy, w, dx, dw=None, dresid=None, dx_bf16=None) -> None:
    """dx = dresid + RMS'(dy; w) (dx may alias dresid); dw += Σ dy·x̂; optional bf16 copy."""
    rows, h = x.shape
    ws = workspace(_lib.query("mmpt_rmsnorm_bwd_workspace_bytes", rows, h), slot=2)
    _lib.call("mmpt_rmsnorm_bwd", rows, h, x.data_ptr(), _ld(x), rstd.data_ptr(), dy.data_ptr(),
              w.data_ptr(), _p(dresid), dx.data_ptr(), _p(dx_bf16), _p(dw), ws.data_ptr(), _stream())


def attention_fwd(qkv, batch, seq, heads, head_dim, head_stride, part_stride, causal, scale,
                  out, lse) -> None:
    _lib.call("mmpt_attention_fwd", batch, seq, heads, head_dim, qkv.data_ptr(), _ld(qkv),
              head_stride, part_stride, int(causal), float(scale), out.data_ptr(), _ld(out),
              lse.data_ptr(), _stream())


def attention_bwd(qkv, batch, seq, heads, head_dim, head_stride, part_stride, causal, scale,
                  out, dout, lse, dqkv) -> None:
    ws = workspace(_lib.query("mmpt_attention_bwd_workspace_bytes", batch, seq, heads, head_dim),
                   slot=3)
    _lib.call("mmpt_attention_bwd", batch, seq, heads, head_dim, qkv.data_ptr(), _ld(qkv),
              head_stride, part_stride, int(causal), float(scale), out.data_ptr(),
              dout.data_ptr(), _ld(out), lse.data_ptr(), dqkv.data_ptr(), ws.data_ptr(),
              _stream())


def attention_bwd_rope(qkv, batch, seq, heads, head_dim, head_stride, part_stride, causal, scale,
                       out, dout, lse, dqkv, rot_dims, cos, sin) -> None:
    """attention_bwd + rope_inplace(dqkv, inverse=True) on the q and k parts (one kernel pass
    less at head_dim 256 / 64 rotary dims: the dK / dQ epilogues rotate)."""
    ws = workspace(_lib.query("mmpt_attention_bwd_workspace_bytes", batch, seq, heads, head_dim),
                   slot=3)
    _lib.call("mmpt_attention_bwd_rope", batch, seq, heads, head_dim, qkv.data_ptr(), _ld(qkv),
              head_stride, part_stride, int(causal), float(scale), out.data_ptr(),
              dout.data_ptr(), _ld(out), lse.data_ptr(), dqkv.data_ptr(), ws.data_ptr(),
              rot_dims, cos.data_ptr(), sin.data_ptr(), _stream())


def attention_gqa_fwd(qkv, batch, seq, heads, kv_heads, head_dim, k_offset, v_offset, causal,
                      scale, out, lse) -> None:
    """Llama GQA: q head h at h*head_dim, its kv head h // (heads/kv_heads) at
    k_offset / v_offset + j*head_dim of each fused-qkv row."""
    _lib.call("mmpt_attention_gqa_fwd", batch, seq, heads, kv_heads, head_dim, qkv.data_ptr(),
              _ld(qkv), head_dim, k_offset, v_offset, int(causal), float(scale), out.data_ptr(),
              _ld(out), lse.data_ptr(), _stream())


def attention_gqa_bwd(qkv, batch, seq, heads, kv_heads, head_dim, k_offset, v_offset, causal,
                      scale, out, dout, lse, dqkv) -> None:
    ws = workspace(_lib.query("mmpt_attention_bwd_workspace_bytes", batch, seq, heads, head_dim),
                   slot=3)
    _lib.call("mmpt_attention_gqa_bwd", batch, seq, heads, kv_heads, head_dim, qkv.data_ptr(),
              _ld(qkv), head_dim, k_offset, v_offset, int(causal), float(scale), out.data_ptr(),
              dout.data_ptr(), _ld(out), lse.data_ptr(), dqkv.data_ptr(), ws.data_ptr(), _stream())


def check_seqlens(lens, max_seq: int | None = None) -> tuple[list[int], int, int]:
    """Validate a host-side list of sequence lengths for the varlen entries (their
    `cu_seqlens` contents are the caller's contract).  Returns (lens, total, max_seq)."""
    try:
        ls = [int(x) for x in lens]
    except (TypeError, ValueError):
        raise ValueError("varlen: lens must be a sequence of integers") from None
    if not ls:
        raise ValueError("varlen: empty length list")
    if any(x != y for x, y in zip(ls, lens)):
        raise ValueError("varlen: lengths must be integers")
    if min(ls) < 1:
        raise ValueError(f"varlen: every length must be >= 1 (got {min(ls)})")
    mx = max(ls) if max_seq is None else int(max_seq)
    if max(ls) > mx:
        raise ValueError(f"varlen: length {max(ls)} exceeds max_seq {mx}")
    return ls, sum(ls), mx


def cu_seqlens_of(lens) -> torch.Tensor:
    """Host int32 [len(lens) + 1] row offsets of packed sequences (cu[0] = 0)."""
    ls, _, _ = check_seqlens(lens)
    cu = torch.zeros(len(ls) + 1, dtype=torch.int32)
    cu[1:] = torch.tensor(ls, dtype=torch.int64).cumsum(0).to(torch.int32)
    return cu


def _varlen_args(qkv, lens, cu_seqlens, max_seq):
    ls, total, mx = check_seqlens(lens, max_seq)
    _check(cu_seqlens, torch.int32, "attention_varlen.cu_seqlens")
    if cu_seqlens.dim() != 1 or cu_seqlens.numel() != len(ls) + 1 or \
            not cu_seqlens.is_contiguous():
        raise ValueError(f"varlen: cu_seqlens must be a contiguous [{len(ls) + 1}] vector")
    if qkv.shape[0] < total:
        raise ValueError(f"varlen: qkv has {qkv.shape[0]} rows, the lengths sum to {total}")
    return len(ls), mx, total


def attention_varlen_fwd(qkv, lens, cu_seqlens, heads, kv_heads, head_dim, head_stride, k_offset,
                         v_offset, causal, scale, out, lse, max_seq: int | None = None) -> None:
    """Attention over packed sequences: sequence b is rows [cu[b], cu[b+1]) of qkv / out.
    lens: the host-side lengths (validated here); cu_seqlens: their device int32 prefix sums
    (`cu_seqlens_of(lens)` on the device); lse: fp32 [len(lens) * heads * max_seq].  Layout
    arguments as mmpt_attention_gqa_fwd (GPTNeoX / ViT: kv_heads = heads, k_offset =
    part_stride, v_offset = 2 * part_stride)."""
    batch, mx, total = _varlen_args(qkv, lens, cu_seqlens, max_seq)
    if out.shape[0] < total or lse.numel() < batch * heads * mx:
        raise ValueError("varlen: out / lse too small")
    _lib.call("mmpt_attention_varlen_fwd", batch, mx, total, heads, kv_heads, head_dim,
              qkv.data_ptr(), _ld(qkv), head_stride, k_offset, v_offset, int(causal),
              float(scale), cu_seqlens.data_ptr(), out.data_ptr(), _ld(out), lse.data_ptr(),
              _stream())


def attention_varlen_bwd(qkv, lens, cu_seqlens, heads, kv_heads, head_dim, head_stride, k_offset,
                         v_offset, causal, scale, out, dout, lse, dqkv,
                         max_seq: int | None = None) -> None:
    """Backward of attention_varlen_fwd: every q, k and v element of the first sum(lens) rows
    of dqkv is written once."""
    batch, mx, total = _varlen_args(qkv, lens, cu_seqlens, max_seq)
    if min(out.shape[0], dout.shape[0], dqkv.shape[0]) < total or \
            lse.numel() < batch * heads * mx:
        raise ValueError("varlen: out / dout / dqkv / lse too small")
    if _ld(dqkv) != _ld(qkv) or _ld(dout) != _ld(out):
        raise ValueError("varlen: dqkv / dout must have the row strides of qkv / out")
    ws = workspace(_lib.query("mmpt_attention_varlen_bwd_workspace_bytes", batch, mx, heads,
                              head_dim), slot=3)
    _lib.call("mmpt_attention_varlen_bwd", batch, mx, total, heads, kv_heads, head_dim,
              qkv.data_ptr(), _ld(qkv), head_stride, k_offset, v_offset, int(causal),
              float(scale), cu_seqlens.data_ptr(), out.data_ptr(), dout.data_ptr(), _ld(out),
              lse.data_ptr(), dqkv.data_ptr(), ws.data_ptr(), _stream())


# ------------------------------------------------------- attention-probability dropout (K19)
def attn_dropout_p_eff(p: float) -> float:
    """The probability the 8-bit threshold realises: floor(p * 256) / 256."""
    return float(_lib.query("mmpt_attn_dropout_p_eff", float(p)))


def attn_dropout_mask(batch: int, heads: int, seq_q: int, seq_k: int, p: float, seed: int,
                      site: int, device=None) -> torch.Tensor:
    """Test hook: the keep mask uint8 [batch][heads][seq_q][seq_k] the drop entries apply."""
    keep = torch.empty(batch, heads, seq_q, seq_k, dtype=torch.uint8,
                       device=device or torch.device("cuda", torch.cuda.current_device()))
    _lib.call("mmpt_attn_dropout_mask", batch, heads, seq_q, seq_k, float(p), int(seed),
              int(site), keep.data_ptr(), _stream())
    return keep


def _drop_geometry(qkv, batch, seq, lens, cu_seqlens, max_seq):
    """(batch, max_seq, total, cu pointer) of a drop call: dense (lens is None) or varlen."""
    if lens is None:
        if cu_seqlens is not None:
            raise ValueError("attention_drop: cu_seqlens without lens")
        return int(batch), int(seq), int(batch) * int(seq), None
    b, mx, total = _varlen_args(qkv, lens, cu_seqlens, max_seq)
    return b, mx, total, cu_seqlens.data_ptr()


def attention_drop_fwd(qkv, heads, kv_heads, head_dim, head_stride, k_offset, v_offset, causal,
                       scale, out, lse, p: float, seed: int, site: int, *, batch=None, seq=None,
                       lens=None, cu_seqlens=None, max_seq: int | None = None) -> None:
    """Attention with dropout on the probabilities (mask: include/mmpt.h K19).  Dense: batch, seq;
    varlen: lens, cu_seqlens (as attention_varlen_fwd).  Layout arguments as
    mmpt_attention_gqa_fwd.  lse is the undropped softmax's.  p < 1/256 is the plain entry."""
    b, mx, total, cu = _drop_geometry(qkv, batch, seq, lens, cu_seqlens, max_seq)
    if out.shape[0] < total or lse.numel() < b * heads * mx:
        raise ValueError("attention_drop: out / lse too small")
    _lib.call("mmpt_attention_drop_fwd", b, mx, total, heads, kv_heads, head_dim, qkv.data_ptr(),
              _ld(qkv), head_stride, k_offset, v_offset, int(causal), float(scale), cu,
              out.data_ptr(), _ld(out), lse.data_ptr(), float(p), int(seed), int(site), _stream())


def attention_drop_bwd(qkv, heads, kv_heads, head_dim, head_stride, k_offset, v_offset, causal,
                       scale, out, dout, lse, dqkv, p: float, seed: int, site: int, *, batch=None,
                       seq=None, lens=None, cu_seqlens=None, max_seq: int | None = None) -> None:
    """Backward of attention_drop_fwd with the same (p, seed, site).  No rope backward is fused:
    rotate dqkv afterwards."""
    b, mx, total, cu = _drop_geometry(qkv, batch, seq, lens, cu_seqlens, max_seq)
    if min(out.shape[0], dout.shape[0], dqkv.shape[0]) < total or lse.numel() < b * heads * mx:
        raise ValueError("attention_drop: out / dout / dqkv / lse too small")
    if _ld(dqkv) != _ld(qkv) or _ld(dout) != _ld(out):
        raise ValueError("attention_drop: dqkv / dout must have the row strides of qkv / out")
    ws = workspace(_lib.query("mmpt_attention_drop_bwd_workspace_bytes", b, mx, heads, head_dim,
                              int(cu is not None), float(p)), slot=3)
    _lib.call("mmpt_attention_drop_bwd", b, mx, total, heads, kv_heads, head_dim, qkv.data_ptr(),
              _ld(qkv), head_stride, k_offset, v_offset, int(causal), float(scale), cu,
              out.data_ptr(), dout.data_ptr(), _ld(out), lse.data_ptr(), dqkv.data_ptr(),
              ws.data_ptr(), float(p), int(seed), int(site), _stream())


# ----------------------------------------------------------------------------- loss
def cross_entropy(logits, labels, ignore_index: int, grad_scale: float, loss_rows,
                  dlogits=None, vocab_valid: int | None = None,
                  label_smoothing: float = 0.0) -> None:
    """vocab_valid: logit columns past it are padding (excluded, zero gradient).
    label_smoothing: F.cross_entropy's (eps / vocab_valid on every real class); 0 runs
    mmpt_cross_entropy itself."""
    rows, vocab = logits.shape
    head = (rows, vocab, vocab_valid or vocab, logits.data_ptr(), _ld(logits), labels.data_ptr(),
            ignore_index, float(grad_scale))
    tail = (loss_rows.data_ptr(), _p(dlogits), 0 if dlogits is None else _ld(dlogits), _stream())
    if label_smoothing == 0.0:
        _lib.call("mmpt_cross_entropy", *head, *tail)
    else:
        _lib.call("mmpt_cross_entropy_smooth", *head, float(label_smoothing), *tail)


def sum_f32(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    n = x.numel()
    ws = workspace(_lib.query("mmpt_sum_workspace_bytes", n), slot=4)
    _lib.call("mmpt_sum_f32", n, x.data_ptr(), out.data_ptr(), ws.data_ptr(), _stream())
    return out


def sumsq_f32(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    n = x.numel()
    ws = workspace(_lib.query("mmpt_l2norm_workspace_bytes", n), slot=4)
    _lib.call("mmpt_sumsq_f32", n, x.data_ptr(), out.data_ptr(), ws.data_ptr(), _stream())
    return out


# ----------------------------------------------------------------------------- ZeRO++ quantization
QUANT_BLOCK = 256


def quant_blocks(n_part: int) -> int:
    """fp32 scales per part of n_part elements (256-element blocks, the last one partial)."""
    return -(-n_part // QUANT_BLOCK)


def _quant_args(n_part, parts, *tensors):
    if n_part <= 0 or n_part % 4:
        raise ValueError(f"quantization part of {n_part} elements (need a positive multiple of 4)")
    for t in tensors:
        if not t.is_contiguous():
            raise ValueError("quantization buffers must be contiguous")


def quant_int8(src: torch.Tensor, parts: int, dst: torch.Tensor, scales: torch.Tensor) -> None:
    """bf16 [parts·n] -> int8 [parts·n] + fp32 scales [parts·blocks] (qwZ)."""
    _check(src, torch.bfloat16, "src")
    n = src.numel() // parts
    _quant_args(n, parts, src, dst, scales)
    if dst.dtype != torch.int8 or dst.numel() < parts * n or scales.numel() < parts * quant_blocks(n):
        raise ValueError("quant_int8: dst int8 / scales too small")
    _lib.call("mmpt_quant_int8", n, parts, src.data_ptr(), dst.data_ptr(), scales.data_ptr(), _stream())


def dequant_int8(src: torch.Tensor, scales: torch.Tensor, parts: int, dst: torch.Tensor) -> None:
    _check(dst, torch.bfloat16, "dst")
    n = dst.numel() // parts
    _quant_args(n, parts, src, dst, scales)
    if src.dtype != torch.int8 or src.numel() < parts * n or scales.numel() < parts * quant_blocks(n):
        raise ValueError("dequant_int8: src int8 / scales too small")
    _lib.call("mmpt_dequant_int8", n, parts, src.data_ptr(), scales.data_ptr(), dst.data_ptr(), _stream())


def quant_int4(src: torch.Tensor, parts: int, dst: torch.Tensor, scales: torch.Tensor) -> None:
    """fp32 [parts·n] -> packed int4 uint8 [parts·n/2] + fp32 scales [parts·blocks] (qgZ)."""
    _check(src, torch.float32, "src")
    n = src.numel() // parts
    _quant_args(n, parts, src, dst, scales)
    if dst.dtype != torch.uint8 or dst.numel() < parts * n // 2 or scales.numel() < parts * quant_blocks(n):
        raise ValueError("quant_int4: dst uint8 / scales too small")
    _lib.call("mmpt_quant_int4", n, parts, src.data_ptr(), dst.data_ptr(), scales.data_ptr(), _stream())


def dequant_int4_sum(src: torch.Tensor, scales: torch.Tensor, parts: int, dst: torch.Tensor) -> None:
    """dst (fp32, n) += Σ over the `parts` packed int4 copies of it in src (rank order)."""
    _check(dst, torch.float32, "dst")
    n = dst.numel()
    _quant_args(n, parts, src, dst, scales)
    if src.dtype != torch.uint8 or src.numel() < parts * n // 2 or scales.numel() < parts * quant_blocks(n):
        raise ValueError("dequant_int4_sum: src uint8 / scales too small")
    _lib.call("mmpt_dequant_int4_sum", n, parts, src.data_ptr(), scales.data_ptr(), dst.data_ptr(),
              _stream())


# ----------------------------------------------------------------------------- embeddings
def gather_rows(src, idx, dst) -> None:
    _lib.call("mmpt_gather_rows_bf16", dst.shape[0], dst.shape[1], _p(idx), src.data_ptr(),
              _ld(src), dst.data_ptr(), _ld(dst), _stream())


def expand_rows(src, row_map, dst) -> None:
    _lib.call("mmpt_expand_rows_bf16", dst.shape[0], dst.shape[1], row_map.data_ptr(),
              src.data_ptr(), _ld(src), dst.data_ptr(), _ld(dst), _stream())


class EmbedNoise(NamedTuple):
    """NEFTune noise of one micro-step (include/mmpt.h K8): U(-mag, mag) drawn per element from
    (seed, site); mag = embed_noise_mag(alpha, S_in, hidden)."""
    mag: float
    seed: int
    site: int


def embed_noise_mag(alpha: float, seq_in: int, hidden: int) -> float:
    """alpha / sqrt(S_in * hidden) in double, rounded once to fp32 (returned as a Python float
    that holds the fp32 value)."""
    return struct.unpack("f", struct.pack("f", float(alpha) / math.sqrt(float(seq_in) * hidden)))[0]


def embed_fwd(ids, table, out, img_map=None, img=None, noise: EmbedNoise | None = None) -> None:
    """out[r] = table[ids[r]], or the image feature row where img_map[r] >= 0; with `noise` the
    text rows get the noise added in the same pass (mmpt_embed_noise_fwd)."""
    rows, h = out.shape
    if noise is None:
        _lib.call("mmpt_embed_fwd", rows, h, ids.data_ptr(), table.data_ptr(), _p(img_map),
                  _p(img), out.data_ptr(), _stream())
        return
    _lib.call("mmpt_embed_noise_fwd", rows, h, ids.data_ptr(), table.data_ptr(), _p(img_map),
              _p(img), out.data_ptr(), float(noise.mag), noise.seed & _U64, noise.site & _U64,
              _stream())


def embed_noise(rows: int, h: int, noise: EmbedNoise, device=None) -> torch.Tensor:
    """fp32 [rows, h]: the noise of the logical elements of a site alone (test hook)."""
    out = torch.empty(rows, h, dtype=torch.float32, device="cuda" if device is None else device)
    _lib.call("mmpt_embed_noise", rows, h, float(noise.mag), noise.seed & _U64, noise.site & _U64,
              out.data_ptr(), _stream())
    return out


def embed_segments(ids, vocab: int, skip_id: int = -1):
    """The deterministic embedding-backward order built on the device (mmpt_embed_segments):
    returns (seg_id, seg_off, perm, nseg, bad) int32 device tensors — the text rows (id !=
    skip_id) stably sorted by id, one segment per distinct id, the segment count `nseg` [1]
    and the out-of-range flag `bad` [1] left in device memory (no host synchronisation)."""
    _check(ids, torch.int64, "embed_segments ids")
    rows = ids.numel()
    dev = ids.device
    out = torch.empty(3 * rows + 3, dtype=torch.int32, device=dev)
    seg_id, seg_off = out[:rows], out[rows:2 * rows + 1]
    perm, nseg, bad = out[2 * rows + 1:3 * rows + 1], out[3 * rows + 1:3 * rows + 2], out[3 * rows + 2:]
    wsb = _lib.query("mmpt_embed_segments_workspace_bytes", rows, vocab)
    if wsb < 0:
        raise ValueError(f"embed_segments: unsupported sizes rows={rows} vocab={vocab}")
    ws = workspace(wsb, slot=7, device=dev)
    _lib.call("mmpt_embed_segments", rows, ids.data_ptr(), vocab, skip_id, seg_id.data_ptr(),
              seg_off.data_ptr(), perm.data_ptr(), nseg.data_ptr(), bad.data_ptr(), ws.data_ptr(),
              ws.numel(), _stream())
    return seg_id, seg_off, perm, nseg, bad


def embed_bwd(segments, dout, dtable=None, img_map=None, dimg=None) -> None:
    """segments = (seg_id, seg_off, perm[, nseg, bad]) int32 device tensors: the text rows
    sorted by token id (engine.Batch.segments) — the deterministic scatter-add order.  With
    the device segment count (embed_segments) the kernel reads nseg from HBM."""
    rows, h = dout.shape
    if len(segments) >= 4:
        # device segments (embed_segments): segments longer than 1024 rows are summed over
        # 256-row chunks of the sorted order, then the chunk sums in order (mmpt_embed_bwd_split)
        seg_id, seg_off, perm, nseg = segments[:4]
        n = perm.numel()
        wsb = _lib.query("mmpt_embed_bwd_split_workspace_bytes", max(n, 1), h)
        ws = workspace(wsb, slot=9, device=dout.device) if dtable is not None and n else None
        _lib.call("mmpt_embed_bwd_split", rows, h, n, nseg.data_ptr(), _p(seg_id),
                  _p(seg_off), _p(perm), _p(img_map), dout.data_ptr(), _p(dtable), _p(dimg),
                  _p(ws), 0 if ws is None else ws.numel(), _stream())
        return
    seg_id, seg_off, perm = segments
    _lib.call("mmpt_embed_bwd", rows, h, seg_id.numel(), _p(seg_id), _p(seg_off), _p(perm),
              _p(img_map), dout.data_ptr(), _p(dtable), _p(dimg), _stream())


def im2col(pixels, patch, cols) -> None:
    b, c, s, _ = pixels.shape
    if patch % 8 == 0 and cols.shape[1] == c * patch * patch:
        _lib.call("mmpt_im2col_patches", b, c, s, patch, pixels.data_ptr(), cols.data_ptr(),
                  _stream())
    else:  # CLIP-L/14 etc.: padded K
        _lib.call("mmpt_im2col_patches_ex", b, c, s, patch, pixels.data_ptr(), cols.data_ptr(),
                  _ld(cols), _stream())


def vit_embed_fwd(batch, num_patches, patch_out, cls, pos, out) -> None:
    h = patch_out.shape[-1]
    _lib.call("mmpt_vit_embed_fwd", batch, num_patches, h, patch_out.data_ptr(), cls.data_ptr(),
              pos.data_ptr(), out.data_ptr(), _stream())


def vit_embed_bwd(batch, num_patches, dout, dcls, dpos, dpatch) -> None:
    h = dout.shape[-1]
    _lib.call("mmpt_vit_embed_bwd", batch, num_patches, h, dout.data_ptr(), _p(dcls), _p(dpos),
              _p(dpatch), _stream())


def select_patches_fwd(batch, num_patches, x, out) -> None:
    _lib.call("mmpt_select_patches_fwd", batch, num_patches, x.shape[-1], x.data_ptr(),
              out.data_ptr(), _stream())


def select_patches_bwd(batch, num_patches, dout, dx, accumulate: bool) -> None:
    _lib.call("mmpt_select_patches_bwd", batch, num_patches, dx.shape[-1], dout.data_ptr(),
              dx.data_ptr(), int(accumulate), _stream())


# ----------------------------------------------------------------------------- optimizer
def adam_step(param, grad, exp_avg, exp_avg_sq, param_bf16, *, lr, beta1, beta2, eps,
              weight_decay, adamw: bool, step: int, grad_scale=None, zero_grad: bool = False,
              max_blocks: int = 0) -> None:
    """zero_grad: the kernel also zeroes `grad` as it consumes it (mmpt_adam_step_zero_grad,
    whose grid max_blocks > 0 caps)."""
    args = [param.numel(), param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(),
            exp_avg_sq.data_ptr(), _p(param_bf16), float(lr), float(beta1), float(beta2),
            float(eps), float(weight_decay), int(adamw), int(step), _p(grad_scale)]
    if zero_grad:
        _lib.call("mmpt_adam_step_zero_grad", *args, int(max_blocks), _stream())
    else:
        _lib.call("mmpt_adam_step", *args, _stream())


def clip_coef(sumsq, max_norm: float, coef) -> None:
    _lib.call("mmpt_clip_coef", sumsq.data_ptr(), float(max_norm), coef.data_ptr(), _stream())


def cast_f32_bf16(src, dst) -> None:
    _lib.call("mmpt_cast_f32_bf16", src.numel(), src.data_ptr(), dst.data_ptr(), _stream())


# ----------------------------------------------------------------------------- dropout
# Hidden dropout with the masks recomputed from (seed, site) by a counter-based generator
# (include/mmpt.h K16): seed and site are unsigned 64-bit integers, p a Python float in [0, 1).
_U64 = (1 << 64) - 1


def dropout_bf16(src, dst, p: float, seed: int, site: int) -> None:
    """dst = keep ? bf16(f32(src) * 1/(1-p)) : 0 over a 2-D bf16 tensor (dst may be src); the
    mask follows the logical index row*h + col whatever the row strides.  Forward and backward."""
    _check(src, torch.bfloat16, "dropout_bf16.src")
    _check(dst, torch.bfloat16, "dropout_bf16.dst")
    rows, h = src.shape
    if tuple(dst.shape) != (rows, h):
        raise ValueError("dropout_bf16: dst shape differs from src")
    _lib.call("mmpt_dropout_bf16", rows, h, src.data_ptr(), _ld(src), dst.data_ptr(), _ld(dst),
              float(p), seed & _U64, site & _U64, _stream())


def dropout_f32(src, dst, p: float, seed: int, site: int) -> None:
    """The same on dense fp32 [rows, h] (the embedding outputs and their gradients)."""
    _check(src, torch.float32, "dropout_f32.src")
    _check(dst, torch.float32, "dropout_f32.dst")
    rows, h = src.shape
    if tuple(dst.shape) != (rows, h) or not (src.is_contiguous() and dst.is_contiguous()):
        raise ValueError("dropout_f32: src and dst must be dense [rows, h] of one shape")
    _lib.call("mmpt_dropout_f32", rows, h, src.data_ptr(), dst.data_ptr(), float(p), seed & _U64,
              site & _U64, _stream())


def dropout_add_f32(y, site_y: int, resid, out, p: float, seed: int, y2=None,
                    site_y2: int = 0) -> None:
    """out = resid + f32(v), v = drop(y) or, with y2, bf16(drop(y2) + drop(y)); y, y2 bf16,
    resid / out dense fp32 (out may be resid)."""
    _check(y, torch.bfloat16, "dropout_add_f32.y")
    _check(resid, torch.float32, "dropout_add_f32.resid")
    _check(out, torch.float32, "dropout_add_f32.out")
    rows, h = y.shape
    if y2 is not None:
        _check(y2, torch.bfloat16, "dropout_add_f32.y2")
    for t in (resid, out) + (() if y2 is None else (y2,)):
        if tuple(t.shape) != (rows, h):
            raise ValueError("dropout_add_f32: shapes differ")
    if not (resid.is_contiguous() and out.is_contiguous()):
        raise ValueError("dropout_add_f32: resid and out must be dense")
    _lib.call("mmpt_dropout_add_f32", rows, h, y.data_ptr(), _ld(y), site_y & _U64, _p(y2),
              0 if y2 is None else _ld(y2), site_y2 & _U64, resid.data_ptr(), out.data_ptr(),
              float(p), seed & _U64, _stream())


def dropout_mask(n: int, p: float, seed: int, site: int, device=None) -> torch.Tensor:
    """uint8 [n]: the keep bits of the logical elements 0 .. n-1 of a site (test hook)."""
    keep = torch.empty(n, dtype=torch.uint8, device="cuda" if device is None else device)
    _lib.call("mmpt_dropout_mask", n, float(p), seed & _U64, site & _U64, keep.data_ptr(),
              _stream())
    return keep


def transpose_bf16_batched(src_flat, dst_flat, desc, total_tiles: int) -> None:
    """Every weight's W^T in one launch: desc = device int64 [n, 4] {offset, rows, cols,
    first tile} into the flat bf16 buffers src_flat / dst_flat."""
    _check(desc, torch.int64, "transpose_batched.desc")
    _lib.call("mmpt_transpose_bf16_batched", desc.shape[0], desc.data_ptr(), int(total_tiles),
              src_flat.data_ptr(), dst_flat.data_ptr(), _stream())


def transpose_bf16(src, dst) -> None:
    rows, cols = src.shape
    if tuple(dst.shape) != (cols, rows):
        raise ValueError("transpose: dst must be [cols, rows]")
    _lib.call("mmpt_transpose_bf16", rows, cols, src.data_ptr(), _ld(src), dst.data_ptr(),
              _ld(dst), _stream())


# ----------------------------------------------------------------------------- post-LN (K20)
# RoBERTa's LayerNorm-after-the-residual family (include/mmpt.h K20).  Every tensor is checked
# here; a bad shape raises before anything is launched.
def _dense(t, dtype, shape, name) -> None:
    _check(t, dtype, name)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name}: expected a dense {tuple(shape)} tensor, got {tuple(t.shape)}")


def _rows_bf16(t, rows, h, name) -> int:
    _check(t, torch.bfloat16, name)
    if tuple(t.shape) != (rows, h):
        raise ValueError(f"{name}: expected [{rows}, {h}], got {tuple(t.shape)}")
    return _ld(t)


def add_layernorm_fwd(resid, v, w, b, eps: float, s, y32, y16, mean, rstd, p: float = 0.0,
                      seed: int = 0, site: int = 0) -> None:
    """s = resid + f32(drop(v)); y32 = LN(s); y16 = bf16(y32); mean / rstd per row.  resid, s,
    y32 dense fp32 [rows, h] (s may be resid); v, y16 bf16 (any row stride)."""
    rows, h = resid.shape
    for t, n in ((resid, "resid"), (s, "s"), (y32, "y32")):
        _dense(t, torch.float32, (rows, h), "add_layernorm_fwd." + n)
    ld_v = _rows_bf16(v, rows, h, "add_layernorm_fwd.v")
    ld_y = _rows_bf16(y16, rows, h, "add_layernorm_fwd.y16")
    _lib.call("mmpt_add_layernorm_fwd", rows, h, float(eps), resid.data_ptr(), v.data_ptr(), ld_v,
              w.data_ptr(), b.data_ptr(), s.data_ptr(), y32.data_ptr(), y16.data_ptr(), ld_y,
              mean.data_ptr(), rstd.data_ptr(), float(p), seed & _U64, site & _U64, _stream())


def add_layernorm_bwd(s, mean, rstd, w, ds32, dvb, dy32=None, dyb=None, dw=None, db=None,
                      dsum=None, dsum2=None, p: float = 0.0, seed: int = 0, site: int = 0) -> None:
    """ds32 = LN'(dy32 + f32(dyb)) (may be dy32); dvb = drop(bf16(ds32)); dw / db += the LayerNorm's
    parameter gradients; dsum (and dsum2) += bf16(Σ_rows dvb), the branch Linear's bias gradient."""
    rows, h = s.shape
    _dense(s, torch.float32, (rows, h), "add_layernorm_bwd.s")
    _dense(ds32, torch.float32, (rows, h), "add_layernorm_bwd.ds32")
    if dy32 is not None:
        _dense(dy32, torch.float32, (rows, h), "add_layernorm_bwd.dy32")
    ld_dyb = 0 if dyb is None else _rows_bf16(dyb, rows, h, "add_layernorm_bwd.dyb")
    ld_dvb = _rows_bf16(dvb, rows, h, "add_layernorm_bwd.dvb")
    ws = workspace(_lib.query("mmpt_add_layernorm_bwd_workspace_bytes", rows, h), slot=2)
    _lib.call("mmpt_add_layernorm_bwd", rows, h, s.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
              w.data_ptr(), _p(dy32), _p(dyb), ld_dyb, ds32.data_ptr(), dvb.data_ptr(), ld_dvb,
              _p(dw), _p(db), _p(dsum), _p(dsum2), float(p), seed & _U64, site & _U64,
              ws.data_ptr(), _stream())


def _embed_tables(ids, pos, word, pos_table, type_row, rows, h, name):
    _check(ids, torch.int64, name + ".ids")
    _check(pos, torch.int64, name + ".pos")
    if ids.numel() != rows or pos.numel() != rows or not (ids.is_contiguous() and
                                                          pos.is_contiguous()):
        raise ValueError(f"{name}: ids / pos must be contiguous [{rows}] vectors")
    for t, n in ((word, "word"), (pos_table, "pos_table")):
        _check(t, torch.float32, f"{name}.{n}")
        if t.dim() != 2 or t.shape[1] != h or not t.is_contiguous():
            raise ValueError(f"{name}: {n} must be a dense [*, {h}] table")
    _dense(type_row, torch.float32, (h,), name + ".type_row")


def roberta_embed_fwd(ids, pos, word, pos_table, type_row, w, b, eps: float, h32, h16, mean, rstd,
                      p: float = 0.0, seed: int = 0, site: int = 0,
                      noise: EmbedNoise | None = None) -> None:
    """h32 = drop(LN((word[ids] + type_row) + pos_table[pos])), h16 = bf16(h32); with `noise` the
    word row is word[ids] + noise (mmpt_roberta_embed_noise_fwd)."""
    rows, h = h32.shape
    _embed_tables(ids, pos, word, pos_table, type_row, rows, h, "roberta_embed_fwd")
    _dense(h32, torch.float32, (rows, h), "roberta_embed_fwd.h32")
    _dense(h16, torch.bfloat16, (rows, h), "roberta_embed_fwd.h16")
    args = (rows, h, float(eps), ids.data_ptr(), pos.data_ptr(),
            word.data_ptr(), word.shape[0], pos_table.data_ptr(), pos_table.shape[0],
            type_row.data_ptr(), w.data_ptr(), b.data_ptr(), h32.data_ptr(), h16.data_ptr(),
            mean.data_ptr(), rstd.data_ptr(), float(p), seed & _U64, site & _U64)
    if noise is None:
        _lib.call("mmpt_roberta_embed_fwd", *args, _stream())
    else:
        _lib.call("mmpt_roberta_embed_noise_fwd", *args, float(noise.mag), noise.seed & _U64,
                  noise.site & _U64, _stream())


def roberta_embed_bwd(ids, pos, word, pos_table, type_row, mean, rstd, w, dh, de, dhb=None,
                      dw=None, db=None, dtype=None, p: float = 0.0, seed: int = 0,
                      site: int = 0, noise: EmbedNoise | None = None) -> None:
    """de = LN'(drop(dh + f32(dhb))) over the re-gathered embedding sum (de may be dh); dw / db /
    dtype +=.  `noise`: the forward's, drawn again with the gather."""
    rows, h = dh.shape
    _embed_tables(ids, pos, word, pos_table, type_row, rows, h, "roberta_embed_bwd")
    _dense(dh, torch.float32, (rows, h), "roberta_embed_bwd.dh")
    _dense(de, torch.float32, (rows, h), "roberta_embed_bwd.de")
    if dhb is not None:
        _dense(dhb, torch.bfloat16, (rows, h), "roberta_embed_bwd.dhb")
    ws = workspace(_lib.query("mmpt_roberta_embed_bwd_workspace_bytes", rows, h), slot=2)
    args = (rows, h, ids.data_ptr(), pos.data_ptr(), word.data_ptr(),
            word.shape[0], pos_table.data_ptr(), pos_table.shape[0], type_row.data_ptr(),
            mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), dh.data_ptr(), _p(dhb), de.data_ptr(),
            _p(dw), _p(db), _p(dtype), float(p), seed & _U64, site & _U64)
    if noise is None:
        _lib.call("mmpt_roberta_embed_bwd", *args, ws.data_ptr(), _stream())
    else:
        _lib.call("mmpt_roberta_embed_noise_bwd", *args, float(noise.mag), noise.seed & _U64,
                  noise.site & _U64, ws.data_ptr(), _stream())


def mlm_ln_fwd(g, w, b, eps: float, n16, mean, rstd) -> None:
    """n16 = bf16(LN(f32(g))): the MLM head's LayerNorm over the bf16 GELU output."""
    rows, h = g.shape
    ld_g = _rows_bf16(g, rows, h, "mlm_ln_fwd.g")
    ld_n = _rows_bf16(n16, rows, h, "mlm_ln_fwd.n16")
    _lib.call("mmpt_mlm_ln_fwd", rows, h, float(eps), g.data_ptr(), ld_g, w.data_ptr(),
              b.data_ptr(), n16.data_ptr(), ld_n, mean.data_ptr(), rstd.data_ptr(), _stream())


def mlm_ln_bwd(g, mean, rstd, w, dn16, pre, dpre, dw=None, db=None, dsum=None) -> None:
    """dpre = bf16(bf16(LN'(dn16)) * gelu'(pre)); dw / db += ; dsum += bf16(Σ_rows dpre)."""
    rows, h = g.shape
    ld_g = _rows_bf16(g, rows, h, "mlm_ln_bwd.g")
    ld_dn = _rows_bf16(dn16, rows, h, "mlm_ln_bwd.dn16")
    ld_pre = _rows_bf16(pre, rows, h, "mlm_ln_bwd.pre")
    ld_dp = _rows_bf16(dpre, rows, h, "mlm_ln_bwd.dpre")
    ws = workspace(_lib.query("mmpt_mlm_ln_bwd_workspace_bytes", rows, h), slot=2)
    _lib.call("mmpt_mlm_ln_bwd", rows, h, g.data_ptr(), ld_g, mean.data_ptr(), rstd.data_ptr(),
              w.data_ptr(), dn16.data_ptr(), ld_dn, pre.data_ptr(), ld_pre, dpre.data_ptr(), ld_dp,
              _p(dw), _p(db), _p(dsum), ws.data_ptr(), _stream())


# ----------------------------------------------------------------------------- ConvNeXt (K21)
# NHWC activations as 4-D dense tensors [B, H, W, C]; depthwise weights tap-major [49, C].
def _nhwc(t, dtype, name, shape=None):
    _check(t, dtype, name)
    if t.dim() != 4 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{name}: expected a dense NHWC tensor{'' if shape is None else ' ' + str(tuple(shape))}, "
                         f"got {tuple(t.shape)}")
    return tuple(t.shape)


def dwconv7_fwd(x, w, bias, c) -> None:
    """c = bf16(dwconv7x7(bf16(x); w, bias)), padding 3; x fp32 / c bf16 NHWC, w bf16 [49, C]."""
    B, H, W, C = _nhwc(x, torch.float32, "dwconv7_fwd.x")
    _nhwc(c, torch.bfloat16, "dwconv7_fwd.c", (B, H, W, C))
    _dense(w, torch.bfloat16, (49, C), "dwconv7_fwd.w")
    _dense(bias, torch.bfloat16, (C,), "dwconv7_fwd.bias")
    _lib.call("mmpt_dwconv7_fwd", B, H, W, C, x.data_ptr(), w.data_ptr(), bias.data_ptr(),
              c.data_ptr(), _stream())


def dwconv7_bwd_input(dc, w, dx_out, dx_in=None) -> None:
    """dx_out = dx_in + f32(bf16(dwconv7x7^T(dc; w))); dx_in None = zero, may be dx_out."""
    B, H, W, C = _nhwc(dc, torch.bfloat16, "dwconv7_bwd_input.dc")
    _nhwc(dx_out, torch.float32, "dwconv7_bwd_input.dx_out", (B, H, W, C))
    if dx_in is not None:
        _nhwc(dx_in, torch.float32, "dwconv7_bwd_input.dx_in", (B, H, W, C))
    _dense(w, torch.bfloat16, (49, C), "dwconv7_bwd_input.w")
    _lib.call("mmpt_dwconv7_bwd_input", B, H, W, C, dc.data_ptr(), w.data_ptr(), _p(dx_in),
              dx_out.data_ptr(), _stream())


def dwconv7_bwd_weight(x, dc, dw, db) -> None:
    """dw [49, C] += bf16(Σ dc * bf16(x) shifted), db [C] += bf16(Σ dc): fp32 gradients."""
    B, H, W, C = _nhwc(x, torch.float32, "dwconv7_bwd_weight.x")
    _nhwc(dc, torch.bfloat16, "dwconv7_bwd_weight.dc", (B, H, W, C))
    _dense(dw, torch.float32, (49, C), "dwconv7_bwd_weight.dw")
    _dense(db, torch.float32, (C,), "dwconv7_bwd_weight.db")
    ws = workspace(_lib.query("mmpt_dwconv7_bwd_weight_workspace_bytes", B, H, W, C), slot=2)
    _lib.call("mmpt_dwconv7_bwd_weight", B, H, W, C, x.data_ptr(), dc.data_ptr(), dw.data_ptr(),
              db.data_ptr(), ws.data_ptr(), _stream())


def layerscale_add_fwd(resid, gamma, y, out) -> None:
    """out = resid + gamma * f32(y), two fp32 roundings; out may be resid."""
    rows, C = resid.shape
    _dense(resid, torch.float32, (rows, C), "layerscale_add_fwd.resid")
    _dense(out, torch.float32, (rows, C), "layerscale_add_fwd.out")
    _dense(gamma, torch.float32, (C,), "layerscale_add_fwd.gamma")
    ld_y = _rows_bf16(y, rows, C, "layerscale_add_fwd.y")
    _lib.call("mmpt_layerscale_add_fwd", rows, C, resid.data_ptr(), gamma.data_ptr(), y.data_ptr(),
              ld_y, out.data_ptr(), _stream())


def layerscale_bwd(g, gamma, y, dy, dgamma) -> None:
    """dy = bf16(gamma * g); dgamma += Σ_rows g * f32(y)."""
    rows, C = g.shape
    _dense(g, torch.float32, (rows, C), "layerscale_bwd.g")
    _dense(gamma, torch.float32, (C,), "layerscale_bwd.gamma")
    _dense(dgamma, torch.float32, (C,), "layerscale_bwd.dgamma")
    ld_y = _rows_bf16(y, rows, C, "layerscale_bwd.y")
    ld_dy = _rows_bf16(dy, rows, C, "layerscale_bwd.dy")
    ws = workspace(_lib.query("mmpt_layerscale_bwd_workspace_bytes", rows, C), slot=2)
    _lib.call("mmpt_layerscale_bwd", rows, C, g.data_ptr(), gamma.data_ptr(), y.data_ptr(), ld_y,
              dy.data_ptr(), ld_dy, dgamma.data_ptr(), ws.data_ptr(), _stream())


# Stochastic depth (include/mmpt.h "K21 stochastic depth"): a block runs over its kept samples.
class KeptSamples:
    """The kept samples of one block: `B` planes in the fp32 stream, host `idx` (the kept planes,
    a tuple), `Bk`, and the device int32 tables `idx_dev` [Bk] (compact -> plane) and `slot_dev`
    [B] (plane -> compact, -1 where dropped).  Async copies on the current stream; nothing is
    read back.  `tables`: the two device tables already made (kept_samples_of: one copy for many
    blocks).  The wrappers check the host copy before every launch."""

    def __init__(self, B: int, idx, device, tables=None):
        self.B, self.idx = int(B), tuple(int(i) for i in idx)
        self.Bk = len(self.idx)
        if tables is None:
            both = torch.tensor(self.idx + self.slots(), dtype=torch.int32)
            both = both.to(torch.device(device), non_blocking=True)
            tables = both[:self.Bk], both[self.Bk:]
        self.idx_dev, self.slot_dev = tables
        self.checked = None

    def slots(self) -> tuple:
        slot = [-1] * self.B
        for k, i in enumerate(self.idx):
            if 0 <= i < self.B:
                slot[i] = k
        return tuple(slot)


def kept_samples_of(B: int, idxs, device) -> list:
    """KeptSamples for several blocks at once (`idxs`: one index tuple per block): every table in
    one buffer, staged in pinned memory and copied by one asynchronous copy on the current
    stream, so drawing a micro-step's masks costs neither a launch per block nor a wait."""
    device = torch.device(device)
    ks = [KeptSamples(B, idx, device, tables=(None, None)) for idx in idxs]
    flat = [v for k in ks for v in k.idx + k.slots()]
    host = torch.tensor(flat, dtype=torch.int32)
    if device.type == "cuda":
        host = host.pin_memory()
    dev = host.to(device, non_blocking=True)
    o = 0
    for k in ks:
        k.idx_dev, k.slot_dev = dev[o:o + k.Bk], dev[o + k.Bk:o + k.Bk + B]
        o += k.Bk + B
    return ks


def _kept(kept: KeptSamples, B: int, name: str, empty_ok: bool = False) -> None:
    idx = kept.idx
    if kept.B != B:
        raise ValueError(f"{name}: the sample map is over {kept.B} planes, the stream has {B}")
    if not idx and not empty_ok:
        raise ValueError(f"{name}: no kept sample (1 <= Bk <= B)")
    if kept.checked is idx:  # the host copy is a tuple: one walk per map, not one per launch
        return
    if any(not 0 <= i < B for i in idx) or any(a >= b for a, b in zip(idx, idx[1:])):
        raise ValueError(f"{name}: idx must be strictly increasing within [0, {B}), got {idx}")
    if tuple(kept.idx_dev.shape) != (len(idx),) or tuple(kept.slot_dev.shape) != (B,) or \
            kept.idx_dev.dtype != torch.int32 or kept.slot_dev.dtype != torch.int32:
        raise ValueError(f"{name}: the device tables do not match the host copy")
    kept.checked = idx


def _check_p(p: float, name: str) -> float:
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{name}: p must lie in [0, 1), got {p!r}")
    return float(p)


def dwconv7_idx_fwd(x, kept: KeptSamples, w, bias, c) -> None:
    """dwconv7_fwd over the kept planes: c[b'] = conv(x[idx[b']]); x fp32 [B, H, W, C] read through
    the map, c bf16 compact [Bk, H, W, C]."""
    B, H, W, C = _nhwc(x, torch.float32, "dwconv7_idx_fwd.x")
    _kept(kept, B, "dwconv7_idx_fwd")
    _nhwc(c, torch.bfloat16, "dwconv7_idx_fwd.c", (kept.Bk, H, W, C))
    _dense(w, torch.bfloat16, (49, C), "dwconv7_idx_fwd.w")
    _dense(bias, torch.bfloat16, (C,), "dwconv7_idx_fwd.bias")
    _lib.call("mmpt_dwconv7_idx_fwd", B, kept.Bk, H, W, C, x.data_ptr(), kept.idx_dev.data_ptr(),
              w.data_ptr(), bias.data_ptr(), c.data_ptr(), _stream())


def dwconv7_idx_bwd_input(dc, kept: KeptSamples, w, dx_out, dx_in=None) -> None:
    """dx_out[idx[b']] = dx_in[idx[b']] + f32(bf16(dwconv7x7^T(dc[b']; w))): only the mapped planes
    of the dense fp32 [B, H, W, C] stream are touched; dc bf16 compact [Bk, H, W, C]."""
    B, H, W, C = _nhwc(dx_out, torch.float32, "dwconv7_idx_bwd_input.dx_out")
    _kept(kept, B, "dwconv7_idx_bwd_input")
    _nhwc(dc, torch.bfloat16, "dwconv7_idx_bwd_input.dc", (kept.Bk, H, W, C))
    if dx_in is not None:
        _nhwc(dx_in, torch.float32, "dwconv7_idx_bwd_input.dx_in", (B, H, W, C))
    _dense(w, torch.bfloat16, (49, C), "dwconv7_idx_bwd_input.w")
    _lib.call("mmpt_dwconv7_idx_bwd_input", B, kept.Bk, H, W, C, dc.data_ptr(),
              kept.idx_dev.data_ptr(), w.data_ptr(), _p(dx_in), dx_out.data_ptr(), _stream())


def dwconv7_idx_bwd_weight(x, kept: KeptSamples, dc, dw, db) -> None:
    """dwconv7_bwd_weight over the kept planes: x fp32 [B, H, W, C] through the map, dc compact."""
    B, H, W, C = _nhwc(x, torch.float32, "dwconv7_idx_bwd_weight.x")
    _kept(kept, B, "dwconv7_idx_bwd_weight")
    _nhwc(dc, torch.bfloat16, "dwconv7_idx_bwd_weight.dc", (kept.Bk, H, W, C))
    _dense(dw, torch.float32, (49, C), "dwconv7_idx_bwd_weight.dw")
    _dense(db, torch.float32, (C,), "dwconv7_idx_bwd_weight.db")
    ws = workspace(_lib.query("mmpt_dwconv7_bwd_weight_workspace_bytes", kept.Bk, H, W, C), slot=2)
    _lib.call("mmpt_dwconv7_idx_bwd_weight", B, kept.Bk, H, W, C, x.data_ptr(),
              kept.idx_dev.data_ptr(), dc.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
              _stream())


def droppath_add_fwd(resid, gamma, y, kept: KeptSamples, p: float, out) -> None:
    """ConvNextDropPath on the residual, one pass: a kept plane b gets resid + s * (gamma *
    f32(y[slot[b]])) (three fp32 roundings, s = float(1 / (1 - p))), a dropped plane is copied.
    resid / out fp32 [B, rows_per_sample, C] (out may be resid); y bf16 [Bk * rows_per_sample, C]
    (None when nobody is kept)."""
    _check(resid, torch.float32, "droppath_add_fwd.resid")
    if resid.dim() != 3 or not resid.is_contiguous():
        raise ValueError("droppath_add_fwd.resid: expected a dense [B, rows_per_sample, C] tensor")
    B, rps, C = resid.shape
    _kept(kept, B, "droppath_add_fwd", empty_ok=True)
    _dense(out, torch.float32, (B, rps, C), "droppath_add_fwd.out")
    _dense(gamma, torch.float32, (C,), "droppath_add_fwd.gamma")
    p = _check_p(p, "droppath_add_fwd")
    ld_y = _rows_bf16(y, kept.Bk * rps, C, "droppath_add_fwd.y") if kept.Bk else 0
    _lib.call("mmpt_droppath_add_fwd", B, kept.Bk, rps, C, resid.data_ptr(), gamma.data_ptr(),
              _p(y) if kept.Bk else None, ld_y, kept.slot_dev.data_ptr(), p, out.data_ptr(),
              _stream())


def droppath_bwd(g, kept: KeptSamples, gamma, y, p: float, dy, dgamma) -> None:
    """layerscale_bwd over the kept samples with g' = g * s: dy = bf16(gamma * g') compact,
    dgamma += Σ g' * f32(y) over the kept rows; g fp32 [B, rows_per_sample, C] read through idx."""
    _check(g, torch.float32, "droppath_bwd.g")
    if g.dim() != 3 or not g.is_contiguous():
        raise ValueError("droppath_bwd.g: expected a dense [B, rows_per_sample, C] tensor")
    B, rps, C = g.shape
    _kept(kept, B, "droppath_bwd")
    _dense(gamma, torch.float32, (C,), "droppath_bwd.gamma")
    _dense(dgamma, torch.float32, (C,), "droppath_bwd.dgamma")
    p = _check_p(p, "droppath_bwd")
    ld_y = _rows_bf16(y, kept.Bk * rps, C, "droppath_bwd.y")
    ld_dy = _rows_bf16(dy, kept.Bk * rps, C, "droppath_bwd.dy")
    ws = workspace(_lib.query("mmpt_droppath_bwd_workspace_bytes", kept.Bk, rps, C), slot=2)
    _lib.call("mmpt_droppath_bwd", B, kept.Bk, rps, C, g.data_ptr(), kept.idx_dev.data_ptr(),
              gamma.data_ptr(), y.data_ptr(), ld_y, p, dy.data_ptr(), ld_dy, dgamma.data_ptr(),
              ws.data_ptr(), _stream())


def ln16_bwd(c, mean, rstd, w, dn16, dc, dw=None, db=None) -> None:
    """dc = bf16(LN'(f32(dn16); f32(c))): the backward of mlm_ln_fwd; dw / db +=."""
    rows, h = c.shape
    ld_c = _rows_bf16(c, rows, h, "ln16_bwd.c")
    ld_dn = _rows_bf16(dn16, rows, h, "ln16_bwd.dn16")
    ld_dc = _rows_bf16(dc, rows, h, "ln16_bwd.dc")
    ws = workspace(_lib.query("mmpt_ln16_bwd_workspace_bytes", rows, h), slot=2)
    _lib.call("mmpt_ln16_bwd", rows, h, c.data_ptr(), ld_c, mean.data_ptr(), rstd.data_ptr(),
              w.data_ptr(), dn16.data_ptr(), ld_dn, dc.data_ptr(), ld_dc, _p(dw), _p(db),
              ws.data_ptr(), _stream())


def avgpool_fwd(x, p) -> None:
    """p [B, C] = mean over HW of x [B, HW, C] (fp32)."""
    _check(x, torch.float32, "avgpool_fwd.x")
    if x.dim() != 3 or not x.is_contiguous():
        raise ValueError("avgpool_fwd.x: expected a dense [B, HW, C] tensor")
    B, HW, C = x.shape
    _dense(p, torch.float32, (B, C), "avgpool_fwd.p")
    _lib.call("mmpt_avgpool_fwd", B, HW, C, x.data_ptr(), p.data_ptr(), _stream())


def avgpool_bwd(dp, dx) -> None:
    """dx [B, HW, C] = dp [B, C] / HW on every row."""
    _check(dx, torch.float32, "avgpool_bwd.dx")
    if dx.dim() != 3 or not dx.is_contiguous():
        raise ValueError("avgpool_bwd.dx: expected a dense [B, HW, C] tensor")
    B, HW, C = dx.shape
    _dense(dp, torch.float32, (B, C), "avgpool_bwd.dp")
    _lib.call("mmpt_avgpool_bwd", B, HW, C, dp.data_ptr(), dx.data_ptr(), _stream())


def patchify2_nhwc(x, rows) -> None:
    """rows [B*H/2*W/2, 4C] (columns (ky, kx, c)) from x bf16 [B, H, W, C]."""
    B, H, W, C = _nhwc(x, torch.bfloat16, "patchify2_nhwc.x")
    if H % 2 or W % 2:
        raise ValueError("patchify2_nhwc: H and W must be even")
    _dense(rows, torch.bfloat16, (B * (H // 2) * (W // 2), 4 * C), "patchify2_nhwc.rows")
    _lib.call("mmpt_patchify2_nhwc", B, H, W, C, x.data_ptr(), rows.data_ptr(), _stream())


def unpatchify2_nhwc(rows, dx) -> None:
    """dx fp32 [B, H, W, C] = the inverse permutation of bf16 rows [B*H/2*W/2, 4C]."""
    B, H, W, C = _nhwc(dx, torch.float32, "unpatchify2_nhwc.dx")
    if H % 2 or W % 2:
        raise ValueError("unpatchify2_nhwc: H and W must be even")
    _dense(rows, torch.bfloat16, (B * (H // 2) * (W // 2), 4 * C), "unpatchify2_nhwc.rows")
    _lib.call("mmpt_unpatchify2_nhwc", B, H, W, C, rows.data_ptr(), dx.data_ptr(), _stream())


# ----------------------------------------------------------------------------- Mamba (K22)
# Rows are tokens (b, t): 2-D tensors [B*L, C] with unit inner stride and any row stride, so the
# halves of the in_proj output and the columns of the x_proj output are passed as views.
def scan_chunk() -> int:
    """Tokens per chunk of the selective scan (fixed: it does not depend on L)."""
    return int(_lib.query("mmpt_selective_scan_chunk"))


def _tokens(t, rows, cols, name) -> int:
    ld = _rows_bf16(t, rows, cols, name)
    if rows == 1:  # a single row has no stride to speak of; torch reports anything
        ld = max(ld, cols)
    return ld


def _seq(rows: int, L: int, name: str) -> int:
    if L <= 0 or rows % L:
        raise ValueError(f"{name}: {rows} rows are not a whole number of length-{L} sequences")
    return rows // L


def causal_conv1d_fwd(x, w, bias, u, L: int) -> None:
    """u = bf16(silu(bf16(causal_conv1d(x; w, bias)))): x, u bf16 [B*L, C], w bf16 [4, C]
    tap-major, bias bf16 [C]; sequences of L rows, no tap crosses a sequence start."""
    rows, C = x.shape
    B = _seq(rows, L, "causal_conv1d_fwd")
    ld_x = _tokens(x, rows, C, "causal_conv1d_fwd.x")
    ld_u = _tokens(u, rows, C, "causal_conv1d_fwd.u")
    _dense(w, torch.bfloat16, (4, C), "causal_conv1d_fwd.w")
    _dense(bias, torch.bfloat16, (C,), "causal_conv1d_fwd.bias")
    _lib.call("mmpt_causal_conv1d_fwd", B, L, C, 4, x.data_ptr(), ld_x, w.data_ptr(),
              bias.data_ptr(), u.data_ptr(), ld_u, _stream())


def causal_conv1d_bwd(x, w, bias, du, dx, dw, db, L: int, du2=None) -> None:
    """dx = bf16(conv^T(dc)), dw [4, C] += bf16(Σ dc * x shifted), db [C] += bf16(Σ dc) with
    dc = bf16((du + du2) * silu'(c)), c recomputed from x; dw, db fp32.  du2: a second gradient
    of u (x_proj's input gradient beside the scan's), summed in fp32."""
    rows, C = x.shape
    B = _seq(rows, L, "causal_conv1d_bwd")
    ld_x = _tokens(x, rows, C, "causal_conv1d_bwd.x")
    ld_du = _tokens(du, rows, C, "causal_conv1d_bwd.du")
    ld_dx = _tokens(dx, rows, C, "causal_conv1d_bwd.dx")
    ld_du2 = 0 if du2 is None else _tokens(du2, rows, C, "causal_conv1d_bwd.du2")
    _dense(w, torch.bfloat16, (4, C), "causal_conv1d_bwd.w")
    _dense(bias, torch.bfloat16, (C,), "causal_conv1d_bwd.bias")
    _dense(dw, torch.float32, (4, C), "causal_conv1d_bwd.dw")
    _dense(db, torch.float32, (C,), "causal_conv1d_bwd.db")
    ws = workspace(_lib.query("mmpt_causal_conv1d_bwd_workspace_bytes", B, L, C), slot=2)
    _lib.call("mmpt_causal_conv1d_bwd", B, L, C, 4, x.data_ptr(), ld_x, w.data_ptr(),
              bias.data_ptr(), du.data_ptr(), ld_du, _p(du2), ld_du2, dx.data_ptr(), ld_dx,
              dw.data_ptr(), db.data_ptr(), ws.data_ptr(), _stream())


def scan_states(B: int, L: int, I: int, N: int, device) -> torch.Tensor:
    """An empty tensor for the chunk-entry states the scan's forward hands to its backward."""
    chunks = (L + scan_chunk() - 1) // scan_chunk()
    return torch.empty(B, chunks, I, N, dtype=torch.float32, device=device)


def _scan_operands(name, u, dt_raw, dt_bias, A_log, Bm, Cm, D, z, L):
    rows, I = u.shape
    N = A_log.shape[1] if A_log.dim() == 2 else -1
    B = _seq(rows, L, name)
    ld = [_tokens(u, rows, I, name + ".u"), _tokens(dt_raw, rows, I, name + ".dt_raw"),
          _tokens(Bm, rows, N, name + ".B"), _tokens(Cm, rows, N, name + ".C"),
          _tokens(z, rows, I, name + ".z")]
    if ld[2] != ld[3]:
        raise ValueError(f"{name}: B and C must share a row stride ({ld[2]} vs {ld[3]})")
    _dense(dt_bias, torch.float32, (I,), name + ".dt_bias")
    _dense(A_log, torch.float32, (I, N), name + ".A_log")
    _dense(D, torch.float32, (I,), name + ".D")
    return B, rows, I, N, ld


def selective_scan_fwd(u, dt_raw, dt_bias, A_log, Bm, Cm, D, z, y, L: int, states=None) -> None:
    """y = bf16((Σ_n C h + D u) * silu(z)) with h_t = exp(δ a) h_{t-1} + δ B u,
    δ = softplus(dt_raw + dt_bias), a = -exp(A_log).  u, dt_raw, z, y bf16 [B*L, I]; Bm, Cm bf16
    [B*L, N]; `states` (from scan_states) receives the chunk-entry states for the backward."""
    B, rows, I, N, ld = _scan_operands("selective_scan_fwd", u, dt_raw, dt_bias, A_log, Bm, Cm, D,
                                       z, L)
    ld_y = _tokens(y, rows, I, "selective_scan_fwd.y")
    if states is not None:
        _dense(states, torch.float32, (B, (L + scan_chunk() - 1) // scan_chunk(), I, N),
               "selective_scan_fwd.states")
    ws = workspace(_lib.query("mmpt_selective_scan_fwd_workspace_bytes", B, L, I, N), slot=2)
    _lib.call("mmpt_selective_scan_fwd", B, L, I, N, u.data_ptr(), ld[0], dt_raw.data_ptr(), ld[1],
              dt_bias.data_ptr(), A_log.data_ptr(), Bm.data_ptr(), Cm.data_ptr(), ld[2],
              D.data_ptr(), z.data_ptr(), ld[4], y.data_ptr(), ld_y, _p(states), ws.data_ptr(),
              _stream())


def selective_scan_bwd(u, dt_raw, dt_bias, A_log, Bm, Cm, D, z, dy, du, dz, ddt_raw, dB, dC,
                       dA_log, dD, ddt_bias, L: int, states=None, du_in=None) -> None:
    """The scan's backward: du (= du_in + the scan's gradient), dz, ddt_raw, dB, dC bf16;
    dA_log, dD, ddt_bias fp32, +=.  `states` is what the forward wrote (needed when L exceeds one
    chunk)."""
    name = "selective_scan_bwd"
    B, rows, I, N, ld = _scan_operands(name, u, dt_raw, dt_bias, A_log, Bm, Cm, D, z, L)
    ld_dy = _tokens(dy, rows, I, name + ".dy")
    ld_du = _tokens(du, rows, I, name + ".du")
    ld_dz = _tokens(dz, rows, I, name + ".dz")
    ld_ddt = _tokens(ddt_raw, rows, I, name + ".ddt_raw")
    ld_db = _tokens(dB, rows, N, name + ".dB")
    if _tokens(dC, rows, N, name + ".dC") != ld_db:
        raise ValueError(f"{name}: dB and dC must share a row stride")
    ld_dui = 0 if du_in is None else _tokens(du_in, rows, I, name + ".du_in")
    _dense(dA_log, torch.float32, (I, N), name + ".dA_log")
    _dense(dD, torch.float32, (I,), name + ".dD")
    _dense(ddt_bias, torch.float32, (I,), name + ".ddt_bias")
    chunks = (L + scan_chunk() - 1) // scan_chunk()
    if states is not None:
        _dense(states, torch.float32, (B, chunks, I, N), name + ".states")
    elif chunks > 1:
        raise ValueError(f"{name}: L = {L} spans {chunks} chunks: the forward's states are needed")
    ws = workspace(_lib.query("mmpt_selective_scan_bwd_workspace_bytes", B, L, I, N), slot=2)
    _lib.call("mmpt_selective_scan_bwd", B, L, I, N, u.data_ptr(), ld[0], dt_raw.data_ptr(), ld[1],
              dt_bias.data_ptr(), A_log.data_ptr(), Bm.data_ptr(), Cm.data_ptr(), ld[2],
              D.data_ptr(), z.data_ptr(), ld[4], _p(states), dy.data_ptr(), ld_dy, _p(du_in),
              ld_dui, du.data_ptr(), ld_du, dz.data_ptr(), ld_dz, ddt_raw.data_ptr(), ld_ddt,
              dB.data_ptr(), dC.data_ptr(), ld_db, dA_log.data_ptr(), dD.data_ptr(),
              ddt_bias.data_ptr(), ws.data_ptr(), _stream())


# Varlen forms: the rows are n_seq sequences laid end to end (a Batch built from position_ids or a
# padding mask).  The conv takes each token's position inside its sequence; the scan takes the
# tables of `scan_tables`, built once per batch.
class ScanTables:
    """Geometry of a packed batch for the varlen scan: host `lens`, device int32 `cu_seqlens`
    [n_seq + 1] (row offsets) and `cu_chunks` [n_seq + 1] (chunk offsets: sequence s has
    ceil(len_s / scan_chunk()) chunks, counted from its own start), T and total_chunks."""

    def __init__(self, lens, device, chunk: int | None = None):
        ls, total, _ = check_seqlens(lens)
        if len(ls) > 65535:
            raise ValueError(f"varlen scan: {len(ls)} sequences; at most 65535")
        c = scan_chunk() if chunk is None else int(chunk)
        self.lens, self.n_seq, self.T = ls, len(ls), total
        cu = torch.zeros(len(ls) + 1, dtype=torch.int64)
        cu[1:] = torch.tensor(ls, dtype=torch.int64).cumsum(0)
        cc = torch.zeros(len(ls) + 1, dtype=torch.int64)
        cc[1:] = torch.tensor([(n + c - 1) // c for n in ls], dtype=torch.int64).cumsum(0)
        self.total_chunks = int(cc[-1])
        device = torch.device(device)
        self.cu_seqlens = cu.to(torch.int32).to(device, non_blocking=True)
        self.cu_chunks = cc.to(torch.int32).to(device, non_blocking=True)


def scan_tables(lens, device) -> ScanTables:
    """The varlen scan's tables for sequences of `lens` rows (async copies on the current
    stream; nothing is read back)."""
    return ScanTables(lens, device)


def _pos_table(pos, rows, name) -> None:
    _check(pos, torch.int32, name)
    if tuple(pos.shape) != (rows,) or not pos.is_contiguous():
        raise ValueError(f"{name}: expected a dense int32 [{rows}] tensor, got {tuple(pos.shape)}")


def causal_conv1d_varlen_fwd(x, w, bias, u, pos) -> None:
    """causal_conv1d_fwd over packed rows: pos int32 [T], each token's position inside its
    sequence; tap t-j is taken iff pos[t] >= j."""
    name = "causal_conv1d_varlen_fwd"
    rows, C = x.shape
    ld_x = _tokens(x, rows, C, name + ".x")
    ld_u = _tokens(u, rows, C, name + ".u")
    _dense(w, torch.bfloat16, (4, C), name + ".w")
    _dense(bias, torch.bfloat16, (C,), name + ".bias")
    _pos_table(pos, rows, name + ".pos")
    _lib.call("mmpt_causal_conv1d_varlen_fwd", rows, C, 4, pos.data_ptr(), x.data_ptr(), ld_x,
              w.data_ptr(), bias.data_ptr(), u.data_ptr(), ld_u, _stream())


def causal_conv1d_varlen_bwd(x, w, bias, du, dx, dw, db, pos, du2=None) -> None:
    """causal_conv1d_bwd over packed rows (pos as in causal_conv1d_varlen_fwd): for dx, tap t+j is
    taken iff t+j < T and pos[t+j] >= j; dw, db fp32, +=."""
    name = "causal_conv1d_varlen_bwd"
    rows, C = x.shape
    ld_x = _tokens(x, rows, C, name + ".x")
    ld_du = _tokens(du, rows, C, name + ".du")
    ld_dx = _tokens(dx, rows, C, name + ".dx")
    ld_du2 = 0 if du2 is None else _tokens(du2, rows, C, name + ".du2")
    _dense(w, torch.bfloat16, (4, C), name + ".w")
    _dense(bias, torch.bfloat16, (C,), name + ".bias")
    _dense(dw, torch.float32, (4, C), name + ".dw")
    _dense(db, torch.float32, (C,), name + ".db")
    _pos_table(pos, rows, name + ".pos")
    ws = workspace(_lib.query("mmpt_causal_conv1d_varlen_bwd_workspace_bytes", rows, C), slot=2)
    _lib.call("mmpt_causal_conv1d_varlen_bwd", rows, C, 4, pos.data_ptr(), x.data_ptr(), ld_x,
              w.data_ptr(), bias.data_ptr(), du.data_ptr(), ld_du, _p(du2), ld_du2, dx.data_ptr(),
              ld_dx, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), _stream())


def scan_varlen_states(tables: ScanTables, I: int, N: int, device) -> torch.Tensor:
    """An empty tensor for the chunk-entry states of a varlen scan: [total_chunks, I, N]."""
    return torch.empty(tables.total_chunks, I, N, dtype=torch.float32, device=device)


def _scan_varlen_geo(name, tables, rows):
    if not isinstance(tables, ScanTables):
        raise TypeError(f"{name}: tables must come from scan_tables()")
    _check(tables.cu_seqlens, torch.int32, name + ".cu_seqlens")
    _check(tables.cu_chunks, torch.int32, name + ".cu_chunks")
    if tables.T != rows:  # the tables' own contents are checked here, on the host copy
        raise ValueError(f"{name}: cu_seqlens ends at {tables.T}, the operands have {rows} rows")
    return rows, tables.n_seq, tables.total_chunks, tables.cu_seqlens.data_ptr(), \
        tables.cu_chunks.data_ptr()


def selective_scan_varlen_fwd(u, dt_raw, dt_bias, A_log, Bm, Cm, D, z, y, tables: ScanTables,
                              states=None) -> None:
    """selective_scan_fwd over packed rows: every sequence of `tables` starts from h = 0 and its
    chunks are counted from its own start.  `states` from scan_varlen_states."""
    name = "selective_scan_varlen_fwd"
    _, rows, I, N, ld = _scan_operands(name, u, dt_raw, dt_bias, A_log, Bm, Cm, D, z, u.shape[0])
    geo = _scan_varlen_geo(name, tables, rows)
    ld_y = _tokens(y, rows, I, name + ".y")
    if states is not None:
        _dense(states, torch.float32, (tables.total_chunks, I, N), name + ".states")
    ws = workspace(_lib.query("mmpt_selective_scan_varlen_fwd_workspace_bytes", geo[2], I, N),
                   slot=2)
    _lib.call("mmpt_selective_scan_varlen_fwd", *geo, I, N, u.data_ptr(), ld[0],
              dt_raw.data_ptr(), ld[1], dt_bias.data_ptr(), A_log.data_ptr(), Bm.data_ptr(),
              Cm.data_ptr(), ld[2], D.data_ptr(), z.data_ptr(), ld[4], y.data_ptr(), ld_y,
              _p(states), ws.data_ptr(), _stream())


def selective_scan_varlen_bwd(u, dt_raw, dt_bias, A_log, Bm, Cm, D, z, dy, du, dz, ddt_raw, dB, dC,
                              dA_log, dD, ddt_bias, tables: ScanTables, states=None,
                              du_in=None) -> None:
    """selective_scan_bwd over packed rows; `states` is what the varlen forward wrote (needed
    when a sequence exceeds one chunk)."""
    name = "selective_scan_varlen_bwd"
    _, rows, I, N, ld = _scan_operands(name, u, dt_raw, dt_bias, A_log, Bm, Cm, D, z, u.shape[0])
    geo = _scan_varlen_geo(name, tables, rows)
    ld_dy = _tokens(dy, rows, I, name + ".dy")
    ld_du = _tokens(du, rows, I, name + ".du")
    ld_dz = _tokens(dz, rows, I, name + ".dz")
    ld_ddt = _tokens(ddt_raw, rows, I, name + ".ddt_raw")
    ld_db = _tokens(dB, rows, N, name + ".dB")
    if _tokens(dC, rows, N, name + ".dC") != ld_db:
        raise ValueError(f"{name}: dB and dC must share a row stride")
    ld_dui = 0 if du_in is None else _tokens(du_in, rows, I, name + ".du_in")
    _dense(dA_log, torch.float32, (I, N), name + ".dA_log")
    _dense(dD, torch.float32, (I,), name + ".dD")
    _dense(ddt_bias, torch.float32, (I,), name + ".ddt_bias")
    if states is not None:
        _dense(states, torch.float32, (tables.total_chunks, I, N), name + ".states")
    elif tables.total_chunks > tables.n_seq:
        raise ValueError(f"{name}: a sequence spans several chunks: the forward's states are "
                         "needed")
    ws = workspace(_lib.query("mmpt_selective_scan_varlen_bwd_workspace_bytes", rows, geo[2], I,
                              N), slot=2)
    _lib.call("mmpt_selective_scan_varlen_bwd", *geo, I, N, u.data_ptr(), ld[0],
              dt_raw.data_ptr(), ld[1], dt_bias.data_ptr(), A_log.data_ptr(), Bm.data_ptr(),
              Cm.data_ptr(), ld[2], D.data_ptr(), z.data_ptr(), ld[4], _p(states), dy.data_ptr(),
              ld_dy, _p(du_in), ld_dui, du.data_ptr(), ld_du, dz.data_ptr(), ld_dz,
              ddt_raw.data_ptr(), ld_ddt, dB.data_ptr(), dC.data_ptr(), ld_db, dA_log.data_ptr(),
              dD.data_ptr(), ddt_bias.data_ptr(), ws.data_ptr(), _stream())
