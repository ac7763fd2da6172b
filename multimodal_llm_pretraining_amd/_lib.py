"""ctypes binding of libmmpt.so — the C-ABI declared in include/mmpt.h.

The library is the product path: there is no Python/PyTorch fallback.  If the
shared object is missing or was built for another ABI version, every op raises
``RuntimeError`` (loud failure, never a silent eager fallback).
"""

from __future__ import annotations

import ctypes
import os
from ctypes import c_double, c_float, c_int, c_int64, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMPT_LIB") or os.path.join(_HERE, "lib", "libmmpt.so")
ABI_VERSION = 16

_lib: ctypes.CDLL | None = None

P = c_void_p
I64 = c_int64
I32 = c_int
F32 = c_float
F64 = c_double
U64 = c_uint64

# name -> (restype, argtypes); mirrors include/mmpt.h one to one.
SIGNATURES: dict[str, tuple] = {
    "mmpt_abi_version": (I32, []),
    "mmpt_last_error": (ctypes.c_char_p, []),
    "mmpt_device_info": (I32, [P, P, P]),
    "mmpt_set_switch": (I32, [ctypes.c_char_p, I32]),
    "mmpt_gemm_workspace_bytes": (I64, [I64, I64, I64, I32]),
    "mmpt_gemm_bf16": (I32, [I32, I32, I32, I64, I64, I64, P, I64, P, I64, P, I64, P, P, I64, P, I64, P, I64, P]),
    "mmpt_gemm_plan": (I32, [I64, I64, I64, I32, I64, P, P]),
    "mmpt_gemm_probe_event": (None, [P]),
    "mmpt_gemm_kernel_name": (I32, [I32, I32, I32, I64, I64, I64, I64, ctypes.c_char_p, I32]),
    "mmpt_gemm_last_kernel_name": (I32, [ctypes.c_char_p, I32]),
    "mmpt_gemm_last_tail_rows": (I64, []),
    "mmpt_gemm_colsum_rows": (I64, [I64, I64, I64]),
    "mmpt_gemm_acc_colsum_rows": (I64, [I64, I64, I64]),
    "mmpt_colsum_f32": (I32, [I64, I64, P, P, P, I32, P]),
    "mmpt_colsum_workspace_bytes": (I64, [I64, I64]),
    "mmpt_colsum_bf16": (I32, [I64, I64, P, I64, P, P, I32, P, P]),
    "mmpt_layernorm_fwd": (I32, [I64, I64, F32, P, I64, P, P, P, P, P, P, P, P, P]),
    "mmpt_layernorm_bwd_workspace_bytes": (I64, [I64, I64]),
    "mmpt_layernorm_bwd": (I32, [I64, I64, P, I64, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    "mmpt_layernorm_bwd_ex_workspace_bytes": (I64, [I64, I64]),
    "mmpt_layernorm_bwd_ex": (I32, [I64, I64, P, I64, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    "mmpt_layernorm_f32_fwd": (I32, [I64, I64, F32, P, P, P, P, P, P, P]),
    "mmpt_layernorm_f32_bwd": (I32, [I64, I64, P, P, P, P, P, P, P, P, P, P]),
    "mmpt_rope_inplace": (I32, [I64, I64, I64, I64, I64, P, I64, I64, I64, I64, P, P, I32, P]),
    "mmpt_rope_inplace_pos": (I32, [I64, I64, I64, I64, P, I64, I64, I64, I64, P, P, I64, P, I32, P]),
    "mmpt_rmsnorm_fwd": (I32, [I64, I64, F32, P, I64, P, P, P, P]),
    "mmpt_rmsnorm_bwd_workspace_bytes": (I64, [I64, I64]),
    "mmpt_rmsnorm_bwd": (I32, [I64, I64, P, I64, P, P, P, P, P, P, P, P, P]),
    "mmpt_attention_fwd": (I32, [I64, I64, I64, I64, P, I64, I64, I64, I32, F32, P, I64, P, P]),
    "mmpt_attention_bwd_workspace_bytes": (I64, [I64, I64, I64, I64]),
    "mmpt_attention_bwd": (I32, [I64, I64, I64, I64, P, I64, I64, I64, I32, F32, P, P, I64, P, P, P, P]),
    "mmpt_attention_bwd_rope": (I32, [I64, I64, I64, I64, P, I64, I64, I64, I32, F32, P, P, I64, P, P, P, I64, P, P, P]),
    "mmpt_attention_gqa_fwd": (I32, [I64, I64, I64, I64, I64, P, I64, I64, I64, I64, I32, F32, P, I64, P, P]),
    "mmpt_attention_gqa_bwd": (I32, [I64, I64, I64, I64, I64, P, I64, I64, I64, I64, I32, F32, P, P, I64, P, P, P, P]),
    "mmpt_attention_varlen_fwd": (I32, [I64, I64, I64, I64, I64, I64, P, I64, I64, I64, I64, I32, F32, P, P, I64, P, P]),
    "mmpt_attention_varlen_bwd_workspace_bytes": (I64, [I64, I64, I64, I64]),
    "mmpt_attention_varlen_bwd": (I32, [I64, I64, I64, I64, I64, I64, P, I64, I64, I64, I64, I32, F32, P, P, P, I64, P, P, P, P]),
    "mmpt_cross_entropy": (I32, [I64, I64, I64, P, I64, P, I64, F32, P, P, I64, P]),
    "mmpt_cross_entropy_smooth": (I32, [I64, I64, I64, P, I64, P, I64, F32, F32, P, P, I64, P]),
    "mmpt_sum_workspace_bytes": (I64, [I64]),
    "mmpt_sum_f32": (I32, [I64, P, P, P, P]),
    "mmpt_gather_rows_bf16": (I32, [I64, I64, P, P, I64, P, I64, P]),
    "mmpt_quant_blocks": (I64, [I64]),
    "mmpt_quant_int8": (I32, [I64, I64, P, P, P, P]),
    "mmpt_dequant_int8": (I32, [I64, I64, P, P, P, P]),
    "mmpt_quant_int4": (I32, [I64, I64, P, P, P, P]),
    "mmpt_dequant_int4_sum": (I32, [I64, I64, P, P, P, P]),
    "mmpt_expand_rows_bf16": (I32, [I64, I64, P, P, I64, P, I64, P]),
    "mmpt_embed_fwd": (I32, [I64, I64, P, P, P, P, P, P]),
    "mmpt_embed_noise_fwd": (I32, [I64, I64, P, P, P, P, P, F32, U64, U64, P]),
    "mmpt_embed_noise": (I32, [I64, I64, F32, U64, U64, P, P]),
    "mmpt_embed_bwd": (I32, [I64, I64, I64, P, P, P, P, P, P, P, P]),
    "mmpt_embed_segments_workspace_bytes": (I64, [I64, I64]),
    "mmpt_embed_segments": (I32, [I64, P, I64, I64, P, P, P, P, P, P, I64, P]),
    "mmpt_embed_bwd_dev": (I32, [I64, I64, I64, P, P, P, P, P, P, P, P, P]),
    "mmpt_embed_bwd_split_workspace_bytes": (I64, [I64, I64]),
    "mmpt_embed_bwd_split": (I32, [I64, I64, I64, P, P, P, P, P, P, P, P, P, I64, P]),
    "mmpt_im2col_patches": (I32, [I64, I64, I64, I64, P, P, P]),
    "mmpt_im2col_patches_ex": (I32, [I64, I64, I64, I64, P, P, I64, P]),
    "mmpt_vit_embed_fwd": (I32, [I64, I64, I64, P, P, P, P, P]),
    "mmpt_vit_embed_bwd": (I32, [I64, I64, I64, P, P, P, P, P]),
    "mmpt_select_patches_fwd": (I32, [I64, I64, I64, P, P, P]),
    "mmpt_select_patches_bwd": (I32, [I64, I64, I64, P, P, I32, P]),
    "mmpt_l2norm_workspace_bytes": (I64, [I64]),
    "mmpt_sumsq_f32": (I32, [I64, P, P, P, P]),
    "mmpt_adam_step": (I32, [I64, P, P, P, P, P, F32, F32, F32, F32, F32, I32, I64, P, P]),
    "mmpt_adam_step_zero_grad": (I32, [I64, P, P, P, P, P, F32, F32, F32, F32, F32, I32, I64, P, I32, P]),
    "mmpt_clip_coef": (I32, [P, F32, P, P]),
    "mmpt_cast_f32_bf16": (I32, [I64, P, P, P]),
    "mmpt_transpose_bf16": (I32, [I64, I64, P, I64, P, I64, P]),
    "mmpt_transpose_bf16_batched": (I32, [I64, P, I64, P, P, P]),
    "mmpt_dropout_bf16": (I32, [I64, I64, P, I64, P, I64, F64, U64, U64, P]),
    "mmpt_dropout_f32": (I32, [I64, I64, P, P, F64, U64, U64, P]),
    "mmpt_dropout_add_f32": (I32, [I64, I64, P, I64, U64, P, I64, U64, P, P, F64, U64, P]),
    "mmpt_dropout_mask": (I32, [I64, F64, U64, U64, P, P]),
    "mmpt_attention_drop_fwd": (I32, [I64, I64, I64, I64, I64, I64, P, I64, I64, I64, I64, I32, F32, P, P, I64, P, F64, U64, U64, P]),
    "mmpt_attention_drop_bwd_workspace_bytes": (I64, [I64, I64, I64, I64, I32, F64]),
    "mmpt_attention_drop_bwd": (I32, [I64, I64, I64, I64, I64, I64, P, I64, I64, I64, I64, I32, F32, P, P, P, I64, P, P, P, F64, U64, U64, P]),
    "mmpt_attn_dropout_mask": (I32, [I64, I64, I64, I64, F64, U64, U64, P, P]),
    "mmpt_attn_dropout_p_eff": (F64, [F64]),
    "mmpt_cls_ln_fwd": (I32, [I64, I64, I64, F32, P, P, P, P, I64, P, P, P]),
    "mmpt_cls_ln_bwd_workspace_bytes": (I64, [I64, I64]),
    "mmpt_cls_ln_bwd": (I32, [I64, I64, I64, P, P, P, P, I64, P, P, P, P, P, P, P, P]),
    "mmpt_add_layernorm_fwd": (I32, [I64, I64, F32, P, P, I64, P, P, P, P, P, I64, P, P, F64, U64, U64, P]),
    "mmpt_add_layernorm_bwd_workspace_bytes": (I64, [I64, I64]),
    "mmpt_add_layernorm_bwd": (I32, [I64, I64, P, P, P, P, P, P, I64, P, P, I64, P, P, P, P, F64, U64, U64, P, P]),
    "mmpt_roberta_embed_fwd": (I32, [I64, I64, F32, P, P, P, I64, P, I64, P, P, P, P, P, P, P, F64, U64, U64, P]),
    "mmpt_roberta_embed_bwd_workspace_bytes": (I64, [I64, I64]),
    "mmpt_roberta_embed_bwd": (I32, [I64, I64, P, P, P, I64, P, I64, P, P, P, P, P, P, P, P, P, P, F64, U64, U64, P, P]),
    "mmpt_roberta_embed_noise_fwd": (I32, [I64, I64, F32, P, P, P, I64, P, I64, P, P, P, P, P, P, P, F64, U64, U64, F32, U64, U64, P]),
    "mmpt_roberta_embed_noise_bwd": (I32, [I64, I64, P, P, P, I64, P, I64, P, P, P, P, P, P, P, P, P, P, F64, U64, U64, F32, U64, U64, P, P]),
    "mmpt_mlm_ln_fwd": (I32, [I64, I64, F32, P, I64, P, P, P, I64, P, P, P]),
    "mmpt_mlm_ln_bwd_workspace_bytes": (I64, [I64, I64]),
    "mmpt_mlm_ln_bwd": (I32, [I64, I64, P, I64, P, P, P, P, I64, P, I64, P, I64, P, P, P, P, P]),
    "mmpt_dwconv7_fwd": (I32, [I64, I64, I64, I64, P, P, P, P, P]),
    "mmpt_dwconv7_bwd_input": (I32, [I64, I64, I64, I64, P, P, P, P, P]),
    "mmpt_dwconv7_bwd_weight_workspace_bytes": (I64, [I64, I64, I64, I64]),
    "mmpt_dwconv7_bwd_weight": (I32, [I64, I64, I64, I64, P, P, P, P, P, P]),
    "mmpt_dwconv7_idx_fwd": (I32, [I64, I64, I64, I64, I64, P, P, P, P, P, P]),
    "mmpt_dwconv7_idx_bwd_input": (I32, [I64, I64, I64, I64, I64, P, P, P, P, P, P]),
    "mmpt_dwconv7_idx_bwd_weight": (I32, [I64, I64, I64, I64, I64, P, P, P, P, P, P, P]),
    "mmpt_droppath_add_fwd": (I32, [I64, I64, I64, I64, P, P, P, I64, P, F64, P, P]),
    "mmpt_droppath_bwd_workspace_bytes": (I64, [I64, I64, I64]),
    "mmpt_droppath_bwd": (I32, [I64, I64, I64, I64, P, P, P, P, I64, F64, P, I64, P, P, P]),
    "mmpt_layerscale_add_fwd": (I32, [I64, I64, P, P, P, I64, P, P]),
    "mmpt_layerscale_bwd_workspace_bytes": (I64, [I64, I64]),
    "mmpt_layerscale_bwd": (I32, [I64, I64, P, P, P, I64, P, I64, P, P, P]),
    "mmpt_ln16_bwd_workspace_bytes": (I64, [I64, I64]),
    "mmpt_ln16_bwd": (I32, [I64, I64, P, I64, P, P, P, P, I64, P, I64, P, P, P, P]),
    "mmpt_avgpool_fwd": (I32, [I64, I64, I64, P, P, P]),
    "mmpt_avgpool_bwd": (I32, [I64, I64, I64, P, P, P]),
    "mmpt_patchify2_nhwc": (I32, [I64, I64, I64, I64, P, P, P]),
    "mmpt_unpatchify2_nhwc": (I32, [I64, I64, I64, I64, P, P, P]),
    "mmpt_causal_conv1d_fwd": (I32, [I64, I64, I64, I64, P, I64, P, P, P, I64, P]),
    "mmpt_causal_conv1d_bwd_workspace_bytes": (I64, [I64, I64, I64]),
    "mmpt_causal_conv1d_bwd": (I32, [I64, I64, I64, I64, P, I64, P, P, P, I64, P, I64, P, I64, P, P, P,
                                     P]),
    "mmpt_selective_scan_chunk": (I64, []),
    "mmpt_selective_scan_states_bytes": (I64, [I64, I64, I64, I64]),
    "mmpt_selective_scan_fwd_workspace_bytes": (I64, [I64, I64, I64, I64]),
    "mmpt_selective_scan_fwd": (I32, [I64, I64, I64, I64, P, I64, P, I64, P, P, P, P, I64, P, P, I64,
                                      P, I64, P, P, P]),
    "mmpt_selective_scan_bwd_workspace_bytes": (I64, [I64, I64, I64, I64]),
    "mmpt_selective_scan_bwd": (I32, [I64, I64, I64, I64, P, I64, P, I64, P, P, P, P, I64, P, P, I64,
                                      P, P, I64, P, I64, P, I64, P, I64, P, I64, P, P, I64, P, P, P,
                                      P, P]),
    # K22 varlen: packed rows, positions / chunk offsets from int32 device tables
    "mmpt_causal_conv1d_varlen_fwd": (I32, [I64, I64, I64, P, P, I64, P, P, P, I64, P]),
    "mmpt_causal_conv1d_varlen_bwd_workspace_bytes": (I64, [I64, I64]),
    "mmpt_causal_conv1d_varlen_bwd": (I32, [I64, I64, I64, P, P, I64, P, P, P, I64, P, I64, P, I64,
                                            P, P, P, P]),
    "mmpt_selective_scan_varlen_states_bytes": (I64, [I64, I64, I64]),
    "mmpt_selective_scan_varlen_fwd_workspace_bytes": (I64, [I64, I64, I64]),
    "mmpt_selective_scan_varlen_fwd": (I32, [I64, I64, I64, P, P, I64, I64, P, I64, P, I64, P, P, P,
                                             P, I64, P, P, I64, P, I64, P, P, P]),
    "mmpt_selective_scan_varlen_bwd_workspace_bytes": (I64, [I64, I64, I64, I64]),
    "mmpt_selective_scan_varlen_bwd": (I32, [I64, I64, I64, P, P, I64, I64, P, I64, P, I64, P, P, P,
                                             P, I64, P, P, I64, P, P, I64, P, I64, P, I64, P, I64,
                                             P, I64, P, P, I64, P, P, P, P, P]),
}


def load() -> ctypes.CDLL:
    """Load (once) and type the shared library; raise if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libmmpt.so not found at {LIB_PATH}: build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or make -C "
            "multimodal_llm_pretraining_amd/csrc). There is no CPU/PyTorch fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    ver = lib.mmpt_abi_version()
    if ver != ABI_VERSION:
        raise RuntimeError(f"libmmpt.so ABI {ver} != expected {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def exported_symbols() -> list[str]:
    return list(SIGNATURES)


def call(name: str, *args) -> int:
    """Invoke an entry point; raise RuntimeError on a non-zero status."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if SIGNATURES[name][0] is I32 and rc != 0:
        msg = lib.mmpt_last_error().decode(errors="replace")
        raise RuntimeError(f"{name} failed (status {rc}): {msg}")
    return rc


def set_switch(name: str, value: int) -> int:
    """mmpt_set_switch: override a kernel-variant switch (read once from the environment
    otherwise); returns the previous value."""
    rc = load().mmpt_set_switch(name.encode(), int(value))
    if rc < 0:
        raise RuntimeError("mmpt_set_switch: " + load().mmpt_last_error().decode(errors="replace"))
    return rc


def query(name: str, *args) -> int:
    """Invoke a size/info query (returns its value)."""
    return getattr(load(), name)(*args)
