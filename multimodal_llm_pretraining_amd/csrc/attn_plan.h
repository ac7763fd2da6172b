// The attention plan: the one place that decides which kernels an attention call runs — the
// kernel head dim D and the dims DR it computes, the backward family, whether the rope backward
// is fused into its epilogues, and the workspace layout.  The entries of attention.hip execute an
// AttnPlan; the workspace queries of include/mmpt.h return its workspace_bytes, so the size a
// caller allocates and the bytes the launch writes come from the same arithmetic.
//
// Host-only integer arithmetic: nothing from HIP, compiles with plain g++ -std=c++17
// (scripts/diag/attn_plan_check.cpp sweeps its invariants under the host sanitizers).
// Everything sits in an unnamed namespace: each including file gets its own copy and the library
// exports none of it.
#pragma once
#include <stdint.h>

namespace mmpt {
namespace {

constexpr int FUSED_ROT = 64;  // the rotary width the fused epilogues handle (Pythia: D / 4)
// dS tiles (ds_tile): 32 queries x 32 keys of bf16, ceil(S/32)^2 of them per (batch, head)
constexpr int64_t DS_TILE_ROWS = 32, DS_TILE_BYTES = 2048;

// The MMPT_ATTN_DS / MMPT_ATTN_PAIR / MMPT_ATTN_NATIVE80 environment switches (attention.hip
// reads them once; mmpt_set_switch overrides them).  The defaults are the values with nothing set.
struct AttnSwitches {
  int ds = 1;        // 0: D = 256 backward on the recomputing dQ kernel, no dS tiles
  int pair = 1;      // 0: D = 256 dK/dV on the one-wave-per-SIMD ring kernel
  int native80 = 1;  // 0: head_dim 80 computes all 128 dims of the D = 128 kernels
};

enum AttnBwdFamily {
  RING_RECOMPUTE,  // ring dK/dV + the dQ kernel that recomputes P (every head dim, every varlen call)
  RING_DS,         // ring dK/dV writing dS tiles + attn_bwd_dq_ds_kernel
  PAIR_DS,         // D-split wave-pair dK/dV writing dS tiles + attn_bwd_dq_ds_kernel
};

struct AttnPlan {
  int D, DR;  // the kernels' head dim and the dims they compute (DR < D: 80 on the D = 128 kernels)
  AttnBwdFamily family;
  bool fused_rope;  // the dK / dQ epilogues apply the inverse rotation (mmpt_attention_bwd_rope)
  // backward workspace: δ (fp32 per query row) at 0, then for the dS families the tiles at
  // ds_offset (256-B aligned; 0 when there are none)
  int64_t delta_bytes, ds_offset, workspace_bytes;
  bool dropout;  // the DROP variants of the forward, ring dK/dV and recomputing dQ kernels
};

int64_t ds_offset(int64_t batch, int64_t seq, int64_t heads) {  // after δ, 256-B aligned
  return (batch * seq * heads * (int64_t)sizeof(float) + 255) & ~(int64_t)255;
}

// seq: max_seq for a varlen call (the stride of δ).  rot_dims / tables_aligned: the rotary width
// and 16-B alignment of both tables of an mmpt_attention_bwd_rope call, 0 / false elsewhere.
// dropout: an mmpt_attention_drop_* call with a non-zero threshold — the ring dK/dV + recomputing
// dQ pair at every head dim, dense or varlen (the dS families have no dropout), no fused rope.
AttnPlan attn_plan(int64_t batch, int64_t seq, int64_t heads, int64_t head_dim, bool varlen,
                   int64_t rot_dims, bool tables_aligned, const AttnSwitches& sw,
                   bool dropout = false) {
  AttnPlan pl{};
  pl.D = head_dim == 64 ? 64 : head_dim == 256 ? 256 : 128;  // 80, 96, 112: the D = 128 kernels
  pl.DR = head_dim == 80 && sw.native80 ? 80 : pl.D;         // (96, 112: padded to 128)
  // (varlen runs the ring dK/dV + recomputing dQ pair at every head dim: the dS tiles and the
  // wave-pair kernel index by the dense geometry)
  const bool ds = head_dim == 256 && !varlen && sw.ds && !dropout;
  pl.dropout = dropout;
  pl.family = !ds ? RING_RECOMPUTE : sw.pair ? PAIR_DS : RING_DS;
  pl.fused_rope = pl.family == PAIR_DS && rot_dims == FUSED_ROT && tables_aligned;
  pl.delta_bytes = batch * seq * heads * (int64_t)sizeof(float);
  pl.workspace_bytes = pl.delta_bytes;
  if (ds) {
    const int64_t nq = (seq + DS_TILE_ROWS - 1) / DS_TILE_ROWS;
    pl.ds_offset = ds_offset(batch, seq, heads);
    pl.workspace_bytes = pl.ds_offset + batch * heads * nq * nq * DS_TILE_BYTES;
  }
  return pl;
}

}  // namespace
}  // namespace mmpt
