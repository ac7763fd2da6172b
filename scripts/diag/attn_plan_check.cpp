// Sweep of the attention plan (multimodal_llm_pretraining_amd/csrc/attn_plan.h) on the host: for
// every head dim, dense and varlen, every rotary width / table alignment of the grid below and
// all 8 settings of the three switches, the plan the entries of attention.hip would execute must
//   - name the kernels of the head dim: 64 -> D/DR 64/64, 256 -> 256/256, 80 -> 128/80 (128/128
//     with MMPT_ATTN_NATIVE80=0), 96 / 112 / 128 -> 128/128,
//   - take a dS family only at head_dim 256, dense, with MMPT_ATTN_DS on (the pair kernel with
//     MMPT_ATTN_PAIR on, else the ring kernel),
//   - fuse the rope backward only into the pair family, at 64 rotary dims, with aligned tables,
//   - place the dS tiles 256-B aligned behind δ, and size the workspace by the closed form of
//     include/mmpt.h (δ only for a varlen call, whatever the switches),
//   - never let the bytes its family writes (δ, and the last dS tile's end) pass workspace_bytes,
//   - with dropout on (mmpt_attention_drop_*): the same D / DR, the ring dK/dV + recomputing dQ
//     family, no fused rope and a δ-only workspace, whatever the switches, dense or varlen; and
//     with it off exactly the plan of a call without the argument.
// Exits non-zero with the offending cases printed.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       scripts/diag/attn_plan_check.cpp -o attn_plan_check; ./attn_plan_check
#include <cstdio>
#include <initializer_list>

#include "../../multimodal_llm_pretraining_amd/csrc/attn_plan.h"

using namespace mmpt;

static long fails = 0, checked = 0;

struct Case {
  int64_t batch, seq, heads, head_dim, rot;
  bool varlen, aligned;
  AttnSwitches sw;
};

static void report(const char* what, const Case& c) {
  if (fails++ >= 20) return;
  std::printf("FAIL %s: batch %lld seq %lld heads %lld head_dim %lld varlen %d rot %lld aligned %d "
              "DS %d PAIR %d NATIVE80 %d\n",
              what, (long long)c.batch, (long long)c.seq, (long long)c.heads, (long long)c.head_dim,
              (int)c.varlen, (long long)c.rot, (int)c.aligned, c.sw.ds, c.sw.pair, c.sw.native80);
}
#define CHECK(cond) \
  do {              \
    if (!(cond)) report(#cond, c); \
  } while (0)

static void check_plan(const Case& c) {
  const AttnPlan pl = attn_plan(c.batch, c.seq, c.heads, c.head_dim, c.varlen, c.rot, c.aligned, c.sw);
  ++checked;
  const int d = (int)c.head_dim;
  CHECK(pl.D == (d == 64 ? 64 : d == 256 ? 256 : 128));
  CHECK(pl.DR == (d == 80 && c.sw.native80 ? 80 : pl.D));

  const bool ds = d == 256 && !c.varlen && c.sw.ds;
  CHECK((pl.family != RING_RECOMPUTE) == ds);
  if (ds) CHECK(pl.family == (c.sw.pair ? PAIR_DS : RING_DS));
  CHECK(pl.fused_rope == (pl.family == PAIR_DS && c.rot == 64 && c.aligned));

  // the workspace: δ = fp32 per query row at 0; dS tiles of 32 x 32 bf16 = 2 KiB,
  // ceil(seq/32)^2 per (batch, head), 256-B aligned behind it
  const int64_t delta = c.batch * c.seq * c.heads * 4;
  const int64_t nq = (c.seq + 31) / 32, tiles = c.batch * c.heads * nq * nq;
  CHECK(pl.delta_bytes == delta);
  int64_t written = delta;  // the δ kernel writes every row
  if (ds) {
    CHECK(pl.ds_offset % 256 == 0 && pl.ds_offset >= pl.delta_bytes && pl.ds_offset < delta + 256);
    CHECK(pl.ds_offset == ds_offset(c.batch, c.seq, c.heads));
    CHECK(pl.workspace_bytes == (delta + 255) / 256 * 256 + tiles * 2048);
    // ds_tile: tile (batch·heads - 1, nq - 1, nq - 1) is the last one the dK/dV kernel writes
    written = pl.ds_offset + ((((c.batch * c.heads - 1) * nq + nq - 1) * nq + nq - 1) + 1) * 2048;
  } else {
    CHECK(pl.ds_offset == 0);
    CHECK(pl.workspace_bytes == delta);
  }
  if (c.varlen) CHECK(pl.workspace_bytes == delta && pl.family == RING_RECOMPUTE && !pl.fused_rope);
  CHECK(written <= pl.workspace_bytes);
  CHECK(!pl.dropout);

  const AttnPlan off = attn_plan(c.batch, c.seq, c.heads, c.head_dim, c.varlen, c.rot, c.aligned, c.sw,
                                 false);
  CHECK(off.D == pl.D && off.DR == pl.DR && off.family == pl.family &&
        off.fused_rope == pl.fused_rope && off.delta_bytes == pl.delta_bytes &&
        off.ds_offset == pl.ds_offset && off.workspace_bytes == pl.workspace_bytes && !off.dropout);
  const AttnPlan dr = attn_plan(c.batch, c.seq, c.heads, c.head_dim, c.varlen, c.rot, c.aligned, c.sw,
                                true);
  ++checked;
  CHECK(dr.dropout);
  CHECK(dr.D == pl.D && dr.DR == pl.DR);
  CHECK(dr.family == RING_RECOMPUTE && !dr.fused_rope);
  CHECK(dr.delta_bytes == delta && dr.ds_offset == 0 && dr.workspace_bytes == delta);
}

int main() {
  const int64_t problems[][3] = {  // batch, seq, heads
      {1, 1, 1},  {1, 31, 1},  {2, 32, 3},    {3, 33, 5},    {2, 707, 8},
      {1, 64, 7}, {5, 127, 2}, {8, 2048, 16}, {1, 8192, 32}, {16, 4096, 40}};
  for (const auto& pr : problems)
    for (int64_t head_dim : {64, 80, 96, 112, 128, 256})
      for (bool varlen : {false, true})
        for (int64_t rot : {0, 32, 64, 256})
          for (bool aligned : {false, true})
            for (int bits = 0; bits < 8; ++bits) {
              Case c{pr[0], pr[1], pr[2], head_dim, rot, varlen, aligned, AttnSwitches{}};
              c.sw.ds = bits & 1, c.sw.pair = (bits >> 1) & 1, c.sw.native80 = (bits >> 2) & 1;
              check_plan(c);
            }
  {  // the defaults are the library's with nothing set
    const AttnSwitches sw;
    Case c{1, 1, 1, 64, 0, false, false, sw};
    CHECK(sw.ds == 1 && sw.pair == 1 && sw.native80 == 1);
  }
  std::printf(fails ? "attention plan: %ld plans, %ld FAILURES\n" : "attention plan: %ld plans ok\n",
              checked, fails);
  return fails ? 1 : 0;
}
