// The GEMM launch schedule: the one place that decides how mmpt_gemm_bf16 runs a problem — the
// tile size, the K splits, the forward and weight-gradient tail splits, the K-tail kernel, the C2
// partial rows and the slab bytes.  mmpt_gemm_bf16 (gemm.hip) executes a GemmSchedule; the
// shape-only queries of include/mmpt.h are the schedule of the "assumed" problem (16-B aligned
// operands, all the workspace it wants).
//
// Host-only integer arithmetic: nothing from HIP, compiles with plain g++ -std=c++17
// (scripts/diag/gemm_plan_check.cpp sweeps its invariants under the host sanitizers).
// Everything sits in an unnamed namespace: each including file gets its own copy and the library
// exports none of it.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/mmpt.h"

// build-time kernel variants (A/B builds only) the schedule has to know about
#ifndef MMPT_GEMM_LUT
#define MMPT_GEMM_LUT 1  // 0: the big-tile kernel evaluates erfc per element, no LDS tables
#endif
#ifndef MMPT_GEMM_4P_FAST
#define MMPT_GEMM_4P_FAST 1  // 0: gemm4p without the fast whole-tile epilogue
#endif

namespace mmpt {
namespace {

constexpr int BK = 64;
// Internal epilogues: split-K fp32 slabs (EPI_SPLIT), and (round 5) the split-K form of
// F32_ACC_COLSUM (EPI_SPLIT_CS: slabs + per-split row sums of op(A), see csa()).
constexpr int EPI_SPLIT = 100, EPI_SPLIT_CS = 102;

// Every input of the decision that is not the problem itself: the MMPT_GEMM_* environment
// switches (gemm.hip reads them once; mmpt_set_switch overrides krev / tail / wtail / tail128)
// and the device.  The defaults are the values with nothing set.
struct GemmSwitches {
  // MMPT_GEMM_4P: big-tile kernel switch, 1 (default, see uses_4p), 0 = gemm128 for every
  // problem (A/B only; the 8-wave gemm256 kernel of rounds 1-3, this switch's 0 arm until
  // round 5, is retired)
  int g4 = 1;
  bool tile128 = false;  // MMPT_GEMM_TILE=128: every GEMM on the 128x128 kernel (A/B only)
  int splits = 0;  // MMPT_GEMM_SPLITS=s (1..16): weight gradients on 256^2 tiles in s K-splits (A/B)
  // MMPT_GEMM_BIG_MIN=t.  Non-split problems run 256^2 tiles from 128 of them on (half the CUs,
  // one wave): at 150-225 tiles gemm4p beats the two 128^2 waves (ViT qkv 6304x2304x768 25.5 vs
  // 36.9 us, fc2 12608x768x3072 73.7 vs 107.7 us), at 75 it loses (19.2 -> 21.5 us); per-rank
  // 32 / 64 steps +0.2% / +0.45% (profiles/r06/bigmin/).
  int64_t big_min = 128;
  int tail = 1;     // MMPT_GEMM_TAIL=0: no forward tail split
  int tail128 = 1;  // MMPT_GEMM_TAIL128=0: tails of <= 128 rows on gemm4p too (A/B only)
  int wtail = 1;    // MMPT_GEMM_WTAIL=0: no weight-gradient tail split; 2: tail tile columns only
  int group = 0;    // MMPT_GEMM_GROUP=<rows> (1..64), 0 = automatic
  int krev = 2;     // MMPT_GEMM_KREV=0/1, 2 = automatic
  int persist = 1;  // MMPT_GEMM_PERSIST=0: one workgroup per tile
  int cus = 256;    // the device's CU count rounded down to a multiple of 8; 256 when unknown
};

struct GemmProblem {
  int la, lb;   // mmpt_layout of A / B
  int epi;      // the caller's epilogue (quick-GELU forms and F32_ACC_COLSUM as given)
  int64_t M, N, K;
  bool aligned;      // every epilogue operand 16-B aligned, rows included (8-column epilogue)
  int64_t ws_bytes;  // workspace given (0: none)
  bool ws_aligned;   // the workspace pointer is 16-B aligned
};

enum GemmFamily { G4, G4_KT, G128 };  // gemm4p_kernel / gemm4p_kt_kernel (K % 64 != 0) / gemm128_kernel
enum GemmFinish { FIN_NONE, FIN_SPLITK_REDUCE, FIN_TAIL_EPI };  // (tail_epi_kernel: forward tail)

const char* gemm_family_name(GemmFamily f) {
  return f == G4 ? "gemm4p_kernel" : f == G4_KT ? "gemm4p_kt_kernel" : "gemm128_kernel";
}

// one GEMM kernel launch over the output rectangle [row0, row0 + rows) x [col0, col0 + cols)
struct GemmLaunch {
  GemmFamily family;
  int epi;  // the launch epilogue (EPI_SPLIT / EPI_SPLIT_CS: into the slabs)
  int64_t row0, col0, rows, cols;
  int splits, kchunk;  // K range of split s: [s * kchunk, min(K, (s + 1) * kchunk))
  int tile;            // 256 (gemm4p) / 128
  int tiles_m, tiles_n;
  int workgroups;  // gemm4p: the persistent grid; gemm128: tiles (x splits in grid.y)
  int group, krev;
};

struct GemmSchedule {
  int n = 0;             // GEMM launches: the main one, then the split tail (if any)
  GemmLaunch launch[2];
  GemmFinish finish = FIN_NONE;  // runs over the last launch's rectangle and splits
  int probe_after = 0;   // the probe event follows this launch (the main one before a forward tail)
  int tile = 0, splits = 0;  // the plan (mmpt_gemm_plan): the whole problem's tile and K splits
  bool wide = false;         // GemmParams::wide
  int64_t slab_bytes = 0;       // workspace the launches use
  int64_t workspace_bytes = 0;  // workspace the problem wants (with less, parts of the plan go)
  // C2 partial rows of the column-sum forms (DGELU_COLSUM / DQGELU_COLSUM and F32_ACC_COLSUM; 0
  // for the other epilogues, and for an F32_ACC_COLSUM problem the big-tile kernel does not
  // take): the rows the launches touch, and how many of them they write in full (the caller
  // zeroes the rest of what the rows query promised)
  int64_t c2_rows = 0, c2_rows_written = 0;
  int64_t tail_rows = 0;  // matrix rows of the forward tail split (mmpt_gemm_last_tail_rows)
};

// The persistent walk (round 5).  At any time an XCD's 32 CUs hold 32 consecutive work ids:
// GROUP tile rows x 32/GROUP tile columns, whose A / B K-slices they share through the XCD's
// L2; over the launch, A is fetched from beyond L2 once per column block and B once per row
// block.  A (the activations, up to GBs) streams from HBM; B (a weight, <= 200 MB) mostly
// stays in the Infinity Cache.  Measured at T = 180,992 (profiles/r05/walk/): N <= 2048
// (8 tile columns: the dX GEMMs, the N = 2048 forwards, the weight gradients) run best with
// GROUP = 2 (the block spans every column, A is read once) — +6..8% over round 4's GROUP = 8;
// wider N with GROUP = 4 (+0.5..1.5%).  KREV: a workgroup's odd tiles walk K last-to-first,
// so the A K-slices the previous tile round left in L2 are read first (qkv forward: -16%
// L2->fabric bytes), measured +0..0.8% on the wide-N shapes and -2..4% on lm_head dX; NOT the
// default: it changes each odd tile's fp32 summation order, hence the step's rounding (the C5
// ZeRO-3 + offload gradient norm moved by 2.4 sigma of its bf16 noise, past its parity bar),
// while GROUP only changes which CU computes a tile — bitwise the round-4 results.
// Overrides (A/B): MMPT_GEMM_GROUP=<rows>, MMPT_GEMM_KREV=0/1.
int walk_group(int tiles_n, const GemmSwitches& sw) {
  return sw.group > 0 ? sw.group : (tiles_n <= 8 ? 2 : 4);
}
int walk_krev(const GemmSwitches& sw) { return sw.krev < 2 ? sw.krev : 0; }

// the forms gemm4p runs by default whatever the fast path: plain, residual, the fp32 ones and,
// since round 5, the dQGELU (CLIP) and dSwiGLU (Llama) backward forms (general epilogue)
constexpr bool epi_4p_default(int e) {
  return e == MMPT_EPI_BF16 || e == MMPT_EPI_F32_RESID || e == MMPT_EPI_F32_ACC ||
         e == MMPT_EPI_F32_STORE || e == MMPT_EPI_BF16_DQGELU ||
         e == MMPT_EPI_BF16_DQGELU_COLSUM || e == MMPT_EPI_BF16_DSWIGLU;
}
// gemm4p runs a big-tile problem when the operands are both K-contiguous or both
// row-contiguous (the weight-gradient form, split-K included) and K is a whole number of
// K-tiles (every split too: kchunk is a multiple of 64).  epi = the launch epilogue
// (quick-GELU forms included, EPI_SPLIT for split-K slabs).  Default (1): every epilogue with
// the fast whole-tile path (plain, erf-GELU, erf-dGELU (+ column sums), and since round 5 the
// quick-GELU and SwiGLU forwards from their tables) and the general-path ones above (fp32
// residual / accumulate / store, split-K slabs, dQGELU, dSwiGLU): +5..10% over round 4's
// 8-wave kernel at the model shapes (profiles/r04/gemm4p_ab/fast_epilogue_T180992.txt,
// profiles/r05/act4p/).  Everything else runs gemm128.
// The epilogues with the fast whole-tile path (epilogue4f) need 16-B aligned outputs and
// operands (`aligned` = GemmParams::wide) and N % 8 == 0.
constexpr bool epi_4p_fast(int e) {
  return MMPT_GEMM_4P_FAST && (e == MMPT_EPI_BF16 || e == MMPT_EPI_F32_RESID ||
                               (MMPT_GEMM_LUT && (e == MMPT_EPI_BF16_GELU || e == MMPT_EPI_BF16_DGELU ||
                                                  e == MMPT_EPI_BF16_DGELU_COLSUM ||
                                                  e == MMPT_EPI_BF16_QGELU ||
                                                  e == MMPT_EPI_BF16_SWIGLU ||
                                                  e == MMPT_EPI_BF16_DSWIGLU)));
}
// the forms with a K-tail (KT) instantiation: weight gradients (K_ROWS x K_ROWS, fp32 accumulate /
// store / split-K slabs) and the plain forward (the CLIP patch embedding, K = 3 x 14 x 14)
constexpr bool kt_form(int la, int epi) {
  return la == MMPT_K_ROWS ? (epi == MMPT_EPI_F32_ACC || epi == MMPT_EPI_F32_STORE || epi == EPI_SPLIT ||
                              epi == MMPT_EPI_F32_ACC_COLSUM || epi == EPI_SPLIT_CS)
                           : epi == MMPT_EPI_BF16;
}
bool uses_4p(bool big, int la, int lb, int epi, int64_t N, int64_t K, bool aligned,
             const GemmSwitches& sw) {
  if (epi == MMPT_EPI_F32_ACC_COLSUM || epi == EPI_SPLIT_CS)  // (K-tail form since round 6)
    return sw.g4 != 0 && big && la == MMPT_K_ROWS && lb == MMPT_K_ROWS;
  if (!big || la != lb || (K % BK != 0 && !kt_form(la, epi))) return false;
  if (epi_4p_fast(epi) && !(aligned && N % 8 == 0)) return false;
  if (epi == MMPT_EPI_BF16_SWIGLU && !epi_4p_fast(epi)) return false;  // no general-path form
  if ((epi == MMPT_EPI_BF16_SWIGLU || epi == MMPT_EPI_BF16_DSWIGLU) && la != MMPT_ROWS_K)
    return false;  // built for the model's K-contiguous operands only
  return sw.g4 != 0 && (epi_4p_default(epi) || epi_4p_fast(epi) || epi == EPI_SPLIT);
}

struct Plan {
  bool big;   // 256x256 tile
  int splits;
  int kchunk;
};
// kchunk = ceil(K / splits) rounded up to whole K-tiles, and the splits that leaves
void set_splits(int64_t K, int64_t sp, int* splits, int* kchunk) {
  const int64_t kc = ((K + sp - 1) / sp + BK - 1) / BK * BK;
  *splits = (int)((K + kc - 1) / kc);
  *kchunk = (int)kc;
}

Plan plan(int64_t M, int64_t N, int64_t K, int epi, const GemmSwitches& sw) {
  Plan pl{};
  const int64_t t256 = ((M + 255) / 256) * ((N + 255) / 256);
  const int64_t t128 = ((M + 127) / 128) * ((N + 127) / 128);
  pl.big = t256 >= sw.big_min || epi == MMPT_EPI_BF16_SWIGLU;  // SWIGLU pairs 128-col quadrants
  if (sw.tile128 && epi != MMPT_EPI_BF16_SWIGLU) pl.big = false;  // A/B only
  pl.splits = 1;
  pl.kchunk = (int)K;
  const bool splittable = epi == MMPT_EPI_F32_ACC || epi == MMPT_EPI_F32_STORE ||
                          epi == MMPT_EPI_F32_ACC_COLSUM;  // (the same plan as F32_ACC)
  if (splittable) {
    // weight gradients: K = tokens. Pick (tile, splits) minimising the padded wave
    // count ceil(blocks / slots) / blocks-work, slots = the CUs (256^2, 1 per CU) or twice
    // that (128^2, 2 per CU); keep >= 1024 k per split and <= 16 splits (<= 2 from 512 tiles).
    // Model: a CU fully busy with one 256^2 block retires 4 128^2-tile units in 4 time
    // units; with two 128^2 blocks it retires 2 units in 2.67 (128^2 runs at ~0.75x the
    // 256^2 rate).  Slab write+read adds sp*8 B per output element vs 2K flops per
    // element: factor (1 + sp*800/K) at ~5 TB/s : ~1 PF/s.
    double best = 1e30;
    for (int big = 1; big >= 0; --big) {
      const int64_t tiles = big ? t256 : t128;
      const int64_t slots = big ? sw.cus : 2 * sw.cus;
      const double wave_cost = big ? 4.0 : 2.67;
      // (many tiles: up to 4 splits, which evens out the last wave — lm_head's weight
      // gradient, 1576 tiles = 6.2 rounds of 256, runs 25 rounds of a quarter of the K:
      // 1108 / 1141 / 1149 / 1165 TF/s at 1 / 2 / 3 / 4 splits, profiles/r04/d80/)
      const int64_t max_sp = tiles < 2 * slots ? 16 : 4;
      for (int64_t sp = 1; sp <= max_sp && (sp == 1 || K / sp >= 1024); ++sp) {
        const int64_t blocks = tiles * sp;
        const double waves = (double)((blocks + slots - 1) / slots);
        const double cost = waves * wave_cost / (double)sp *
                            (sp > 1 ? 1.0 + (double)sp * 800.0 / (double)K : 1.0);
        if (cost < best - 1e-9) {
          best = cost;
          pl.big = big;
          pl.splits = (int)sp;
        }
      }
    }
    if (sw.splits > 0) {
      pl.big = true;
      pl.splits = sw.splits;
    }
    if (pl.splits > 1) set_splits(K, pl.splits, &pl.splits, &pl.kchunk);
  }
  return pl;
}

// Tail split (round 5).  A persistent launch runs ceil(tiles / 256) rounds; the N = 2048 GEMMs
// of the step have 707 x 8 = 5656 tiles = 22 rounds + 24 tiles, so one CU in ten works through a
// 23rd tile (up to ~0.2 ms at K = 8192) while the rest wait.  Instead the bottom `rows` tile rows
// — the fewest that leave a whole number of rounds above them — run as a split-K GEMM over
// ~all CUs (fp32 slabs in the caller's workspace) and tail_epi_kernel applies the epilogue.
// Only for the fast plain / residual epilogues on gemm4p shapes with K >= 2048; the tail rows'
// fp32 sums run in split order (the other rows are bitwise unchanged).  MMPT_GEMM_TAIL=0: off.
struct TailPlan {
  int rows = 0;    // tail tile rows (0: no tail split)
  int splits = 0;  // K splits of the tail
  int kchunk = 0;
  int64_t mt = 0;      // matrix rows in the tail
  bool small = false;  // <= 128 rows: on 128-row tiles (gemm128)
};
TailPlan tail_plan(const GemmProblem& p, const Plan& pl, const GemmSwitches& sw) {
  TailPlan t;
  const int64_t M = p.M, N = p.N, K = p.K;
  if (!sw.tail || p.la != MMPT_ROWS_K || p.lb != MMPT_ROWS_K) return t;
  if (p.epi != MMPT_EPI_BF16 && p.epi != MMPT_EPI_F32_RESID) return t;
  if (K % BK != 0 || K < 2048 || N % 8 != 0) return t;
  if (!pl.big || pl.splits != 1) return t;
  const int64_t slots = sw.persist ? sw.cus : 0;  // (a persistent launch only)
  if (slots <= 0) return t;
  const int64_t tm = (M + 255) / 256, tn = (N + 255) / 256;
  int64_t g = slots, b = tn;  // q = slots / gcd(tn, slots) tile rows make whole rounds
  while (b) {
    const int64_t r = g % b;
    g = b;
    b = r;
  }
  const int64_t q = slots / g;
  const int64_t rt = tm % q;
  if (rt == 0 || tm - rt < q) return t;
  // a tail of <= 128 rows (T = 16 * 2049 = 32,784: 16 rows) runs on 128-row tiles (gemm128: a
  // 256-row tile would run 16x the MFMAs its rows need; MMPT_GEMM_TAIL128=0: gemm4p, A/B only)
  // in up to 16 splits of >= 2 K-tiles: its few rows make the slabs small (16 x 16 x 2048 fp32
  // = 2 MiB at C2's shape)
  const int64_t mt = M - (tm - rt) * 256;
  const bool small = mt <= 128 && sw.tail128 == 1;
  const int64_t tail_tiles = small ? (N + 127) / 128 : rt * tn;
  int64_t sp = slots / tail_tiles;
  sp = std::min<int64_t>(sp, 16);
  sp = std::min<int64_t>(sp, K / BK / (small ? 2 : 8));  // >= 8 (2) K-tiles per split
  if (sp < 2) return t;
  const int64_t kc = (K / sp + BK - 1) / BK * BK;
  t.rows = (int)rt;
  t.splits = (int)((K + kc - 1) / kc);
  t.kchunk = (int)kc;
  t.mt = mt;
  t.small = small;
  return t;
}

// Weight-gradient tail split (round 6).  The planner splits a weight-gradient GEMM's K over all
// of its tiles when they make a partial round (C5's fc1 dW: 400 tiles = 1.56 rounds, 5 splits),
// so every tile pays the fp32 slab write + reduce — measured ~4% of the GEMM per split at K =
// 69,568 (scripts/diag/p28_dw_splits.sh), 3x the planner's slab term.  Instead the whole rounds'
// tile rows (or columns) run unsplit, straight into C, and only the rest is split: fc1 dW 1.91
// -> ~1.69 full-K rounds.  F32_ACC / F32_STORE / F32_ACC_COLSUM on 256^2 tiles (the fused row
// sums: a row tail's rows get one partial row per split there, the unsplit rows one; a column
// tail leaves the sums to the unsplit columns, which cover all of K).  The main part's fp32
// sums run in one pass, the tail's in split order (as before).
// MMPT_GEMM_WTAIL=0: off; 2: tail tile columns only (tests).
struct WTail {
  int dim = 0;     // 0: none, 1: tail tile rows (M), 2: tail tile columns (N)
  int lines = 0;   // whole tile rows / columns of the unsplit part
  int splits = 0;
  int kchunk = 0;
};
constexpr double SLAB_K = 2000.0;  // measured slab cost per split, in K units (p28 dW sweep)
WTail wtail_plan(const GemmProblem& p, const Plan& pl, const GemmSwitches& sw) {
  WTail w;
  const int64_t K = p.K;
  if (!sw.wtail || (p.epi != MMPT_EPI_F32_ACC && p.epi != MMPT_EPI_F32_STORE &&
                    p.epi != MMPT_EPI_F32_ACC_COLSUM))
    return w;
  if (!pl.big || pl.splits < 2 || sw.splits > 0) return w;
  const int64_t slots = sw.cus, tm = (p.M + 255) / 256, tn = (p.N + 255) / 256, tiles = tm * tn;
  const int64_t rounds = tiles / slots;
  if (rounds < 1) return w;
  auto split_cost = [&](int64_t t, int64_t sp) {
    return (double)((t * sp + slots - 1) / slots) / (double)sp * (1.0 + (double)sp * SLAB_K / (double)K);
  };
  double best = split_cost(tiles, pl.splits) * 0.97;  // the planner's split, 3% margin
  for (int dim = sw.wtail == 2 ? 2 : 1; dim <= 2; ++dim) {
    const int64_t nl = dim == 1 ? tm : tn, other = dim == 1 ? tn : tm;
    const int64_t lines = rounds * slots / other;
    if (lines < 1 || lines >= nl) continue;
    const int64_t tt = (nl - lines) * other;
    for (int64_t sp = 2; sp <= 16 && K / sp >= 1024; ++sp) {
      const double c = (double)((lines * other + slots - 1) / slots) + split_cost(tt, sp);
      if (c < best - 1e-9) {
        best = c;
        w.dim = dim;
        w.lines = (int)lines;
        w.splits = (int)sp;
      }
    }
  }
  if (w.dim != 0) set_splits(K, w.splits, &w.splits, &w.kchunk);
  return w;
}

// one launch of p's rectangle [row0, row0 + rows) x [col0, col0 + cols): gemm4p for the big
// problems it takes (uses_4p), gemm128 for everything else (small problems, mixed layouts,
// unaligned operands, K tails outside kt_form, and `small`, the <= 128-row forward tail)
GemmLaunch launch_of(const GemmProblem& p, const GemmSwitches& sw, bool big, bool wide, int epi,
                     int64_t row0, int64_t col0, int64_t rows, int64_t cols, int splits, int kchunk,
                     bool small = false) {
  GemmLaunch l{};
  const bool g4 = !small && uses_4p(big, p.la, p.lb, epi, cols, p.K, wide, sw);
  l.family = !g4 ? G128 : p.K % BK != 0 ? G4_KT : G4;
  l.epi = epi;
  l.row0 = row0, l.col0 = col0, l.rows = rows, l.cols = cols;
  l.splits = splits, l.kchunk = kchunk;
  l.tile = g4 ? 256 : 128;
  l.tiles_m = (int)((rows + l.tile - 1) / l.tile);
  l.tiles_n = (int)((cols + l.tile - 1) / l.tile);
  if (g4) {  // persistent: one workgroup per CU walks its XCD's run of tiles
    const int nwg = l.tiles_m * l.tiles_n * splits, slots = sw.persist ? sw.cus : 0;
    l.workgroups = slots > 0 && nwg > slots ? slots : nwg;
    l.group = walk_group(l.tiles_n, sw);  // the walk measured for gemm4p
    // (never with the fused row sums: their K-tile shares are split by loop index, so the
    // columns of one tile row must walk K in the same direction)
    const bool cs = epi == MMPT_EPI_F32_ACC_COLSUM || epi == EPI_SPLIT_CS;
    l.krev = p.K % BK == 0 && !cs ? walk_krev(sw) : 0;
  } else {  // gemm128: one workgroup per tile, round 4's GROUP = 8, forward K order
    l.workgroups = l.tiles_m * l.tiles_n;
    l.group = sw.group > 0 ? sw.group : 8;
    l.krev = 0;
  }
  return l;
}

GemmSchedule gemm_schedule(const GemmProblem& p, const GemmSwitches& sw) {
  GemmSchedule s;
  const int64_t M = p.M, N = p.N, K = p.K, f32 = (int64_t)sizeof(float);
  const bool acc_cs = p.epi == MMPT_EPI_F32_ACC_COLSUM;
  Plan pl = plan(M, N, K, p.epi, sw);
  WTail wt = wtail_plan(p, pl, sw);
  auto wtail_bytes = [&] {  // (no more than the full split's)
    const int64_t l0 = (int64_t)wt.lines * 256;
    return wt.dim == 0 ? 0 : (int64_t)wt.splits * (wt.dim == 1 ? M - l0 : M) * (wt.dim == 2 ? N - l0 : N) * f32;
  };
  if (pl.splits > 1) {
    const int64_t split_bytes = (int64_t)pl.splits * M * N * f32;
    s.workspace_bytes = std::max(split_bytes, wtail_bytes());
    if (p.ws_bytes < split_bytes) {  // no workspace: single pass (same numerics, less parallelism)
      pl.splits = 1;
      pl.kchunk = (int)K;
      wt = WTail{};
    }
  }
  s.tile = pl.big ? 256 : 128;
  s.splits = pl.splits;
  s.wide = p.aligned && (pl.splits == 1 || (N % 8 == 0 && p.ws_aligned));
  const TailPlan tp = tail_plan(p, pl, sw);
  if (tp.rows > 0) s.workspace_bytes = (int64_t)tp.splits * tp.mt * N * f32;

  if (tp.rows > 0 && s.wide && p.ws_aligned && p.ws_bytes >= s.workspace_bytes &&
      uses_4p(true, p.la, p.lb, p.epi, N, K, true, sw)) {
    // rows [0, M - mt): whole rounds; rows [M - mt, M): split-K slabs + tail_epi_kernel
    s.launch[0] = launch_of(p, sw, pl.big, s.wide, p.epi, 0, 0, M - tp.mt, N, 1, (int)K);
    s.launch[1] = launch_of(p, sw, pl.big, s.wide, EPI_SPLIT, M - tp.mt, 0, tp.mt, N, tp.splits,
                            tp.kchunk, tp.small);
    s.n = 2;
    s.finish = FIN_TAIL_EPI;
    s.probe_after = 0;  // bench.py: end of the main kernel (the tail is probed apart)
    s.tail_rows = tp.mt;
    s.slab_bytes = s.workspace_bytes;
  } else if (wt.dim != 0 && s.wide && p.ws_aligned && p.ws_bytes >= wtail_bytes()) {
    // whole rounds unsplit into C, the rest split-K through slabs + splitk_reduce
    const int64_t l0 = (int64_t)wt.lines * 256;
    const bool by_rows = wt.dim == 1;
    s.launch[0] = launch_of(p, sw, pl.big, s.wide, p.epi, 0, 0, by_rows ? l0 : M, by_rows ? N : l0,
                            1, (int)K);
    // (the tail rows' partial sums, one row per split; a column tail has none)
    s.launch[1] = launch_of(p, sw, pl.big, s.wide, acc_cs && by_rows ? EPI_SPLIT_CS : EPI_SPLIT,
                            by_rows ? l0 : 0, by_rows ? 0 : l0, by_rows ? M - l0 : M,
                            by_rows ? N : N - l0, wt.splits, wt.kchunk);
    s.n = 2;
    s.finish = FIN_SPLITK_REDUCE;
    s.probe_after = 1;  // bench.py: end of the GEMM launches (before the reduce)
    s.slab_bytes = wtail_bytes();
  } else {
    const int epi = pl.splits > 1 ? (acc_cs ? EPI_SPLIT_CS : EPI_SPLIT) : p.epi;
    s.launch[0] = launch_of(p, sw, pl.big, s.wide, epi, 0, 0, M, N, pl.splits, pl.kchunk);
    s.n = 1;
    s.finish = pl.splits > 1 ? FIN_SPLITK_REDUCE : FIN_NONE;
    s.slab_bytes = pl.splits > 1 ? (int64_t)pl.splits * M * N * f32 : 0;
  }

  const bool g4 = s.launch[0].family != G128;
  if (p.epi == MMPT_EPI_BF16_DGELU_COLSUM || p.epi == MMPT_EPI_BF16_DQGELU_COLSUM) {
    // one partial row per 128-row half tile of the kernel that runs (gemm4p: 256-row tiles;
    // gemm128: 128-row)
    s.c2_rows = s.c2_rows_written = 2 * ((M + s.launch[0].tile - 1) / s.launch[0].tile);
  } else if (acc_cs && g4) {
    // one partial row per (K split, 256-column tile): see gemm4p_body's CSA; the weight-gradient
    // tail split's row tail may run more splits than the plan.  With less workspace the call
    // runs fewer splits; under the weight-gradient tail split its parts write subsets of the
    // rows, so none counts as written.
    const int64_t tn = (N + 255) / 256;
    s.c2_rows = std::max<int64_t>(pl.splits, wt.dim == 1 ? wt.splits : 1) * tn;
    s.c2_rows_written = wt.dim != 0 ? 0 : pl.splits * tn;
  }
  return s;
}

// ---- the shape-only answers (include/mmpt.h): the schedule of the assumed problem — 16-B
// aligned operands and workspace, the given layouts (K-contiguous where the query takes none)
GemmSchedule assumed_schedule(int la, int lb, int epi, int64_t M, int64_t N, int64_t K,
                              int64_t ws_bytes, const GemmSwitches& sw) {
  return gemm_schedule(GemmProblem{la, lb, epi, M, N, K, true, ws_bytes, true}, sw);
}
constexpr int64_t WS_ALL = INT64_MAX;  // all the workspace the problem wants

int64_t gemm_workspace_bytes(int64_t M, int64_t N, int64_t K, int epi, const GemmSwitches& sw) {
  // (ROWS_K x ROWS_K: the only layout the step's forward / dX GEMMs, which the tail split takes, use)
  return assumed_schedule(MMPT_ROWS_K, MMPT_ROWS_K, epi, M, N, K, WS_ALL, sw).workspace_bytes;
}
// The query answers for BOTH column-sum epilogues: the larger count when the erf and quick forms
// would take different kernels (N % 8 != 0: the fast erf form needs it, the general quick form
// does not).
int64_t gemm_colsum_rows(int64_t M, int64_t N, int64_t K, const GemmSwitches& sw) {
  auto rows = [&](int epi) { return assumed_schedule(MMPT_ROWS_K, MMPT_ROWS_K, epi, M, N, K, WS_ALL, sw).c2_rows; };
  return std::max(rows(MMPT_EPI_BF16_DGELU_COLSUM), rows(MMPT_EPI_BF16_DQGELU_COLSUM));
}
int64_t gemm_acc_colsum_rows(int64_t M, int64_t N, int64_t K, const GemmSwitches& sw) {
  return assumed_schedule(MMPT_K_ROWS, MMPT_K_ROWS, MMPT_EPI_F32_ACC_COLSUM, M, N, K, WS_ALL, sw).c2_rows;
}

}  // namespace
}  // namespace mmpt
