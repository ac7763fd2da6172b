// K20: the post-LN family (RoBERTa, tf:models/roberta/modeling_roberta.py): LayerNorm AFTER the
// residual add — RobertaSelfOutput / RobertaOutput `LayerNorm(dropout(dense(x)) + input)`, the
// LayerNorm over the summed word / type / position embeddings (RobertaEmbeddings) and the
// LayerNorm of RobertaLMHead, which reads a bf16 activation.  fp32 statistics, as autocast runs
// aten::layer_norm in fp32.
//
// Forward kernels: one wave per row, float4 per lane.  Each mode fills the row's registers its
// own way (the residual add with dropout, the embedding sum, the bf16 row); the statistics and
// the normalise are rownorm.h's, the ones layernorm.hip's ln_fwd32_kernel runs.  For the two
// entries whose row is fp32 (add_layernorm, roberta_embed) LN over the same fp32 row gives the
// same bits (tests/test_roberta_gpu.py pins it); for the bf16 row of mlm_ln hipcc fuses the
// squares differently and rstd may move by an ulp.  Backward kernels: one workgroup (256
// threads) per row, grid-stride, rownorm.h's backward row pieces; the per-thread dγ / dβ /
// bias-gradient accumulators go to [block][3][h] partials that partials_reduce sums in block
// order.  No atomics: every result is bitwise reproducible.  The dropout
// masks follow K16's element numbering (philox.h): the float4 at quad q = row * h/4 + i takes the
// four words of dropout_words(q, site, seed).
#include <float.h>

#include "philox.h"
#include "rownorm.h"

namespace mmpt {
namespace {

constexpr int PL_WAVES = 4;
constexpr int PL_BLOCKS = 1024;
enum { PL_ADD = 0, PL_EMB = 1, PL_MLM = 2, PL_LN16 = 3, PL_EMBN = 4 };  // LN16: MLM's backward without the dGELU
// EMBN: EMB with NEFTune noise on the gathered word row (a mode of its own, so that EMB's
// instantiations are the code they were)
constexpr bool pl_emb(int mode) { return mode == PL_EMB || mode == PL_EMBN; }

// drop of one bf16 value held as a float: bf16(x * scale) (one rounding) or +0 (dropout.hip)
__device__ __forceinline__ float drop_bf_f(float x, bool keep, float scale) {
  return keep ? round_bf(x * scale) : 0.f;
}

struct PlArgs {
  int rows, h;
  float eps;
  const float* w;
  const float* b;
  const float* mean_in;
  const float* rstd_in;
  // the row the LayerNorm reads
  const float* x32;      // ADD fwd: resid; ADD bwd: s  (dense fp32 [rows][h])
  const bf16_t* x16;     // ADD fwd: v; MLM: g  (bf16, leading dimension ld_x16)
  long ld_x16;
  const int64_t* ids;    // EMB: token ids [rows]
  const int64_t* pos;    // EMB: position ids [rows]
  const float* word;     // EMB: [vocab][h]
  const float* ptab;     // EMB: [max_pos][h]
  const float* type0;    // EMB: [h]
  int vocab, max_pos;
  // gradients in (backward)
  const float* dy32;
  const bf16_t* dy16;
  long ld_dy16;
  const bf16_t* pre;     // MLM bwd: the head dense's pre-activation
  long ld_pre;
  // outputs
  float* s;              // ADD fwd: the sum the LayerNorm reads
  float* o32;            // fwd: y32 / h32; bwd: ds32 / de
  bf16_t* o16;           // fwd: y16 / h16 / n16; bwd: dvb / dpre
  long ld_o16;
  float* mean;
  float* rstd;
  float* partials;
  int want_q2;
  // dropout
  uint32_t thr;
  float scale;
  uint64_t seed, site;
  // EMBN: the embedding noise (philox.h embed_noise_add)
  float nmag;
  uint64_t nseed, nsite;
};

// Hands row_stats four plain registers, as a float4 load would, so that it compiles as it does for
// ln_fwd32_kernel; without it EMBN at MAXJ = 8 also takes 82 VGPRs, one occupancy step down.
__device__ __forceinline__ void opaque4(float4& v) {
  asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
}

__device__ __forceinline__ long clampl(long v, long hi) { return v < 0 ? 0 : v >= hi ? hi - 1 : v; }

// e = (word[id] + type[0]) + pos[p]: HF's order (inputs_embeds + token_type_embeddings, then
// + position_embeddings), fp32
__device__ __forceinline__ float4 emb_sum(const float4 t, const float4 ty, const float4 ps) {
  return make_float4((t.x + ty.x) + ps.x, (t.y + ty.y) + ps.y, (t.z + ty.z) + ps.z,
                     (t.w + ty.w) + ps.w);
}
// EMBN: e = ((word[id] + noise) + type[0]) + pos[p] — HF's neftune hook sits on word_embeddings.
// The forward and the backward both gather through this, so they draw the same noise.
__device__ __forceinline__ float4 emb_noisy(float4 t, const PlArgs& a, int row, int nv, int i) {
  const philox4 k = dropout_words((uint64_t)row * nv + i, a.nsite, a.nseed);
  return make_float4(embed_noise_add(t.x, k.w[0], a.nmag), embed_noise_add(t.y, k.w[1], a.nmag),
                     embed_noise_add(t.z, k.w[2], a.nmag), embed_noise_add(t.w, k.w[3], a.nmag));
}

template <int MODE, int MAXJ>
__global__ __launch_bounds__(256) void postln_fwd_kernel(const PlArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * PL_WAVES + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  const int h = a.h, nv = h >> 2;
  const float4 *wr = nullptr, *pr = nullptr;
  if (pl_emb(MODE)) {
    wr = (const float4*)(a.word + clampl(a.ids[row], a.vocab) * h);
    pr = (const float4*)(a.ptab + clampl(a.pos[row], a.max_pos) * h);
  }
  float4 v[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int i = j * 64 + lane;
    v[j] = zero4();
    if (i < nv) {
      if (MODE == PL_ADD) {
        const float4 r = ((const float4*)(a.x32 + (long)row * h))[i];
        float4 u = ld_bf16x4(a.x16 + (long)row * a.ld_x16 + i * 4);
        if (a.thr != 0) {
          const philox4 k = dropout_words((uint64_t)row * nv + i, a.site, a.seed);
          u.x = drop_bf_f(u.x, k.w[0] >= a.thr, a.scale);
          u.y = drop_bf_f(u.y, k.w[1] >= a.thr, a.scale);
          u.z = drop_bf_f(u.z, k.w[2] >= a.thr, a.scale);
          u.w = drop_bf_f(u.w, k.w[3] >= a.thr, a.scale);
        }
        v[j] = make_float4(r.x + u.x, r.y + u.y, r.z + u.z, r.w + u.w);
        ((float4*)(a.s + (long)row * h))[i] = v[j];
      } else if (MODE == PL_EMB) {
        v[j] = emb_sum(wr[i], ((const float4*)a.type0)[i], pr[i]);
      } else if (MODE == PL_EMBN) {
        v[j] = emb_sum(emb_noisy(wr[i], a, row, nv, i), ((const float4*)a.type0)[i], pr[i]);
      } else {
        v[j] = ld_bf16x4(a.x16 + (long)row * a.ld_x16 + i * 4);
      }
      if (MODE != PL_ADD) opaque4(v[j]);
    }
  }
  float mean, rstd;
  row_stats<MAXJ, false>(v, lane, nv, h, a.eps, mean, rstd);
  if (lane == 0) {
    a.mean[row] = mean;
    a.rstd[row] = rstd;
  }
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int i = j * 64 + lane;
    if (i >= nv) continue;
    float4 y = affine4(xhat4(v[j], mean, rstd), ((const float4*)a.w)[i], ((const float4*)a.b)[i]);
    if (pl_emb(MODE) && a.thr != 0) {  // h0 = dropout(y), fp32 (mmpt_dropout_f32's arithmetic)
      const philox4 k = dropout_words((uint64_t)row * nv + i, a.site, a.seed);
      y.x = k.w[0] >= a.thr ? y.x * a.scale : 0.f;
      y.y = k.w[1] >= a.thr ? y.y * a.scale : 0.f;
      y.z = k.w[2] >= a.thr ? y.z * a.scale : 0.f;
      y.w = k.w[3] >= a.thr ? y.w * a.scale : 0.f;
    }
    if (MODE != PL_MLM) ((float4*)(a.o32 + (long)row * h))[i] = y;
    st_bf16x4(a.o16 + (long)row * a.ld_o16 + i * 4, y);
  }
}

// partials layout: [block][3][h] = dγ, dβ, q2 (ADD: Σ dvb; EMB: Σ de; MLM: Σ dpre)
template <int MODE, int PT>
__global__ __launch_bounds__(256) void postln_bwd_kernel(const PlArgs a) {
  __shared__ float red[2][4][2];
  const int tid = threadIdx.x;
  const int h = a.h, nv = h >> 2;
  float4 aw[PT], ab[PT], aq[PT], ww[PT];
#pragma unroll
  for (int j = 0; j < PT; ++j) {
    aw[j] = ab[j] = aq[j] = zero4();
    const int i = j * 256 + tid;
    ww[j] = i < nv ? ((const float4*)a.w)[i] : zero4();
  }
  int par = 0;
  for (int row = blockIdx.x; row < a.rows; row += gridDim.x, par ^= 1) {
    const float mu = a.mean_in[row], rs = a.rstd_in[row];
    const float4 *wr = nullptr, *pr = nullptr;
    if (pl_emb(MODE)) {
      wr = (const float4*)(a.word + clampl(a.ids[row], a.vocab) * h);
      pr = (const float4*)(a.ptab + clampl(a.pos[row], a.max_pos) * h);
    }
    float4 xh[PT], g1[PT];
    float s1a = 0.f, s1b = 0.f;
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int i = j * 256 + tid;
      xh[j] = g1[j] = zero4();
      if (i >= nv) continue;
      float4 xv, d1;
      if (MODE == PL_ADD) {
        xv = ((const float4*)(a.x32 + (long)row * h))[i];
        if (a.dy32 != nullptr) {
          d1 = ((const float4*)(a.dy32 + (long)row * h))[i];
          if (a.dy16 != nullptr) {
            const float4 e = ld_bf16x4(a.dy16 + (long)row * a.ld_dy16 + i * 4);
            d1 = make_float4(d1.x + e.x, d1.y + e.y, d1.z + e.z, d1.w + e.w);
          }
        } else {
          d1 = ld_bf16x4(a.dy16 + (long)row * a.ld_dy16 + i * 4);
        }
      } else if (pl_emb(MODE)) {
        const float4 t = MODE == PL_EMBN ? emb_noisy(wr[i], a, row, nv, i) : wr[i];
        xv = emb_sum(t, ((const float4*)a.type0)[i], pr[i]);
        d1 = ((const float4*)(a.dy32 + (long)row * h))[i];
        if (a.dy16 != nullptr) {  // + the bf16 input gradient of the GEMM that read bf16(h0)
          const float4 e = ld_bf16x4(a.dy16 + (long)row * a.ld_dy16 + i * 4);
          d1 = make_float4(d1.x + e.x, d1.y + e.y, d1.z + e.z, d1.w + e.w);
        }
        if (a.thr != 0) {  // the dropout backward: the forward's map on the gradient
          const philox4 k = dropout_words((uint64_t)row * nv + i, a.site, a.seed);
          d1.x = k.w[0] >= a.thr ? d1.x * a.scale : 0.f;
          d1.y = k.w[1] >= a.thr ? d1.y * a.scale : 0.f;
          d1.z = k.w[2] >= a.thr ? d1.z * a.scale : 0.f;
          d1.w = k.w[3] >= a.thr ? d1.w * a.scale : 0.f;
        }
      } else {
        xv = ld_bf16x4(a.x16 + (long)row * a.ld_x16 + i * 4);
        d1 = ld_bf16x4(a.dy16 + (long)row * a.ld_dy16 + i * 4);
      }
      xh[j] = xhat4(xv, mu, rs);
      bwd_accum(xh[j], d1, ww[j], g1[j], s1a, s1b, aw[j], ab[j]);
    }
    row_sums_put(red[par], 0, s1a, s1b);
    __syncthreads();
    const float inv_h = 1.0f / (float)h;
    const float c1a = row_sum_get(red[par], 0) * inv_h, c1b = row_sum_get(red[par], 1) * inv_h;
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int i = j * 256 + tid;
      if (i >= nv) continue;
      float4 o = zero4();
      dx_add(o, rs, g1[j], xh[j], c1a, c1b);
      if (MODE != PL_MLM && MODE != PL_LN16) ((float4*)(a.o32 + (long)row * h))[i] = o;
      if (pl_emb(MODE)) {  // dtype[0] = Σ_rows de in fp32: these gradients are outside autocast
        aq[j].x += o.x; aq[j].y += o.y; aq[j].z += o.z; aq[j].w += o.w;
        continue;
      }
      float4 q = make_float4(round_bf(o.x), round_bf(o.y), round_bf(o.z), round_bf(o.w));
      if (MODE == PL_ADD) {  // dvb = drop(bf16(ds)) with the forward's site
        if (a.thr != 0) {
          const philox4 k = dropout_words((uint64_t)row * nv + i, a.site, a.seed);
          q.x = drop_bf_f(q.x, k.w[0] >= a.thr, a.scale);
          q.y = drop_bf_f(q.y, k.w[1] >= a.thr, a.scale);
          q.z = drop_bf_f(q.z, k.w[2] >= a.thr, a.scale);
          q.w = drop_bf_f(q.w, k.w[3] >= a.thr, a.scale);
        }
      } else if (MODE == PL_MLM) {  // dpre = bf16(dg * gelu'(pre)): the BF16_DGELU epilogue's arithmetic
        const float4 pv = ld_bf16x4(a.pre + (long)row * a.ld_pre + i * 4);
        q.x = round_bf(q.x * gelu_grad_f(pv.x));
        q.y = round_bf(q.y * gelu_grad_f(pv.y));
        q.z = round_bf(q.z * gelu_grad_f(pv.z));
        q.w = round_bf(q.w * gelu_grad_f(pv.w));
      }
      st_bf16x4(a.o16 + (long)row * a.ld_o16 + i * 4, q);
      if (a.want_q2) {
        aq[j].x += q.x; aq[j].y += q.y; aq[j].z += q.z; aq[j].w += q.w;
      }
    }
  }
  float4* out = (float4*)(a.partials + (long)blockIdx.x * 3 * h);
#pragma unroll
  for (int j = 0; j < PT; ++j) {
    const int i = j * 256 + tid;
    if (i >= nv) continue;
    out[i] = aw[j];
    out[nv + i] = ab[j];
    if (a.want_q2) out[2 * nv + i] = aq[j];
  }
}

// the entry points cap h at 4096, so pick_maxj / pick_pt always find an instantiation
template <int MODE>
int launch_fwd(const PlArgs& a, hipStream_t s, const char* what) {
  const unsigned g = (unsigned)((a.rows + PL_WAVES - 1) / PL_WAVES);
  dispatch_maxj(pick_maxj(a.h), [&](auto J) {
    constexpr int MJ = decltype(J)::value == 12 ? 16 : decltype(J)::value;  // no 12 here: 16's code
    postln_fwd_kernel<MODE, MJ><<<g, 256, 0, s>>>(a);
  });
  return check_launch(what);
}

// d0 / d1 / d2 (+=, nullable) take Σ dγ, Σ dβ and quantity 2; with round2 quantity 2 is a bias
// gradient: rounded to bf16 and also added to d2b
template <int MODE>
int launch_bwd(const PlArgs& a, float* d0, float* d1, float* d2, float* d2b, int round2,
               hipStream_t s, const char* what) {
  const int nblk = (int)std::min<int64_t>(PL_BLOCKS, a.rows);
  dispatch_pt(pick_pt(a.h), [&](auto PT) {
    postln_bwd_kernel<MODE, decltype(PT)::value><<<nblk, 256, 0, s>>>(a);
  });
  int rc = check_launch(what);
  if (rc) return rc;
  if (d0 == nullptr && d1 == nullptr && d2 == nullptr) return rc;
  dim3 rg((unsigned)((a.h + 63) / 64), 3u);
  partials_reduce<<<rg, 256, 0, s>>>(nblk, a.h, 3, a.partials, d0, d1, d2, nullptr, nullptr,
                                     round2 ? 2 : -1, d2b);
  return check_launch(what);
}

}  // namespace
}  // namespace mmpt

using namespace mmpt;

#define MMPT_PL_SHAPE(what)                                                                     \
  MMPT_REQUIRE(rows > 0 && rows < ((int64_t)1 << 31) && h > 0 && h % 8 == 0 && h <= 4096,       \
               what ": rows in [1, 2^31), h a positive multiple of 8 and <= 4096 (rows %lld, " \
               "h %lld)", (long long)rows, (long long)h)
#define MMPT_PL_LD(what, ld) \
  MMPT_REQUIRE((ld) >= h && (ld) % 8 == 0, what ": " #ld " must be a multiple of 8 and >= h")
#define MMPT_PL_P(what) \
  MMPT_REQUIRE(p >= 0.0 && p < 1.0, what ": p must lie in [0, 1), got %g", p)

extern "C" int mmpt_add_layernorm_fwd(int64_t rows, int64_t h, float eps, const float* resid,
                                      const void* v, int64_t ld_v, const float* w, const float* b,
                                      float* s, float* y32, void* y16, int64_t ld_y16, float* mean,
                                      float* rstd, double p, uint64_t seed, uint64_t site,
                                      void* stream) {
  MMPT_PL_SHAPE("add_layernorm_fwd");
  MMPT_PL_P("add_layernorm_fwd");
  MMPT_PL_LD("add_layernorm_fwd", ld_v);
  MMPT_PL_LD("add_layernorm_fwd", ld_y16);
  MMPT_REQUIRE(resid && v && w && b && s && y32 && y16 && mean && rstd,
               "add_layernorm_fwd: null pointer");
  MMPT_REQUIRE(al16(resid) && al16(v) && al16(w) && al16(b) && al16(s) && al16(y32) && al16(y16),
               "add_layernorm_fwd: pointers must be 16-byte aligned");
  PlArgs a = {};
  a.rows = (int)rows; a.h = (int)h; a.eps = eps; a.w = w; a.b = b;
  a.x32 = resid; a.x16 = (const bf16_t*)v; a.ld_x16 = ld_v;
  a.s = s; a.o32 = y32; a.o16 = (bf16_t*)y16; a.ld_o16 = ld_y16; a.mean = mean; a.rstd = rstd;
  a.thr = dropout_threshold(p); a.scale = dropout_scale(p); a.seed = seed; a.site = site;
  return launch_fwd<PL_ADD>(a, (hipStream_t)stream, "add_layernorm_fwd");
}

extern "C" int64_t mmpt_add_layernorm_bwd_workspace_bytes(int64_t rows, int64_t h) {
  return std::min<int64_t>(PL_BLOCKS, rows) * 3 * h * (int64_t)sizeof(float);
}

extern "C" int mmpt_add_layernorm_bwd(int64_t rows, int64_t h, const float* s, const float* mean,
                                      const float* rstd, const float* w, const float* dy32,
                                      const void* dyb, int64_t ld_dyb, float* ds32, void* dvb,
                                      int64_t ld_dvb, float* dw, float* db, float* dsum,
                                      float* dsum2, double p, uint64_t seed, uint64_t site,
                                      void* workspace, void* stream) {
  MMPT_PL_SHAPE("add_layernorm_bwd");
  MMPT_PL_P("add_layernorm_bwd");
  MMPT_REQUIRE(dy32 || dyb, "add_layernorm_bwd: at least one of dy32 / dyb is needed");
  MMPT_REQUIRE(dyb == nullptr || (ld_dyb >= h && ld_dyb % 8 == 0),
               "add_layernorm_bwd: ld_dyb must be a multiple of 8 and >= h");
  MMPT_PL_LD("add_layernorm_bwd", ld_dvb);
  MMPT_REQUIRE(s && mean && rstd && w && ds32 && dvb && workspace, "add_layernorm_bwd: null pointer");
  MMPT_REQUIRE(dsum2 == nullptr || dsum, "add_layernorm_bwd: dsum2 needs dsum");
  MMPT_REQUIRE(al16(s) && al16(w) && al16(dy32) && al16(dyb) && al16(ds32) && al16(dvb) &&
                   al16(workspace),
               "add_layernorm_bwd: pointers must be 16-byte aligned");
  PlArgs a = {};
  a.rows = (int)rows; a.h = (int)h; a.w = w; a.mean_in = mean; a.rstd_in = rstd; a.x32 = s;
  a.dy32 = dy32; a.dy16 = (const bf16_t*)dyb; a.ld_dy16 = ld_dyb;
  a.o32 = ds32; a.o16 = (bf16_t*)dvb; a.ld_o16 = ld_dvb;
  a.partials = (float*)workspace; a.want_q2 = dsum != nullptr;
  a.thr = dropout_threshold(p); a.scale = dropout_scale(p); a.seed = seed; a.site = site;
  return launch_bwd<PL_ADD>(a, dw, db, dsum, dsum2, 1, (hipStream_t)stream, "add_layernorm_bwd");
}

#define MMPT_PL_EMB_ARGS(what)                                                                  \
  MMPT_REQUIRE(vocab > 0 && max_pos > 0 && vocab <= INT32_MAX && max_pos <= INT32_MAX,          \
               what ": bad table sizes");                                                       \
  MMPT_REQUIRE(ids && pos && word && pos_table && type_row && w, what ": null pointer");        \
  MMPT_REQUIRE(al16(word) && al16(pos_table) && al16(type_row) && al16(w),                      \
               what ": pointers must be 16-byte aligned")

// mag finite and >= 0 (a NaN fails both comparisons)
#define MMPT_PL_MAG(what) \
  MMPT_REQUIRE(mag >= 0.f && mag <= FLT_MAX, what ": mag must be finite and >= 0, got %g", (double)mag)

// MODE = PL_EMB: mmpt_roberta_embed_fwd (mag, noise_site unused); PL_EMBN: the noise entry
template <int MODE>
static int roberta_embed_fwd_impl(int64_t rows, int64_t h, float eps, const int64_t* ids,
                                  const int64_t* pos, const float* word, int64_t vocab,
                                  const float* pos_table, int64_t max_pos, const float* type_row,
                                  const float* w, const float* b, float* h32, void* h16,
                                  float* mean, float* rstd, double p, uint64_t seed, uint64_t site,
                                  float mag, uint64_t noise_seed, uint64_t noise_site,
                                  void* stream) {
  MMPT_PL_SHAPE("roberta_embed_fwd");
  MMPT_PL_P("roberta_embed_fwd");
  MMPT_PL_EMB_ARGS("roberta_embed_fwd");
  MMPT_REQUIRE(b && h32 && h16 && mean && rstd, "roberta_embed_fwd: null pointer");
  MMPT_REQUIRE(al16(b) && al16(h32) && al16(h16),
               "roberta_embed_fwd: pointers must be 16-byte aligned");
  PlArgs a = {};
  a.rows = (int)rows; a.h = (int)h; a.eps = eps; a.w = w; a.b = b;
  a.ids = ids; a.pos = pos; a.word = word; a.ptab = pos_table; a.type0 = type_row;
  a.vocab = (int)vocab; a.max_pos = (int)max_pos;
  a.o32 = h32; a.o16 = (bf16_t*)h16; a.ld_o16 = h; a.mean = mean; a.rstd = rstd;
  a.thr = dropout_threshold(p); a.scale = dropout_scale(p); a.seed = seed; a.site = site;
  a.nmag = mag; a.nseed = noise_seed; a.nsite = noise_site;
  return launch_fwd<MODE>(a, (hipStream_t)stream, "roberta_embed_fwd");
}

extern "C" int mmpt_roberta_embed_fwd(int64_t rows, int64_t h, float eps, const int64_t* ids,
                                      const int64_t* pos, const float* word, int64_t vocab,
                                      const float* pos_table, int64_t max_pos,
                                      const float* type_row, const float* w, const float* b,
                                      float* h32, void* h16, float* mean, float* rstd, double p,
                                      uint64_t seed, uint64_t site, void* stream) {
  return roberta_embed_fwd_impl<PL_EMB>(rows, h, eps, ids, pos, word, vocab, pos_table, max_pos,
                                        type_row, w, b, h32, h16, mean, rstd, p, seed, site, 0.f,
                                        0, 0, stream);
}

extern "C" int mmpt_roberta_embed_noise_fwd(int64_t rows, int64_t h, float eps, const int64_t* ids,
                                            const int64_t* pos, const float* word, int64_t vocab,
                                            const float* pos_table, int64_t max_pos,
                                            const float* type_row, const float* w, const float* b,
                                            float* h32, void* h16, float* mean, float* rstd,
                                            double p, uint64_t seed, uint64_t site, float mag,
                                            uint64_t noise_seed, uint64_t noise_site,
                                            void* stream) {
  MMPT_PL_MAG("roberta_embed_noise_fwd");
  return roberta_embed_fwd_impl<PL_EMBN>(rows, h, eps, ids, pos, word, vocab, pos_table, max_pos,
                                         type_row, w, b, h32, h16, mean, rstd, p, seed, site, mag,
                                         noise_seed, noise_site, stream);
}

extern "C" int64_t mmpt_roberta_embed_bwd_workspace_bytes(int64_t rows, int64_t h) {
  return mmpt_add_layernorm_bwd_workspace_bytes(rows, h);
}

template <int MODE>
static int roberta_embed_bwd_impl(int64_t rows, int64_t h, const int64_t* ids, const int64_t* pos,
                                  const float* word, int64_t vocab, const float* pos_table,
                                  int64_t max_pos, const float* type_row, const float* mean,
                                  const float* rstd, const float* w, const float* dh,
                                  const void* dhb, float* de, float* dw, float* db, float* dtype,
                                  double p, uint64_t seed, uint64_t site, float mag,
                                  uint64_t noise_seed, uint64_t noise_site, void* workspace,
                                  void* stream) {
  MMPT_PL_SHAPE("roberta_embed_bwd");
  MMPT_PL_P("roberta_embed_bwd");
  MMPT_PL_EMB_ARGS("roberta_embed_bwd");
  MMPT_REQUIRE(mean && rstd && dh && de && workspace, "roberta_embed_bwd: null pointer");
  MMPT_REQUIRE(al16(dh) && al16(dhb) && al16(de) && al16(workspace),
               "roberta_embed_bwd: pointers must be 16-byte aligned");
  PlArgs a = {};
  a.rows = (int)rows; a.h = (int)h; a.w = w; a.mean_in = mean; a.rstd_in = rstd;
  a.ids = ids; a.pos = pos; a.word = word; a.ptab = pos_table; a.type0 = type_row;
  a.vocab = (int)vocab; a.max_pos = (int)max_pos;
  a.dy32 = dh; a.dy16 = (const bf16_t*)dhb; a.ld_dy16 = h; a.o32 = de; a.partials = (float*)workspace; a.want_q2 = dtype != nullptr;
  a.thr = dropout_threshold(p); a.scale = dropout_scale(p); a.seed = seed; a.site = site;
  a.nmag = mag; a.nseed = noise_seed; a.nsite = noise_site;
  return launch_bwd<MODE>(a, dw, db, dtype, nullptr, 0, (hipStream_t)stream, "roberta_embed_bwd");
}

extern "C" int mmpt_roberta_embed_bwd(int64_t rows, int64_t h, const int64_t* ids,
                                      const int64_t* pos, const float* word, int64_t vocab,
                                      const float* pos_table, int64_t max_pos,
                                      const float* type_row, const float* mean, const float* rstd,
                                      const float* w, const float* dh, const void* dhb,
                                      float* de, float* dw, float* db, float* dtype, double p, uint64_t seed,
                                      uint64_t site, void* workspace, void* stream) {
  return roberta_embed_bwd_impl<PL_EMB>(rows, h, ids, pos, word, vocab, pos_table, max_pos,
                                        type_row, mean, rstd, w, dh, dhb, de, dw, db, dtype, p,
                                        seed, site, 0.f, 0, 0, workspace, stream);
}

// The backward of mmpt_roberta_embed_noise_fwd: it gathers e again and so draws the forward's
// noise again (same mag, noise_seed and noise_site); nothing random was stored.
extern "C" int mmpt_roberta_embed_noise_bwd(int64_t rows, int64_t h, const int64_t* ids,
                                            const int64_t* pos, const float* word, int64_t vocab,
                                            const float* pos_table, int64_t max_pos,
                                            const float* type_row, const float* mean,
                                            const float* rstd, const float* w, const float* dh,
                                            const void* dhb, float* de, float* dw, float* db,
                                            float* dtype, double p, uint64_t seed, uint64_t site,
                                            float mag, uint64_t noise_seed,
                                            uint64_t noise_site, void* workspace, void* stream) {
  MMPT_PL_MAG("roberta_embed_noise_bwd");
  return roberta_embed_bwd_impl<PL_EMBN>(rows, h, ids, pos, word, vocab, pos_table, max_pos,
                                         type_row, mean, rstd, w, dh, dhb, de, dw, db, dtype, p,
                                         seed, site, mag, noise_seed, noise_site, workspace,
                                         stream);
}

extern "C" int mmpt_mlm_ln_fwd(int64_t rows, int64_t h, float eps, const void* g, int64_t ld_g,
                               const float* w, const float* b, void* n16, int64_t ld_n16,
                               float* mean, float* rstd, void* stream) {
  MMPT_PL_SHAPE("mlm_ln_fwd");
  MMPT_PL_LD("mlm_ln_fwd", ld_g);
  MMPT_PL_LD("mlm_ln_fwd", ld_n16);
  MMPT_REQUIRE(g && w && b && n16 && mean && rstd, "mlm_ln_fwd: null pointer");
  MMPT_REQUIRE(al16(g) && al16(w) && al16(b) && al16(n16),
               "mlm_ln_fwd: pointers must be 16-byte aligned");
  PlArgs a = {};
  a.rows = (int)rows; a.h = (int)h; a.eps = eps; a.w = w; a.b = b;
  a.x16 = (const bf16_t*)g; a.ld_x16 = ld_g;
  a.o16 = (bf16_t*)n16; a.ld_o16 = ld_n16; a.mean = mean; a.rstd = rstd;
  return launch_fwd<PL_MLM>(a, (hipStream_t)stream, "mlm_ln_fwd");
}

extern "C" int64_t mmpt_mlm_ln_bwd_workspace_bytes(int64_t rows, int64_t h) {
  return mmpt_add_layernorm_bwd_workspace_bytes(rows, h);
}

extern "C" int mmpt_mlm_ln_bwd(int64_t rows, int64_t h, const void* g, int64_t ld_g,
                               const float* mean, const float* rstd, const float* w,
                               const void* dn16, int64_t ld_dn16, const void* pre, int64_t ld_pre,
                               void* dpre, int64_t ld_dpre, float* dw, float* db, float* dsum,
                               void* workspace, void* stream) {
  MMPT_PL_SHAPE("mlm_ln_bwd");
  MMPT_PL_LD("mlm_ln_bwd", ld_g);
  MMPT_PL_LD("mlm_ln_bwd", ld_dn16);
  MMPT_PL_LD("mlm_ln_bwd", ld_pre);
  MMPT_PL_LD("mlm_ln_bwd", ld_dpre);
  MMPT_REQUIRE(g && mean && rstd && w && dn16 && pre && dpre && workspace,
               "mlm_ln_bwd: null pointer");
  MMPT_REQUIRE(al16(g) && al16(w) && al16(dn16) && al16(pre) && al16(dpre) && al16(workspace),
               "mlm_ln_bwd: pointers must be 16-byte aligned");
  PlArgs a = {};
  a.rows = (int)rows; a.h = (int)h; a.w = w; a.mean_in = mean; a.rstd_in = rstd;
  a.x16 = (const bf16_t*)g; a.ld_x16 = ld_g;
  a.dy16 = (const bf16_t*)dn16; a.ld_dy16 = ld_dn16;
  a.pre = (const bf16_t*)pre; a.ld_pre = ld_pre;
  a.o16 = (bf16_t*)dpre; a.ld_o16 = ld_dpre;
  a.partials = (float*)workspace; a.want_q2 = dsum != nullptr;
  return launch_bwd<PL_MLM>(a, dw, db, dsum, nullptr, 1, (hipStream_t)stream, "mlm_ln_bwd");
}

extern "C" int64_t mmpt_ln16_bwd_workspace_bytes(int64_t rows, int64_t h) {
  return mmpt_add_layernorm_bwd_workspace_bytes(rows, h);
}

extern "C" int mmpt_ln16_bwd(int64_t rows, int64_t h, const void* c, int64_t ld_c,
                             const float* mean, const float* rstd, const float* w,
                             const void* dn16, int64_t ld_dn16, void* dc, int64_t ld_dc, float* dw,
                             float* db, void* workspace, void* stream) {
  MMPT_PL_SHAPE("ln16_bwd");
  MMPT_PL_LD("ln16_bwd", ld_c);
  MMPT_PL_LD("ln16_bwd", ld_dn16);
  MMPT_PL_LD("ln16_bwd", ld_dc);
  MMPT_REQUIRE(c && mean && rstd && w && dn16 && dc && workspace, "ln16_bwd: null pointer");
  MMPT_REQUIRE(al16(c) && al16(w) && al16(dn16) && al16(dc) && al16(workspace),
               "ln16_bwd: pointers must be 16-byte aligned");
  PlArgs a = {};
  a.rows = (int)rows; a.h = (int)h; a.w = w; a.mean_in = mean; a.rstd_in = rstd;
  a.x16 = (const bf16_t*)c; a.ld_x16 = ld_c;
  a.dy16 = (const bf16_t*)dn16; a.ld_dy16 = ld_dn16;
  a.o16 = (bf16_t*)dc; a.ld_o16 = ld_dc;
  a.partials = (float*)workspace;
  return launch_bwd<PL_LN16>(a, dw, db, nullptr, nullptr, 0, (hipStream_t)stream, "ln16_bwd");
}
