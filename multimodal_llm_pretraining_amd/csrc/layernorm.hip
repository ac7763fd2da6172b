// K4: LayerNorm forward / backward (fp32 statistics, as autocast runs
// aten::layer_norm in fp32).  One wave per row, float4 loads; GPTNeoX's two
// LayerNorms over the same residual (input_layernorm / post_attention_layernorm,
// tf:models/gpt_neox/modeling_gpt_neox.py:245-246, 263-269) share one read of x
// and one set of statistics.  The backward fuses the residual-gradient add and
// both LN input-gradients into one pass; dγ/dβ use a fixed-shape two-stage
// reduction (per-block partial rows, then partials_reduce's column sum) so results
// are bitwise reproducible.  The row arithmetic itself (statistics, x̂, the backward
// accumulate and dx expression) is rownorm.h's, shared with postln.hip.
#include "rownorm.h"

namespace mmpt {
namespace {

constexpr int LN_WAVES = 4;
constexpr int LN_BWD_BLOCKS = 512;

#ifndef MMPT_LN_FWD_PERSIST
#define MMPT_LN_FWD_PERSIST 1  // round 5: Pythia's dual LN 623 -> 551 us (profiles/r05/ln_prefetch/)
#endif
#ifndef MMPT_LN_FWD_BLOCKS
#define MMPT_LN_FWD_BLOCKS 1024
#endif
// PERSIST = true: the workgroups are persistent (a grid of MMPT_LN_FWD_BLOCKS) and γ / β of
// both LayerNorms are staged once per workgroup in LDS ([4][h/4] float4): one workgroup per 4
// rows re-reads 4 × h floats of weights per row through the vector-memory path (32 of its 56
// VMEM instructions per row at h = 2048).
template <int MAXJ, bool PERSIST>
__global__ __launch_bounds__(256) void ln_fwd_kernel(int rows, int h, float eps,
                                                     const float* __restrict__ x, long ldx,
                                                     const float* __restrict__ w1,
                                                     const float* __restrict__ b1, bf16_t* y1,
                                                     const float* __restrict__ w2,
                                                     const float* __restrict__ b2, bf16_t* y2,
                                                     float* mean_out, float* rstd_out, long ldy) {
  extern __shared__ float4 wl[];  // PERSIST: [q][nv] = γ1, β1, γ2, β2
  const int lane = threadIdx.x & 63, nv = h >> 2;
  if (PERSIST) {
    const int nq = y2 != nullptr ? 4 : 2;
    for (int e = threadIdx.x; e < nq * nv; e += 256) {
      const int q = e / nv, i = e - q * nv;
      const float* src = q == 0 ? w1 : q == 1 ? b1 : q == 2 ? w2 : b2;
      wl[e] = ((const float4*)src)[i];
    }
    __syncthreads();
  }
  for (int row = blockIdx.x * LN_WAVES + (threadIdx.x >> 6); row < rows; row += gridDim.x * LN_WAVES) {
    float4 v[MAXJ];
    ld_row<MAXJ>(v, (const float4*)(x + (long)row * ldx), lane, nv);
    float mean, rstd;
    row_stats<MAXJ, false>(v, lane, nv, h, eps, mean, rstd);
    if (lane == 0) {
      mean_out[row] = mean;
      rstd_out[row] = rstd;
    }
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      const int i = j * 64 + lane;
      if (i >= nv) continue;
      const float4 xh = xhat4(v[j], mean, rstd);
      const float4 g = PERSIST ? wl[i] : ((const float4*)w1)[i];
      const float4 bb = PERSIST ? wl[nv + i] : ((const float4*)b1)[i];
      st_norm_bf16x4(y1 + (long)row * ldy, i, xh, g, bb);
      if (y2 != nullptr) {
        const float4 g2 = PERSIST ? wl[2 * nv + i] : ((const float4*)w2)[i];
        const float4 c2 = PERSIST ? wl[3 * nv + i] : ((const float4*)b2)[i];
        st_norm_bf16x4(y2 + (long)row * ldy, i, xh, g2, c2);
      }
    }
    if (!PERSIST) break;  // one workgroup per LN_WAVES rows
  }
}

// LlamaRMSNorm (tf:models/llama/modeling_llama.py LlamaRMSNorm.forward, fp32 under autocast):
// rstd = rsqrt(mean(x²) + eps), y = bf16(w · (x · rstd)) — no mean, no bias.  A kernel of its
// own with the row load written out: as an instantiation of ln_fwd_kernel (ld_row + row_stats)
// hipcc fuses the other square of each pair into the FMA and rstd moves by an ulp.
template <int MAXJ>
__global__ __launch_bounds__(256) void rms_fwd_kernel(int rows, int h, float eps,
                                                      const float* __restrict__ x, long ldx,
                                                      const float* __restrict__ w, bf16_t* y,
                                                      float* rstd_out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nv = h >> 2;
  const float4* xr = (const float4*)(x + (long)row * ldx);
  float4 v[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int i = j * 64 + lane;
    v[j] = i < nv ? xr[i] : zero4();
  }
  float mean, rstd;
  row_stats<MAXJ, true>(v, lane, nv, h, eps, mean, rstd);
  if (lane == 0) rstd_out[row] = rstd;
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int i = j * 64 + lane;
    if (i >= nv) continue;
    st_norm_bf16x4(y + (long)row * h, i, xhat4(v[j], mean, rstd), ((const float4*)w)[i], zero4());
  }
}

// fp32-output LayerNorm (CLIP's pre_layrnorm: its output IS the fp32 residual stream,
// tf:models/clip/modeling_clip.py CLIPVisionTransformer.forward), one wave per row.
template <int MAXJ>
__global__ __launch_bounds__(256) void ln_fwd32_kernel(int rows, int h, float eps,
                                                       const float* __restrict__ x,
                                                       const float* __restrict__ w,
                                                       const float* __restrict__ b, float* y,
                                                       float* mean_out, float* rstd_out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nv = h >> 2;
  float4 v[MAXJ];
  ld_row<MAXJ>(v, (const float4*)(x + (long)row * h), lane, nv);
  float mean, rstd;
  row_stats<MAXJ, false>(v, lane, nv, h, eps, mean, rstd);
  if (lane == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int i = j * 64 + lane;
    if (i >= nv) continue;
    ((float4*)(y + (long)row * h))[i] =
        affine4(xhat4(v[j], mean, rstd), ((const float4*)w)[i], ((const float4*)b)[i]);
  }
}

// Backward, one WAVE per row; every wave holds the 4 accumulator sets of all its rows.
// partials layout: [block][4][h] = dw1, db1, dw2, db2
// DY32: dy1 is fp32 (the fp32-output LayerNorm above); otherwise bf16 (GEMM operand)
template <int MAXJ, bool DY32>
__global__ __launch_bounds__(256) void ln_bwd_kernel(
    int rows, int h, const float* __restrict__ x, long ldx, const float* __restrict__ mean,
    const float* __restrict__ rstd, const bf16_t* __restrict__ dy1, const float* __restrict__ w1,
    const bf16_t* __restrict__ dy2, const float* __restrict__ w2, const float* dresid, float* dx,
    float* __restrict__ partials) {
  __shared__ float red[LN_WAVES][256 * 4];  // staging for the cross-wave dγ/dβ sum
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nv = h >> 2;
  const bool two = dy2 != nullptr;
  float4 aw1[MAXJ], ab1[MAXJ], aw2[MAXJ], ab2[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) aw1[j] = ab1[j] = aw2[j] = ab2[j] = zero4();
  for (int row = blockIdx.x * LN_WAVES + wave; row < rows; row += gridDim.x * LN_WAVES) {
    const float mu = mean[row], rs = rstd[row];
    const float4* xr = (const float4*)(x + (long)row * ldx);
    float4 xh[MAXJ], g1[MAXJ], g2[MAXJ];
    float s1a = 0.f, s1b = 0.f, s2a = 0.f, s2b = 0.f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      const int i = j * 64 + lane;
      xh[j] = g1[j] = g2[j] = zero4();
      if (i >= nv) continue;
      xh[j] = xhat4(xr[i], mu, rs);
      // bwd_accum's arithmetic, kept written out: through the helper hipcc contracts other
      // products into FMAs from MAXJ = 8 up and dx moves by an ulp
      const float4 d1 = DY32 ? ((const float4*)((const float*)(const void*)dy1 + (long)row * h))[i]
                             : ld_bf16x4(dy1 + (long)row * h + i * 4);
      const float4 ww1 = ((const float4*)w1)[i];
      g1[j] = make_float4(d1.x * ww1.x, d1.y * ww1.y, d1.z * ww1.z, d1.w * ww1.w);
      s1a += (g1[j].x * xh[j].x + g1[j].y * xh[j].y) + (g1[j].z * xh[j].z + g1[j].w * xh[j].w);
      s1b += (g1[j].x + g1[j].y) + (g1[j].z + g1[j].w);
      aw1[j].x += d1.x * xh[j].x; aw1[j].y += d1.y * xh[j].y;
      aw1[j].z += d1.z * xh[j].z; aw1[j].w += d1.w * xh[j].w;
      ab1[j].x += d1.x; ab1[j].y += d1.y; ab1[j].z += d1.z; ab1[j].w += d1.w;
      if (two) {
        const float4 d2 = ld_bf16x4(dy2 + (long)row * h + i * 4);
        const float4 ww2 = ((const float4*)w2)[i];
        g2[j] = make_float4(d2.x * ww2.x, d2.y * ww2.y, d2.z * ww2.z, d2.w * ww2.w);
        s2a += (g2[j].x * xh[j].x + g2[j].y * xh[j].y) + (g2[j].z * xh[j].z + g2[j].w * xh[j].w);
        s2b += (g2[j].x + g2[j].y) + (g2[j].z + g2[j].w);
        aw2[j].x += d2.x * xh[j].x; aw2[j].y += d2.y * xh[j].y;
        aw2[j].z += d2.z * xh[j].z; aw2[j].w += d2.w * xh[j].w;
        ab2[j].x += d2.x; ab2[j].y += d2.y; ab2[j].z += d2.z; ab2[j].w += d2.w;
      }
    }
    const float inv_h = 1.0f / (float)h;
    const float c1a = wave_sum(s1a) * inv_h, c1b = wave_sum(s1b) * inv_h;
    float c2a = 0.f, c2b = 0.f;
    if (two) {
      c2a = wave_sum(s2a) * inv_h;
      c2b = wave_sum(s2b) * inv_h;
    }
    float4* dxr = (float4*)(dx + (long)row * h);
    const float4* drr = dresid ? (const float4*)(dresid + (long)row * h) : nullptr;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      const int i = j * 64 + lane;
      if (i >= nv) continue;
      float4 o = drr ? drr[i] : zero4();
      dx_add(o, rs, g1[j], xh[j], c1a, c1b);
      if (two) dx_add(o, rs, g2[j], xh[j], c2a, c2b);
      dxr[i] = o;
    }
  }
  // cross-wave reduction of the per-lane dγ/dβ accumulators, one quantity at a time
  // (fully unrolled: every accumulator index is a compile-time constant, no scratch)
  float* out = partials + (long)blockIdx.x * 4 * h;
#pragma unroll
  for (int qn = 0; qn < 4; ++qn) {
    if (qn >= 2 && !two) break;
#pragma unroll
    for (int j0 = 0; j0 < MAXJ; j0 += 4) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int j = j0 + jj;
        if (j < MAXJ) {
          const float4 val = qn == 0 ? aw1[j] : qn == 1 ? ab1[j] : qn == 2 ? aw2[j] : ab2[j];
          *(float4*)&red[wave][(jj * 64 + lane) * 4] = val;
        }
      }
      __syncthreads();
      for (int e = threadIdx.x; e < 1024; e += 256) {
        const int jj = e >> 8, rem = e & 255;  // rem = lane*4 + comp
        const int j = j0 + jj;
        const int col = (j * 64 + (rem >> 2)) * 4 + (rem & 3);
        if (j < MAXJ && col < h)
          out[qn * h + col] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
      }
      __syncthreads();
    }
  }
}

// Backward, one WORKGROUP per row (256 threads, PT float4 per thread): ~70 VGPRs, so
// 8 waves/SIMD keep enough loads in flight to stream at HBM rate (the wave-per-row
// kernel above holds every row's 4 accumulator sets in one wave: ~240 VGPRs, 2 waves/
// SIMD, latency-bound at ~2.3 TB/s).  Row sums: block_row_sums, one barrier per row.
// Optional fused outputs: dx_bf16 = bf16(dx) (the next GEMMs' operand) and Σ_rows bf16(dx)
// (a bias gradient that autocast's addmm backward would compute from that bf16 tensor) as
// quantity 4.
// partials layout: [block][5][h] = dw1, db1, dw2, db2, Σ bf16(dx)
#ifndef MMPT_LN_BLOCKS
#define MMPT_LN_BLOCKS 1024
#endif
#ifndef MMPT_LN_PREFETCH
#define MMPT_LN_PREFETCH 1  // the residual-gradient row loads before the row-sum barrier (round 5: -0.9%); 0 = after it
#endif
constexpr int LNR_BLOCKS = MMPT_LN_BLOCKS;
// dx_bf16 = bf16(dx) and, with want_dsum, the Σ_rows bf16(dx) accumulator
__device__ __forceinline__ void st_dx_bf16(bf16_t* row, int i, const float4 o, int want_dsum,
                                           float4& as) {
  ((uint2*)row)[i] = make_uint2(pack2(o.x, o.y), pack2(o.z, o.w));
  if (want_dsum) {
    as.x += round_bf(o.x); as.y += round_bf(o.y);
    as.z += round_bf(o.z); as.w += round_bf(o.w);
  }
}
// RMS = true: the RMSNorm backward (μ = 0, no dβ): dx = rstd·(g − x̂·mean(g·x̂)), g = dy·w.
template <int PT, bool RMS>
__global__ __launch_bounds__(256) void ln_bwd_rows_kernel(
    int rows, int h, const float* __restrict__ x, long ldx, const float* __restrict__ mean,
    const float* __restrict__ rstd, const bf16_t* __restrict__ dy1, const float* __restrict__ w1,
    const bf16_t* __restrict__ dy2, const float* __restrict__ w2, const float* dresid, float* dx,
    bf16_t* __restrict__ dxb, int want_dsum, float* __restrict__ partials) {
  __shared__ float red[2][4][4];
  const int tid = threadIdx.x;
  const int nv = h >> 2;
  const bool two = dy2 != nullptr;
  float4 aw1[PT], ab1[PT], aw2[PT], ab2[PT], as[PT];
  float4 ww1[PT], ww2[PT];
#pragma unroll
  for (int j = 0; j < PT; ++j) {
    aw1[j] = ab1[j] = aw2[j] = ab2[j] = as[j] = zero4();
    const int i = j * 256 + tid;
    ww1[j] = i < nv ? ((const float4*)w1)[i] : zero4();
    ww2[j] = (two && i < nv) ? ((const float4*)w2)[i] : zero4();
  }
  int par = 0;
  for (int row = blockIdx.x; row < rows; row += gridDim.x, par ^= 1) {
    const float mu = RMS ? 0.f : mean[row], rs = rstd[row];
    const float4* xr = (const float4*)(x + (long)row * ldx);
    float4 xh[PT], g1[PT], g2[PT], dr[PT];
    float s1a = 0.f, s1b = 0.f, s2a = 0.f, s2b = 0.f;
    const float4* drr = dresid ? (const float4*)(dresid + (long)row * h) : nullptr;
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int i = j * 256 + tid;
      xh[j] = g1[j] = g2[j] = dr[j] = zero4();
      if (i >= nv) continue;
      if (MMPT_LN_PREFETCH && drr) dr[j] = drr[i];
      xh[j] = xhat4(xr[i], mu, rs);
      bwd_accum(xh[j], ld_bf16x4(dy1 + (long)row * h + i * 4), ww1[j], g1[j], s1a, s1b, aw1[j],
                ab1[j]);
      if (two)
        bwd_accum(xh[j], ld_bf16x4(dy2 + (long)row * h + i * 4), ww2[j], g2[j], s2a, s2b,
                  aw2[j], ab2[j]);
    }
    // row_sums_put's steps for four sums, written out: through two calls of the helper hipcc
    // takes 4 more VGPRs at PT = 2 (132: one occupancy step down)
    s1a = wave_sum(s1a);
    s1b = wave_sum(s1b);
    if (two) {
      s2a = wave_sum(s2a);
      s2b = wave_sum(s2b);
    }
    if ((tid & 63) == 0) {
      const int wave = tid >> 6;
      red[par][wave][0] = s1a;
      red[par][wave][1] = s1b;
      red[par][wave][2] = s2a;
      red[par][wave][3] = s2b;
    }
    __syncthreads();
    const float inv_h = 1.0f / (float)h;
    const float c1a = row_sum_get(red[par], 0) * inv_h;
    const float c1b = RMS ? 0.f : row_sum_get(red[par], 1) * inv_h;
    const float c2a = row_sum_get(red[par], 2) * inv_h, c2b = row_sum_get(red[par], 3) * inv_h;
    float4* dxr = (float4*)(dx + (long)row * h);
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int i = j * 256 + tid;
      if (i >= nv) continue;
      float4 o = MMPT_LN_PREFETCH ? dr[j] : drr ? drr[i] : zero4();
      dx_add(o, rs, g1[j], xh[j], c1a, c1b);
      if (two) dx_add(o, rs, g2[j], xh[j], c2a, c2b);
      dxr[i] = o;
      if (dxb != nullptr) st_dx_bf16(dxb + (long)row * h, i, o, want_dsum, as[j]);
    }
  }
  float4* out = (float4*)(partials + (long)blockIdx.x * 5 * h);
#pragma unroll
  for (int j = 0; j < PT; ++j) {
    const int i = j * 256 + tid;
    if (i >= nv) continue;
    out[i] = aw1[j];
    if (!RMS) out[nv + i] = ab1[j];
    if (two) {
      out[2 * nv + i] = aw2[j];
      out[3 * nv + i] = ab2[j];
    }
    if (want_dsum) out[4 * nv + i] = as[j];
  }
}

// K18: the classification head's LayerNorm backward (ViTForImageClassification reads only
// the CLS row of vit.layernorm's output).  One launch: workgroups [0, nblk) run the row pieces
// of ln_bwd_rows_kernel on the CLS rows (x / dx row b*tokens, dy row b) and leave the same
// [block][5][h] partials; the workgroups after them store +0 over every other row of dx and
// dx_bf16 (16-B vector stores), so the dense gradient of the residual stream and its bf16 copy
// come out of one pass with no memset before it.
#ifndef MMPT_CLS_ZERO_BLOCKS
#define MMPT_CLS_ZERO_BLOCKS 2048
#endif
template <int PT>
__global__ __launch_bounds__(256) void cls_ln_bwd_kernel(
    int batch, int tokens, int h, int nblk, const float* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ rstd, const bf16_t* __restrict__ dy1,
    long ld_dy, const float* __restrict__ w1, float* dx, bf16_t* __restrict__ dxb, int want_dsum,
    float* __restrict__ partials) {
  __shared__ float red[2][4][2];
  const int tid = threadIdx.x;
  const int nv = h >> 2;
  if ((int)blockIdx.x >= nblk) {  // the zero rows: every row r with r % tokens != 0
    const long total = (long)batch * tokens;
    const int nz = gridDim.x - nblk, n8 = h >> 3;
    const uint4 z8 = make_uint4(0u, 0u, 0u, 0u);
    for (long r = blockIdx.x - nblk; r < total; r += nz) {
      if (r % tokens == 0) continue;
      float4* d4 = (float4*)(dx + r * h);
      for (int i = tid; i < nv; i += 256) d4[i] = zero4();
      if (dxb != nullptr) {
        uint4* d8 = (uint4*)(dxb + r * h);
        for (int i = tid; i < n8; i += 256) d8[i] = z8;
      }
    }
    return;
  }
  float4 aw1[PT], ab1[PT], as[PT];
  float4 ww1[PT];
#pragma unroll
  for (int j = 0; j < PT; ++j) {
    aw1[j] = ab1[j] = as[j] = zero4();
    const int i = j * 256 + tid;
    ww1[j] = i < nv ? ((const float4*)w1)[i] : zero4();
  }
  int par = 0;
  for (int row = blockIdx.x; row < batch; row += nblk, par ^= 1) {
    const float mu = mean[row], rs = rstd[row];
    const long xrow = (long)row * tokens * h;
    const float4* xr = (const float4*)(x + xrow);
    float4 xh[PT], g1[PT];
    float s1a = 0.f, s1b = 0.f;
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int i = j * 256 + tid;
      xh[j] = g1[j] = zero4();
      if (i >= nv) continue;
      xh[j] = xhat4(xr[i], mu, rs);
      bwd_accum(xh[j], ld_bf16x4(dy1 + (long)row * ld_dy + i * 4), ww1[j], g1[j], s1a, s1b,
                aw1[j], ab1[j]);
    }
    row_sums_put(red[par], 0, s1a, s1b);
    __syncthreads();
    const float inv_h = 1.0f / (float)h;
    const float c1a = row_sum_get(red[par], 0) * inv_h, c1b = row_sum_get(red[par], 1) * inv_h;
    float4* dxr = (float4*)(dx + xrow);
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int i = j * 256 + tid;
      if (i >= nv) continue;
      float4 o = zero4();
      dx_add(o, rs, g1[j], xh[j], c1a, c1b);
      dxr[i] = o;
      if (dxb != nullptr) st_dx_bf16(dxb + xrow, i, o, want_dsum, as[j]);
    }
  }
  float4* out = (float4*)(partials + (long)blockIdx.x * 5 * h);
#pragma unroll
  for (int j = 0; j < PT; ++j) {
    const int i = j * 256 + tid;
    if (i >= nv) continue;
    out[i] = aw1[j];
    out[nv + i] = ab1[j];
    if (want_dsum) out[4 * nv + i] = as[j];
  }
}

// blocks of the wave-per-row backward / of the workgroup-per-row backward
int bwd_blocks(int64_t rows) {
  return (int)std::min<int64_t>(LN_BWD_BLOCKS, (rows + LN_WAVES - 1) / LN_WAVES);
}
int rows_blocks(int64_t rows) { return (int)std::min<int64_t>(LNR_BLOCKS, rows); }

// ln_fwd_kernel over `rows` rows; the persistent form when allowed and the rows need more
// than MMPT_LN_FWD_BLOCKS workgroups (it writes y at leading dimension h)
template <bool MAY_PERSIST>
void launch_fwd(int mj, int64_t rows, int64_t h, float eps, const float* x, long ldx,
                const float* w1, const float* b1, bf16_t* y1, const float* w2, const float* b2,
                bf16_t* y2, float* mean, float* rstd, long ldy, hipStream_t s) {
  const int nblk = (int)((rows + LN_WAVES - 1) / LN_WAVES);
  dispatch_maxj(mj, [&](auto J) {
    constexpr int MJ = decltype(J)::value;
    if (MAY_PERSIST && MMPT_LN_FWD_PERSIST && nblk > MMPT_LN_FWD_BLOCKS) {
      const size_t lds = (size_t)(y2 != nullptr ? 4 : 2) * h * sizeof(float);
      ln_fwd_kernel<MJ, MAY_PERSIST><<<MMPT_LN_FWD_BLOCKS, 256, lds, s>>>(
          (int)rows, (int)h, eps, x, ldx, w1, b1, y1, w2, b2, y2, mean, rstd, (long)h);
    } else {
      ln_fwd_kernel<MJ, false><<<nblk, 256, 0, s>>>((int)rows, (int)h, eps, x, ldx, w1, b1, y1,
                                                    w2, b2, y2, mean, rstd, ldy);
    }
  });
}

// ln_bwd_kernel + its reduce (dw1 … db2 nullable)
template <bool DY32>
int launch_bwd(const char* what, const char* what_reduce, int mj, int64_t rows, int64_t h,
               const float* x, long ldx, const float* mean, const float* rstd, const bf16_t* dy1,
               const float* w1, const bf16_t* dy2, const float* w2, const float* dresid,
               float* dx, float* dw1, float* db1, float* dw2, float* db2, float* part,
               hipStream_t s) {
  const int nblk = bwd_blocks(rows);
  dispatch_maxj(mj, [&](auto J) {
    ln_bwd_kernel<decltype(J)::value, DY32><<<nblk, 256, 0, s>>>(
        (int)rows, (int)h, x, ldx, mean, rstd, dy1, w1, dy2, w2, dresid, dx, part);
  });
  int rc = check_launch(what);
  if (rc) return rc;
  if (dw1 || db1 || dw2 || db2) {
    dim3 rg((unsigned)((h + 63) / 64), dy2 ? 4u : 2u);
    partials_reduce<<<rg, 256, 0, s>>>(nblk, (int)h, 4, part, dw1, db1, dy2 ? dw2 : nullptr,
                                       dy2 ? db2 : nullptr, nullptr, -1, nullptr);
    rc = check_launch(what_reduce);
  }
  return rc;
}

// the reduce of the [block][5][h] partials, over the first nq quantities
int reduce_rows(const char* what, int nblk, int64_t h, unsigned nq, const float* part, float* dw1,
                float* db1, float* dw2, float* db2, float* dsum, float* dsum2, hipStream_t s) {
  dim3 rg((unsigned)((h + 63) / 64), nq);
  partials_reduce<<<rg, 256, 0, s>>>(nblk, (int)h, 5, part, dw1, db1, dw2, db2, dsum, 4, dsum2);
  return check_launch(what);
}

}  // namespace
}  // namespace mmpt

using namespace mmpt;

extern "C" int mmpt_layernorm_fwd(int64_t rows, int64_t h, float eps, const float* x,
                                  int64_t ldx, const float* w1, const float* b1, void* y1,
                                  const float* w2, const float* b2, void* y2, float* mean,
                                  float* rstd, void* stream) {
  MMPT_REQUIRE(rows > 0 && h > 0 && h % 4 == 0 && ldx % 4 == 0, "layernorm_fwd: bad shape");
  MMPT_REQUIRE(x && w1 && b1 && y1 && mean && rstd, "layernorm_fwd: null pointer");
  MMPT_REQUIRE(y2 == nullptr || (w2 && b2), "layernorm_fwd: y2 needs w2/b2");
  const int mj = pick_maxj(h);
  MMPT_REQUIRE(mj > 0, "layernorm_fwd: h=%lld too large", (long long)h);
  launch_fwd<true>(mj, rows, h, eps, x, ldx, w1, b1, (bf16_t*)y1, w2, b2, (bf16_t*)y2, mean,
                          rstd, h, (hipStream_t)stream);
  return check_launch("layernorm_fwd");
}

extern "C" int64_t mmpt_layernorm_bwd_workspace_bytes(int64_t rows, int64_t h) {
  return bwd_blocks(rows) * 4 * h * (int64_t)sizeof(float);
}

extern "C" int mmpt_layernorm_bwd(int64_t rows, int64_t h, const float* x, int64_t ldx,
                                  const float* mean, const float* rstd, const void* dy1,
                                  const float* w1, const void* dy2, const float* w2,
                                  const float* dresid, float* dx, float* dw1, float* db1,
                                  float* dw2, float* db2, void* workspace, void* stream) {
  MMPT_REQUIRE(rows > 0 && h > 0 && h % 4 == 0 && ldx % 4 == 0, "layernorm_bwd: bad shape");
  MMPT_REQUIRE(x && mean && rstd && dy1 && w1 && dx && workspace, "layernorm_bwd: null pointer");
  MMPT_REQUIRE(dy2 == nullptr || w2, "layernorm_bwd: dy2 needs w2");
  const int mj = pick_maxj(h);
  MMPT_REQUIRE(mj > 0, "layernorm_bwd: h=%lld too large", (long long)h);
  return launch_bwd<false>("layernorm_bwd", "layernorm_bwd_reduce", mj, rows, h, x, ldx, mean,
                           rstd, (const bf16_t*)dy1, w1, (const bf16_t*)dy2, w2, dresid, dx, dw1,
                           db1, dw2, db2, (float*)workspace, (hipStream_t)stream);
}

extern "C" int64_t mmpt_layernorm_bwd_ex_workspace_bytes(int64_t rows, int64_t h) {
  return rows_blocks(rows) * 5 * h * (int64_t)sizeof(float);
}

extern "C" int mmpt_layernorm_bwd_ex(int64_t rows, int64_t h, const float* x, int64_t ldx,
                                     const float* mean, const float* rstd, const void* dy1,
                                     const float* w1, const void* dy2, const float* w2,
                                     const float* dresid, float* dx, void* dx_bf16, float* dw1,
                                     float* db1, float* dw2, float* db2, float* dsum,
                                     float* dsum2, void* workspace, void* stream) {
  MMPT_REQUIRE(rows > 0 && h > 0 && h % 4 == 0 && ldx % 4 == 0, "layernorm_bwd_ex: bad shape");
  MMPT_REQUIRE(x && mean && rstd && dy1 && w1 && dx && workspace, "layernorm_bwd_ex: null pointer");
  MMPT_REQUIRE(dy2 == nullptr || w2, "layernorm_bwd_ex: dy2 needs w2");
  MMPT_REQUIRE(dsum == nullptr || dx_bf16, "layernorm_bwd_ex: dsum needs dx_bf16");
  MMPT_REQUIRE(dsum2 == nullptr || dsum, "layernorm_bwd_ex: dsum2 needs dsum");
  const int pt = pick_pt(h);
  MMPT_REQUIRE(pt > 0, "layernorm_bwd_ex: h=%lld too large", (long long)h);
  const int nblk = rows_blocks(rows);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  dispatch_pt(pt, [&](auto PT) {
    ln_bwd_rows_kernel<decltype(PT)::value, false><<<nblk, 256, 0, s>>>(
        (int)rows, (int)h, x, ldx, mean, rstd, (const bf16_t*)dy1, w1, (const bf16_t*)dy2, w2,
        dresid, dx, (bf16_t*)dx_bf16, dsum != nullptr, part);
  });
  int rc = check_launch("layernorm_bwd_ex");
  if (rc) return rc;
  return reduce_rows("layernorm_bwd_ex_reduce", nblk, h, 5u, part, dw1, db1, dy2 ? dw2 : nullptr,
                     dy2 ? db2 : nullptr, dsum, dsum2, s);
}

extern "C" int mmpt_layernorm_f32_fwd(int64_t rows, int64_t h, float eps, const float* x,
                                      const float* w, const float* b, float* y, float* mean,
                                      float* rstd, void* stream) {
  MMPT_REQUIRE(rows > 0 && h > 0 && h % 4 == 0, "layernorm_f32_fwd: bad shape");
  MMPT_REQUIRE(x && w && b && y && mean && rstd, "layernorm_f32_fwd: null pointer");
  const int mj = pick_maxj(h);
  MMPT_REQUIRE(mj > 0, "layernorm_f32_fwd: h=%lld too large", (long long)h);
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = (unsigned)((rows + LN_WAVES - 1) / LN_WAVES);
  dispatch_maxj(mj, [&](auto J) {
    ln_fwd32_kernel<decltype(J)::value><<<g, 256, 0, s>>>((int)rows, (int)h, eps, x, w, b, y, mean,
                                                          rstd);
  });
  return check_launch("layernorm_f32_fwd");
}

extern "C" int mmpt_layernorm_f32_bwd(int64_t rows, int64_t h, const float* x, const float* mean,
                                      const float* rstd, const float* dy, const float* w,
                                      float* dx, float* dw, float* db, void* workspace,
                                      void* stream) {
  MMPT_REQUIRE(rows > 0 && h > 0 && h % 4 == 0, "layernorm_f32_bwd: bad shape");
  MMPT_REQUIRE(x && mean && rstd && dy && w && dx && workspace, "layernorm_f32_bwd: null pointer");
  const int mj = pick_maxj(h);
  MMPT_REQUIRE(mj > 0, "layernorm_f32_bwd: h=%lld too large", (long long)h);
  return launch_bwd<true>("layernorm_f32_bwd", "layernorm_f32_bwd_reduce", mj, rows, h, x, h, mean,
                          rstd, (const bf16_t*)(const void*)dy, w, nullptr, nullptr, nullptr, dx,
                          dw, db, nullptr, nullptr, (float*)workspace, (hipStream_t)stream);
}

// ---- RMSNorm (Llama): forward / backward over the same kernels (RMS instantiation) ----
extern "C" int mmpt_rmsnorm_fwd(int64_t rows, int64_t h, float eps, const float* x, int64_t ldx,
                                const float* w, void* y, float* rstd, void* stream) {
  MMPT_REQUIRE(rows > 0 && h > 0 && h % 4 == 0 && ldx % 4 == 0, "rmsnorm_fwd: bad shape");
  MMPT_REQUIRE(x && w && y && rstd, "rmsnorm_fwd: null pointer");
  const int mj = pick_maxj(h);
  MMPT_REQUIRE(mj > 0, "rmsnorm_fwd: h=%lld too large", (long long)h);
  const unsigned g = (unsigned)((rows + LN_WAVES - 1) / LN_WAVES);
  dispatch_maxj(mj, [&](auto J) {
    rms_fwd_kernel<decltype(J)::value><<<g, 256, 0, (hipStream_t)stream>>>(
        (int)rows, (int)h, eps, x, ldx, w, (bf16_t*)y, rstd);
  });
  return check_launch("rmsnorm_fwd");
}

extern "C" int64_t mmpt_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t h) {
  return mmpt_layernorm_bwd_ex_workspace_bytes(rows, h);
}

extern "C" int mmpt_rmsnorm_bwd(int64_t rows, int64_t h, const float* x, int64_t ldx,
                                const float* rstd, const void* dy, const float* w,
                                const float* dresid, float* dx, void* dx_bf16, float* dw,
                                void* workspace, void* stream) {
  MMPT_REQUIRE(rows > 0 && h > 0 && h % 4 == 0 && ldx % 4 == 0, "rmsnorm_bwd: bad shape");
  MMPT_REQUIRE(x && rstd && dy && w && dx && workspace, "rmsnorm_bwd: null pointer");
  const int pt = pick_pt(h);
  MMPT_REQUIRE(pt > 0, "rmsnorm_bwd: h=%lld too large", (long long)h);
  const int nblk = rows_blocks(rows);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  dispatch_pt(pt, [&](auto PT) {
    ln_bwd_rows_kernel<decltype(PT)::value, true><<<nblk, 256, 0, s>>>(
        (int)rows, (int)h, x, ldx, nullptr, rstd, (const bf16_t*)dy, w, nullptr, nullptr, dresid,
        dx, (bf16_t*)dx_bf16, 0, part);
  });
  int rc = check_launch("rmsnorm_bwd");
  if (rc || dw == nullptr) return rc;
  return reduce_rows("rmsnorm_bwd_reduce", nblk, h, 1u, part, dw, nullptr, nullptr, nullptr,
                     nullptr, nullptr, s);
}

// ---- K18: classification head (final LayerNorm on the CLS rows) ----
extern "C" int mmpt_cls_ln_fwd(int64_t batch, int64_t tokens, int64_t h, float eps, const float* x,
                               const float* w, const float* b, void* y, int64_t ld_y, float* mean,
                               float* rstd, void* stream) {
  MMPT_REQUIRE(batch > 0 && tokens > 0 && h > 0 && h % 8 == 0, "cls_ln_fwd: bad shape");
  MMPT_REQUIRE(batch * tokens < (int64_t)1 << 31, "cls_ln_fwd: batch*tokens too large");
  MMPT_REQUIRE(ld_y >= h && ld_y % 8 == 0, "cls_ln_fwd: ld_y must be a multiple of 8 and >= h");
  MMPT_REQUIRE(x && w && b && y && mean && rstd, "cls_ln_fwd: null pointer");
  MMPT_REQUIRE(al16(x) && al16(w) && al16(b) && al16(y),
               "cls_ln_fwd: pointers must be 16-byte aligned");
  const int mj = pick_maxj(h);
  MMPT_REQUIRE(mj > 0, "cls_ln_fwd: h=%lld too large", (long long)h);
  launch_fwd<false>(mj, batch, h, eps, x, (long)(tokens * h), w, b, (bf16_t*)y, nullptr,
                           nullptr, nullptr, mean, rstd, (long)ld_y, (hipStream_t)stream);
  return check_launch("cls_ln_fwd");
}

extern "C" int64_t mmpt_cls_ln_bwd_workspace_bytes(int64_t batch, int64_t h) {
  return mmpt_layernorm_bwd_ex_workspace_bytes(batch, h);
}

extern "C" int mmpt_cls_ln_bwd(int64_t batch, int64_t tokens, int64_t h, const float* x,
                               const float* mean, const float* rstd, const void* dy, int64_t ld_dy,
                               const float* w, float* dx, void* dx_bf16, float* dw, float* db,
                               float* dsum, void* workspace, void* stream) {
  MMPT_REQUIRE(batch > 0 && tokens > 0 && h > 0 && h % 8 == 0, "cls_ln_bwd: bad shape");
  MMPT_REQUIRE(batch * tokens < (int64_t)1 << 31, "cls_ln_bwd: batch*tokens too large");
  MMPT_REQUIRE(ld_dy >= h && ld_dy % 8 == 0, "cls_ln_bwd: ld_dy must be a multiple of 8 and >= h");
  MMPT_REQUIRE(x && mean && rstd && dy && w && dx && workspace, "cls_ln_bwd: null pointer");
  MMPT_REQUIRE(dsum == nullptr || dx_bf16, "cls_ln_bwd: dsum needs dx_bf16");
  MMPT_REQUIRE(al16(x) && al16(dy) && al16(w) && al16(dx) && al16(dx_bf16) && al16(workspace),
               "cls_ln_bwd: pointers must be 16-byte aligned");
  const int pt = pick_pt(h);
  MMPT_REQUIRE(pt > 0, "cls_ln_bwd: h=%lld too large", (long long)h);
  const int nblk = rows_blocks(batch);
  const int nzero = (int)std::min<int64_t>(MMPT_CLS_ZERO_BLOCKS, batch * (tokens - 1));
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  dispatch_pt(pt, [&](auto PT) {
    cls_ln_bwd_kernel<decltype(PT)::value><<<nblk + nzero, 256, 0, s>>>(
        (int)batch, (int)tokens, (int)h, nblk, x, mean, rstd, (const bf16_t*)dy, (long)ld_dy, w,
        dx, (bf16_t*)dx_bf16, dsum != nullptr, part);
  });
  int rc = check_launch("cls_ln_bwd");
  if (rc) return rc;
  return reduce_rows("cls_ln_bwd_reduce", nblk, h, 5u, part, dw, db, nullptr, nullptr, dsum,
                     nullptr, s);
}
