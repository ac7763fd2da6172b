// The row-normalisation pieces that layernorm.hip (K4, K18) and postln.hip (K20) share: each
// piece of arithmetic is written here once, so every kernel that normalises a row rounds alike.
//   forward:  ld_row, row_stats (mean, rstd of a row held in registers), xhat4, affine4,
//             st_norm_bf16x4
//   backward: bwd_accum (g, the two row sums, the dγ / dβ accumulators), row_sums_put /
//             row_sum_get (the wave -> 4-wave exchange of the workgroup-per-row kernels), dx_add
//   partials_reduce: Σ over blocks of the per-block dγ / dβ / bias-gradient partial rows
//   host:     pick_maxj, dispatch_maxj, dispatch_pt
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>

#include "common.h"

namespace mmpt {
namespace {

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// ---- forward: one wave per row, float4 j * 64 + lane of the row in v[j] (+0 past the row) ----
template <int MAXJ>
__device__ __forceinline__ void ld_row(float4* v, const float4* xr, int lane, int nv) {
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int i = j * 64 + lane;
    v[j] = i < nv ? xr[i] : zero4();
  }
}

// fp32 statistics: mean = Σx / h, rstd = 1 / sqrt(Σ(x − mean)² / h + eps), both sums pairwise
// per float4 and a butterfly across the wave.  RMS: mean = 0, so rstd = 1 / sqrt(Σx² / h + eps).
template <int MAXJ, bool RMS>
__device__ __forceinline__ void row_stats(const float4* v, int lane, int nv, int h, float eps,
                                          float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
  mean = RMS ? 0.f : wave_sum(s) / (float)h;
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    if (j * 64 + lane < nv) {
      const float a = v[j].x - mean, b = v[j].y - mean, c = v[j].z - mean, d = v[j].w - mean;
      ss += (a * a + b * b) + (c * c + d * d);
    }
  }
  rstd = 1.0f / sqrtf(wave_sum(ss) / (float)h + eps);
}

// x̂ = (x − μ) · rstd
__device__ __forceinline__ float4 xhat4(const float4 x, float mu, float rs) {
  return make_float4((x.x - mu) * rs, (x.y - mu) * rs, (x.z - mu) * rs, (x.w - mu) * rs);
}
// y = x̂ · γ + β
__device__ __forceinline__ float4 affine4(const float4 xh, const float4 g, const float4 b) {
  return make_float4(xh.x * g.x + b.x, xh.y * g.y + b.y, xh.z * g.z + b.z, xh.w * g.w + b.w);
}
__device__ __forceinline__ void st_norm_bf16x4(bf16_t* row, int i, const float4 xh, const float4 g,
                                               const float4 b) {
  const float4 y = affine4(xh, g, b);
  ((uint2*)row)[i] = make_uint2(pack2(y.x, y.y), pack2(y.z, y.w));
}

// ---- backward ----
// One float4 of one LayerNorm of a row: g = dy · γ, the row sums Σ g·x̂ and Σ g, and the
// dγ += dy · x̂, dβ += dy accumulators.
__device__ __forceinline__ void bwd_accum(const float4 xh, const float4 d, const float4 w,
                                          float4& g, float& sa, float& sb, float4& aw,
                                          float4& ab) {
  g = make_float4(d.x * w.x, d.y * w.y, d.z * w.z, d.w * w.w);
  sa += (g.x * xh.x + g.y * xh.y) + (g.z * xh.z + g.w * xh.w);
  sb += (g.x + g.y) + (g.z + g.w);
  aw.x += d.x * xh.x; aw.y += d.y * xh.y;
  aw.z += d.z * xh.z; aw.w += d.w * xh.w;
  ab.x += d.x; ab.y += d.y; ab.z += d.z; ab.w += d.w;
}

// dx += rstd · (g − x̂ · ca − cb), ca = mean(g·x̂), cb = mean(g)
__device__ __forceinline__ void dx_add(float4& o, float rs, const float4 g, const float4 xh,
                                       float ca, float cb) {
  o.x += rs * (g.x - xh.x * ca - cb);
  o.y += rs * (g.y - xh.y * ca - cb);
  o.z += rs * (g.z - xh.z * ca - cb);
  o.w += rs * (g.w - xh.w * ca - cb);
}

// The row sums of a 256-thread workgroup, in two steps around the row's one barrier: each wave
// puts its wave_sum pair at red[par][wave][k], k + 1 (`red` is double-buffered by row parity);
// after __syncthreads() every thread takes (w0 + w1) + (w2 + w3).
template <int NS>
__device__ __forceinline__ void row_sums_put(float (&red)[4][NS], int k, float& a, float& b) {
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][k] = a;
    red[threadIdx.x >> 6][k + 1] = b;
  }
}
template <int NS>
__device__ __forceinline__ float row_sum_get(const float (&red)[4][NS], int k) {
  return (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// Σ over blocks of partials[b][q][c] (nq quantities per block) -> d_q[c] (+=, skipped when
// null): one workgroup per (64 columns, quantity); its 4 waves take blocks wave, wave + 4, …,
// then (r0 + r1) + (r2 + r3).  Quantity qbf (-1: none) is a bias gradient: rounded to bf16 first
// (autocast's grad dtype) and also added to dbf2 when that is given.
__global__ __launch_bounds__(256) void partials_reduce(int nblk, int h, int nq,
                                                       const float* __restrict__ partials,
                                                       float* d0, float* d1, float* d2, float* d3,
                                                       float* d4, int qbf, float* dbf2) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.y, c = blockIdx.x * 64 + lane;
  float* dst = q == 0 ? d0 : q == 1 ? d1 : q == 2 ? d2 : q == 3 ? d3 : d4;
  if (dst == nullptr) return;  // uniform per workgroup
  float s = 0.f;
  if (c < h)
#pragma unroll 8
    for (int b = wave; b < nblk; b += 4) s += partials[((long)b * nq + q) * h + c];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < h) {
    float v = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    if (q == qbf) {
      v = round_bf(v);
      if (dbf2 != nullptr) dbf2[c] += v;
    }
    dst[c] += v;
  }
}

// ---- host dispatch ----
// float4 per lane of the wave-per-row kernels (64 lanes): 1, 2, 4, 8, 12 or 16; -1: h too large
inline int pick_maxj(int64_t h) {
  const int64_t per = (h / 4 + 63) / 64;
  return per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : per <= 8 ? 8 : per <= 12 ? 12 : per <= 16 ? 16 : -1;
}
// float4 per thread of the workgroup-per-row kernels (256 threads): 1, 2 or 4 (h <= 4096)
inline int pick_pt(int64_t h) {
  const int64_t per = (h / 4 + 255) / 256;
  return per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : -1;
}

// f(std::integral_constant<int, V>{}) for the V of Vs... that equals v
template <int... Vs, class F>
inline void dispatch_int(int v, std::integer_sequence<int, Vs...>, F&& f) {
  (void)((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
template <class F>
inline void dispatch_maxj(int mj, F&& f) {
  dispatch_int(mj, std::integer_sequence<int, 1, 2, 4, 8, 12, 16>{}, f);
}
template <class F>
inline void dispatch_pt(int pt, F&& f) {
  dispatch_int(pt, std::integer_sequence<int, 1, 2, 4>{}, f);
}

}  // namespace
}  // namespace mmpt
