// K16  hidden dropout (nn.Dropout at GPTNeoX's emb_dropout / post_attention_dropout /
// post_mlp_dropout, tf:models/gpt_neox/modeling_gpt_neox.py, and at ViTEmbeddings.dropout /
// ViTSelfOutput.dropout / ViTOutput.dropout, tf:models/vit/modeling_vit.py) with the masks
// never stored: every kernel recomputes the keep bit of logical element e = row*h + col from a
// counter-based generator (philox.h), so the backward, an activation-checkpoint recompute and
// the test hook all see the forward's mask.
//
// One thread handles 8 consecutive elements of a row (h % 8 == 0): two Philox calls, one 16-B
// bf16 access (two for fp32).  A workgroup is 256 threads laid out as (256 / W) rows x W column
// octets, W = the power of two covering min(h / 8, 256); grid-stride over rows.  No atomics, no
// LDS; an output may alias its input (each thread reads its 8 elements before it writes them).
#include "common.h"
#include "philox.h"

namespace mmpt {
namespace {

struct DropArgs {
  uint32_t thr;   // keep iff word >= thr
  float scale;    // 1 / (1 - p)
  uint64_t seed;
};

// keep bits (bit j: element 8*o + j) of the octet o of a site
__device__ __forceinline__ uint32_t keep8(uint64_t o, uint64_t site, const DropArgs& a) {
  const philox4 lo = dropout_words(2 * o, site, a.seed), hi = dropout_words(2 * o + 1, site, a.seed);
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    m |= (uint32_t)(lo.w[j] >= a.thr) << j;
    m |= (uint32_t)(hi.w[j] >= a.thr) << (4 + j);
  }
  return m;
}

// drop of one bf16 element: bf16(f32(x) * scale) (one rounding) or +0
__device__ __forceinline__ bf16_t drop_bf(bf16_t x, bool keep, float scale) {
  return keep ? f2bf(bf2f(x) * scale) : (bf16_t)0;
}

__device__ __forceinline__ v8s drop8(v8s x, uint32_t m, float scale) {
  v8s r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (short)drop_bf((bf16_t)x[j], (m >> j) & 1, scale);
  return r;
}

// row / column-octet walk shared by the kernels: body(row, c8) for every octet of the matrix
#define MMPT_DROP_WALK(rows, h8, wshift)                                                 \
  const int W_ = 1 << (wshift);                                                          \
  const long rb_ = 256 >> (wshift);                                                      \
  const int c0_ = threadIdx.x & (W_ - 1);                                                \
  for (long row = (long)blockIdx.x * rb_ + (threadIdx.x >> (wshift)); row < (rows);      \
       row += (long)gridDim.x * rb_)                                                     \
    for (int c8 = c0_; c8 < (h8); c8 += W_)

__global__ __launch_bounds__(256) void dropout_bf16_kernel(long rows, int h8, int wshift,
                                                           const bf16_t* src, long ld_src,
                                                           bf16_t* dst, long ld_dst, uint64_t site,
                                                           DropArgs a) {
  MMPT_DROP_WALK(rows, h8, wshift) {
    const v8s x = *(const v8s*)(src + row * ld_src + 8L * c8);
    const uint32_t m = keep8((uint64_t)row * h8 + c8, site, a);
    *(v8s*)(dst + row * ld_dst + 8L * c8) = drop8(x, m, a.scale);
  }
}

__global__ __launch_bounds__(256) void dropout_f32_kernel(long rows, int h8, int wshift,
                                                          const float* src, float* dst,
                                                          uint64_t site, DropArgs a) {
  MMPT_DROP_WALK(rows, h8, wshift) {
    const uint64_t o = (uint64_t)row * h8 + c8;
    const v4f x0 = *(const v4f*)(src + 8 * o), x1 = *(const v4f*)(src + 8 * o + 4);
    const uint32_t m = keep8(o, site, a);
    v4f y0, y1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      y0[j] = (m >> j) & 1 ? x0[j] * a.scale : 0.f;
      y1[j] = (m >> (4 + j)) & 1 ? x1[j] * a.scale : 0.f;
    }
    *(v4f*)(dst + 8 * o) = y0;
    *(v4f*)(dst + 8 * o + 4) = y1;
  }
}

// out = resid + f32(v); v = drop(y), or bf16(drop(y2) + drop(y)): the rounding order of
// MMPT_EPI_F32_RESID (v = bf16(branch); v = bf16(v + aux); C = resid + v)
template <bool TWO>
__global__ __launch_bounds__(256) void dropout_add_f32_kernel(
    long rows, int h8, int wshift, const bf16_t* y, long ld_y, uint64_t site_y, const bf16_t* y2,
    long ld_y2, uint64_t site_y2, const float* resid, float* out, DropArgs a) {
  MMPT_DROP_WALK(rows, h8, wshift) {
    const uint64_t o = (uint64_t)row * h8 + c8;
    v8s v = drop8(*(const v8s*)(y + row * ld_y + 8L * c8), keep8(o, site_y, a), a.scale);
    if (TWO) {
      const v8s u = drop8(*(const v8s*)(y2 + row * ld_y2 + 8L * c8), keep8(o, site_y2, a), a.scale);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (short)f2bf(bf2f((bf16_t)u[j]) + bf2f((bf16_t)v[j]));
    }
    const v4f r0 = *(const v4f*)(resid + 8 * o), r1 = *(const v4f*)(resid + 8 * o + 4);
    v4f o0, o1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o0[j] = r0[j] + bf2f((bf16_t)v[j]);
      o1[j] = r1[j] + bf2f((bf16_t)v[4 + j]);
    }
    *(v4f*)(out + 8 * o) = o0;
    *(v4f*)(out + 8 * o + 4) = o1;
  }
}

// keep[e] = 1 / 0 for e < n: one Philox call (4 elements) per thread
__global__ __launch_bounds__(256) void dropout_mask_kernel(long n, uint64_t site, uint8_t* keep,
                                                           DropArgs a) {
  const long n4 = (n + 3) >> 2;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long)gridDim.x * 256) {
    const philox4 w = dropout_words((uint64_t)q, site, a.seed);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * q + j < n) keep[4 * q + j] = (uint8_t)(w.w[j] >= a.thr);
  }
}

// 8 workgroups (32 waves) per CU
int64_t grid_cap() {
  static const int64_t cap = (int64_t)cu_slots(nullptr) * 8;
  return cap;
}

struct Launch {
  unsigned grid;
  int h8, wshift;
};

// W = the power of two >= min(h8, 256); one workgroup covers 256 / W rows per pass
Launch plan(int64_t rows, int64_t h) {
  Launch l;
  l.h8 = (int)(h / 8);
  l.wshift = 0;
  while ((1 << l.wshift) < l.h8 && l.wshift < 8) ++l.wshift;
  const int64_t rb = 256 >> l.wshift;
  int64_t g = (rows + rb - 1) / rb;
  const int64_t cap = grid_cap();
  l.grid = (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
  return l;
}

}  // namespace
}  // namespace mmpt

using namespace mmpt;

#define MMPT_DROP_COMMON(what)                                                                  \
  MMPT_REQUIRE(p >= 0.0 && p < 1.0, what ": p must lie in [0, 1), got %g", p);                  \
  MMPT_REQUIRE(rows >= 0 && h > 0 && h % 8 == 0, what ": h must be a positive multiple of 8 "   \
               "(rows %lld, h %lld)", (long long)rows, (long long)h);                           \
  MMPT_REQUIRE(h / 8 <= INT32_MAX && rows <= (INT64_MAX >> 1) / h, what ": sizes out of range"); \
  const DropArgs a = {dropout_threshold(p), dropout_scale(p), seed}

extern "C" int mmpt_dropout_bf16(int64_t rows, int64_t h, const void* src, int64_t ld_src,
                                 void* dst, int64_t ld_dst, double p, uint64_t seed, uint64_t site,
                                 void* stream) {
  MMPT_DROP_COMMON("dropout_bf16");
  MMPT_REQUIRE(src && dst, "dropout_bf16: null pointer");
  MMPT_REQUIRE(ld_src >= h && ld_dst >= h && ld_src % 8 == 0 && ld_dst % 8 == 0,
               "dropout_bf16: leading dims must be multiples of 8 and >= h");
  MMPT_REQUIRE(al16(src) && al16(dst), "dropout_bf16: pointers must be 16-B aligned");
  if (rows == 0) return MMPT_OK;
  const Launch l = plan(rows, h);
  dropout_bf16_kernel<<<l.grid, 256, 0, (hipStream_t)stream>>>(
      rows, l.h8, l.wshift, (const bf16_t*)src, ld_src, (bf16_t*)dst, ld_dst, site, a);
  return check_launch("dropout_bf16");
}

extern "C" int mmpt_dropout_f32(int64_t rows, int64_t h, const float* src, float* dst, double p,
                                uint64_t seed, uint64_t site, void* stream) {
  MMPT_DROP_COMMON("dropout_f32");
  MMPT_REQUIRE(src && dst, "dropout_f32: null pointer");
  MMPT_REQUIRE(al16(src) && al16(dst), "dropout_f32: pointers must be 16-B aligned");
  if (rows == 0) return MMPT_OK;
  const Launch l = plan(rows, h);
  dropout_f32_kernel<<<l.grid, 256, 0, (hipStream_t)stream>>>(rows, l.h8, l.wshift, src, dst, site,
                                                              a);
  return check_launch("dropout_f32");
}

extern "C" int mmpt_dropout_add_f32(int64_t rows, int64_t h, const void* y, int64_t ld_y,
                                    uint64_t site_y, const void* y2, int64_t ld_y2,
                                    uint64_t site_y2, const float* resid, float* out, double p,
                                    uint64_t seed, void* stream) {
  MMPT_DROP_COMMON("dropout_add_f32");
  MMPT_REQUIRE(y && resid && out, "dropout_add_f32: null pointer");
  MMPT_REQUIRE(ld_y >= h && ld_y % 8 == 0 && (!y2 || (ld_y2 >= h && ld_y2 % 8 == 0)),
               "dropout_add_f32: leading dims must be multiples of 8 and >= h");
  MMPT_REQUIRE(al16(y) && al16(y2) && al16(resid) && al16(out),
               "dropout_add_f32: pointers must be 16-B aligned");
  if (rows == 0) return MMPT_OK;
  const Launch l = plan(rows, h);
  if (y2)
    dropout_add_f32_kernel<true><<<l.grid, 256, 0, (hipStream_t)stream>>>(
        rows, l.h8, l.wshift, (const bf16_t*)y, ld_y, site_y, (const bf16_t*)y2, ld_y2, site_y2,
        resid, out, a);
  else
    dropout_add_f32_kernel<false><<<l.grid, 256, 0, (hipStream_t)stream>>>(
        rows, l.h8, l.wshift, (const bf16_t*)y, ld_y, site_y, nullptr, 0, 0, resid, out, a);
  return check_launch("dropout_add_f32");
}

extern "C" int mmpt_dropout_mask(int64_t n, double p, uint64_t seed, uint64_t site, uint8_t* keep,
                                 void* stream) {
  MMPT_REQUIRE(p >= 0.0 && p < 1.0, "dropout_mask: p must lie in [0, 1), got %g", p);
  MMPT_REQUIRE(n >= 0 && n <= (INT64_MAX >> 2), "dropout_mask: bad n");
  MMPT_REQUIRE(n == 0 || keep, "dropout_mask: null pointer");
  if (n == 0) return MMPT_OK;
  const DropArgs a = {dropout_threshold(p), dropout_scale(p), seed};
  const int64_t g = ((n + 3) / 4 + 255) / 256, cap = grid_cap();
  dropout_mask_kernel<<<(unsigned)(g > cap ? cap : g), 256, 0, (hipStream_t)stream>>>(n, site, keep,
                                                                                     a);
  return check_launch("dropout_mask");
}
