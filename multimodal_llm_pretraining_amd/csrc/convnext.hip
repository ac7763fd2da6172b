// K21: the ConvNeXt family (tf:models/convnext/modeling_convnext.py).  The one hot op here that is
// neither a GEMM nor an attention: the 7x7 depthwise convolution of ConvNextLayer, forward, input
// gradient and weight gradient; then the layer-scale residual (out = x + gamma * branch), the
// global average pool and the 2x2/s2 patch permutations that turn the downsample conv into a GEMM.
//
// Layout: activations NHWC (rows (b, y, x), columns c), depthwise weights tap-major [49][C]
// (tap = ky*7 + kx), so one lane owns 8 channels and every access is 16 B.  A workgroup takes a
// spatial tile of up to 14x14 outputs x 64 channels; the tile plus its 3-pixel halo is staged in
// LDS as bf16 (fp32 inputs are cast on the way in), the weights of the 64 channels beside it.
// Pixels outside the image are never loaded: the loader checks every coordinate against its own
// image b and writes zeros, so a halo row above y = 0 cannot read image b-1.  A thread computes a
// strip of 7 outputs along x: per filter row it reads 13 inputs and 7 weights from LDS for 392
// FMAs.  No MFMA: 49 FMAs against 6 compulsory bytes per element.
//
// Reductions over rows (dw, db, dgamma, the pool) are per-workgroup partials summed in a fixed
// order by a second kernel: no atomics, bitwise reproducible.
//
// Stochastic depth (ConvNextDropPath): a block runs over its kept samples only.  The depthwise
// kernels take a template flag IDX: the fp32 stream (x, dx_in / dx_out) is then addressed through
// idx[b'] (compact sample b' -> source plane) while the bf16 side stays compact [Bk][H][W][C]; the
// dense instantiations (IDX = false) never read the map.  droppath_add / droppath_bwd are the
// layer-scale residual and its backward over the kept samples with the factor 1 / keep_prob.
#include <algorithm>

#include "common.h"
#include "philox.h"

namespace mmpt {
namespace {

constexpr int DW_T = 14;       // outputs per tile side (two strips of 7)
constexpr int DW_P = DW_T + 6; // tile + halo
constexpr int DW_WG_TARGET = 512;

struct DwArgs {
  int B, H, W, C, G;           // G = C / 8 lane groups
  int tiles_y, tiles_x;
  int TH, TW, segs, PW, PH;    // tile extents, strips per row, padded tile (PW = segs*7 + 6)
  const float* x32;            // fwd / bwd_weight: the fp32 activation
  const bf16_t* x16;           // bwd_input / bwd_weight: the bf16 gradient dc
  const bf16_t* w;
  const bf16_t* bias;
  bf16_t* o16;                 // fwd
  const float* r32;            // bwd_input: dx_in (nullable)
  float* o32;                  // bwd_input: dx_out
  float* partials;             // bwd_weight
  int nb;                      // bwd_weight: workgroups per channel chunk
  const int* idx;              // IDX kernels: plane of compact sample b' in the fp32 stream
  int planes;                  // IDX kernels: planes in the fp32 stream (idx[b'] < planes)
};

__device__ __forceinline__ void ld8f(const float* p, float* f) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
__device__ __forceinline__ void st8f(float* p, const float* f) {
  *(float4*)p = make_float4(f[0], f[1], f[2], f[3]);
  *(float4*)(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
}

// Stage the pixels [y0, y0 + ph) x [x0, x0 + pw) of image b, channel groups chunk*8 .. +8, into
// lds[(py*pw + px)*8 + g] as bf16.  Loaded only where the pixel lies inside the image AND inside
// the window [y0, y0 + vy) x [x0, x0 + vx); everything else is +0.
template <bool F32>
__device__ __forceinline__ void stage_tile(const DwArgs& a, const void* src, uint4* lds, int b,
                                           int chunk, int y0, int x0, int ph, int pw, int vy,
                                           int vx) {
  const int n = ph * pw * 8;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int g = i & 7, p = i >> 3;
    const int py = p / pw, px = p - py * pw;
    const int gy = y0 + py, gx = x0 + px, gg = chunk * 8 + g;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && py < vy && px < vx && gg < a.G) {
      const long e = (((long)b * a.H + gy) * a.W + gx) * a.C + gg * 8;
      if (F32) {
        const float4 lo = *(const float4*)((const float*)src + e);
        const float4 hi = *(const float4*)((const float*)src + e + 4);
        v = make_uint4(pack2(lo.x, lo.y), pack2(lo.z, lo.w), pack2(hi.x, hi.y), pack2(hi.z, hi.w));
      } else {
        v = *(const uint4*)((const bf16_t*)src + e);
      }
    }
    lds[i] = v;
  }
}

// forward (BWD = false): c = bf16(acc + bias); input gradient (BWD = true): the same correlation
// over dc with the filter flipped, dx_out = dx_in + f32(bf16(acc)).
template <bool BWD, int P, bool IDX = false>
__global__ __launch_bounds__(256) void dwconv7_kernel(const DwArgs a) {
  __shared__ uint4 sw[49 * 8];
  __shared__ uint4 st[P * P * 8];
  const int ntiles = a.tiles_y * a.tiles_x;
  const int b = blockIdx.x / ntiles, tile = blockIdx.x - b * ntiles;
  const int chunk = blockIdx.y;
  const int y0 = (tile / a.tiles_x) * a.TH, x0 = (tile % a.tiles_x) * a.TW;
  // the plane of the fp32 side: through the map, and a map entry outside the stream does nothing
  const int bs = IDX ? a.idx[b] : b;
  if (IDX && (unsigned)bs >= (unsigned)a.planes) return;
  for (int i = threadIdx.x; i < 49 * 8; i += blockDim.x) {
    const int g = i & 7, tap = i >> 3, gg = chunk * 8 + g;
    const int ts = BWD ? 48 - tap : tap;
    sw[i] = gg < a.G ? *(const uint4*)(a.w + (long)ts * a.C + gg * 8) : make_uint4(0u, 0u, 0u, 0u);
  }
  if (BWD) stage_tile<false>(a, a.x16, st, b, chunk, y0 - 3, x0 - 3, a.PH, a.PW, a.PH, a.PW);
  else stage_tile<true>(a, a.x32, st, bs, chunk, y0 - 3, x0 - 3, a.PH, a.PW, a.PH, a.PW);
  __syncthreads();
  const int g = threadIdx.x & 7, strip = threadIdx.x >> 3, gg = chunk * 8 + g;
  if (strip >= a.TH * a.segs || gg >= a.G) return;
  const int ty = strip / a.segs, sx = (strip - ty * a.segs) * 7;
  const int oy = y0 + ty;
  if (oy >= a.H) return;
  float acc[7][8];
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[r][c] = 0.f;
#pragma unroll 1
  for (int ky = 0; ky < 7; ++ky) {
    float wf[7][8];
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) unpack8(sw[(ky * 7 + kx) * 8 + g], wf[kx]);
    const uint4* row = st + ((ty + ky) * a.PW + sx) * 8 + g;
#pragma unroll
    for (int j = 0; j < 13; ++j) {
      float v[8];
      unpack8(row[j * 8], v);
#pragma unroll
      for (int r = 0; r < 7; ++r) {
        const int kx = j - r;
        if (kx < 0 || kx > 6) continue;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[r][c] = fmaf(v[c], wf[kx][c], acc[r][c]);
      }
    }
  }
  float bf[8];
  if (!BWD) unpack8(*(const uint4*)(a.bias + gg * 8), bf);
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    const int ox = x0 + sx + r;
    if (ox >= a.W || sx + r >= a.TW) continue;
    const long e = (((long)(BWD ? bs : b) * a.H + oy) * a.W + ox) * a.C + gg * 8;
    if (!BWD) {
      float o[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) o[c] = acc[r][c] + bf[c];
      *(uint4*)(a.o16 + e) = pack8(o);
    } else {
      float4 lo = make_float4(round_bf(acc[r][0]), round_bf(acc[r][1]), round_bf(acc[r][2]),
                              round_bf(acc[r][3]));
      float4 hi = make_float4(round_bf(acc[r][4]), round_bf(acc[r][5]), round_bf(acc[r][6]),
                              round_bf(acc[r][7]));
      if (a.r32 != nullptr) {
        const float4 p = *(const float4*)(a.r32 + e), q = *(const float4*)(a.r32 + e + 4);
        lo = make_float4(p.x + lo.x, p.y + lo.y, p.z + lo.z, p.w + lo.w);
        hi = make_float4(q.x + hi.x, q.y + hi.y, q.z + hi.z, q.w + hi.w);
      }
      *(float4*)(a.o32 + e) = lo;
      *(float4*)(a.o32 + e + 4) = hi;
    }
  }
}

// Weight gradient.  Threads = 8 lane groups x 7 filter rows x 4 strip slots (224 of 256 compute):
// thread (g, ky, slot) holds dw[ky][0..6][8 channels] in registers and walks the strips
// slot, slot + 4, ... of every tile its workgroup visits (grid-stride over (b, tile)).  The four
// slots are then summed in slot order through LDS and the workgroup writes one [50][64] partial
// (row 49 = the bias gradient, gathered by the ky = 0 threads).
template <int P, int T, bool IDX = false>
__global__ __launch_bounds__(256) void dwconv7_bwd_weight_kernel(const DwArgs a) {
  __shared__ uint4 sx[P * P * 8];
  __shared__ uint4 sd[T * T * 8];
  __shared__ float red[50 * 64];
  const int ntiles = a.tiles_y * a.tiles_x, items = a.B * ntiles;
  const int chunk = blockIdx.y;
  const int tid = threadIdx.x, g = tid & 7, ky = (tid >> 3) % 7, slot = tid / 56;
  const int gg = chunk * 8 + g, DW = a.segs * 7, nstrips = a.TH * a.segs;
  float acc[7][8], dbs[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    dbs[c] = 0.f;
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k][c] = 0.f;
  }
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int b = item / ntiles, tile = item - b * ntiles;
    const int y0 = (tile / a.tiles_x) * a.TH, x0 = (tile % a.tiles_x) * a.TW;
    const int bs = IDX ? a.idx[b] : b;
    if (IDX && (unsigned)bs >= (unsigned)a.planes) continue;  // uniform over the workgroup
    __syncthreads();  // the previous item's readers are done
    stage_tile<true>(a, a.x32, sx, bs, chunk, y0 - 3, x0 - 3, a.PH, a.PW, a.PH, a.PW);
    stage_tile<false>(a, a.x16, sd, b, chunk, y0, x0, a.TH, DW, a.TH, a.TW);
    __syncthreads();
    if (slot < 4 && gg < a.G)
#pragma unroll 1
      for (int strip = slot; strip < nstrips; strip += 4) {
        const int ty = strip / a.segs, so = (strip - ty * a.segs) * 7;
        float df[7][8];
#pragma unroll
        for (int r = 0; r < 7; ++r) unpack8(sd[(ty * DW + so + r) * 8 + g], df[r]);
        if (ky == 0)
#pragma unroll
          for (int r = 0; r < 7; ++r)
#pragma unroll
            for (int c = 0; c < 8; ++c) dbs[c] += df[r][c];
        const uint4* row = sx + ((ty + ky) * a.PW + so) * 8 + g;
#pragma unroll
        for (int j = 0; j < 13; ++j) {
          float v[8];
          unpack8(row[j * 8], v);
#pragma unroll
          for (int r = 0; r < 7; ++r) {
            const int kx = j - r;
            if (kx < 0 || kx > 6) continue;
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[kx][c] = fmaf(df[r][c], v[c], acc[kx][c]);
          }
        }
      }
  }
  for (int s = 0; s < 4; ++s) {
    if (slot == s) {
#pragma unroll
      for (int kx = 0; kx < 7; ++kx)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          float* d = red + (ky * 7 + kx) * 64 + g * 8 + c;
          *d = s == 0 ? acc[kx][c] : *d + acc[kx][c];
        }
      if (ky == 0)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          float* d = red + 49 * 64 + g * 8 + c;
          *d = s == 0 ? dbs[c] : *d + dbs[c];
        }
    }
    __syncthreads();
  }
  float* out = a.partials + ((long)chunk * a.nb + blockIdx.x) * (50 * 64);
  for (int i = tid; i < 50 * 64; i += blockDim.x) out[i] = red[i];
}

// dw[tap][c] += f32(bf16(Σ_n partial)), db[c] likewise: one thread per (row, channel), the
// partials summed in workgroup order
__global__ __launch_bounds__(256) void dwconv7_reduce_kernel(int C, int nb,
                                                             const float* __restrict__ partials,
                                                             float* dw, float* db) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= 50L * C) return;
  const int r = (int)(i / C), c = (int)(i - (long)r * C);
  const int chunk = c >> 6, cc = c & 63;
  const float* p = partials + ((long)chunk * nb * 50 + r) * 64 + cc;
  float s = 0.f;
  for (int n = 0; n < nb; ++n) s += p[(long)n * 50 * 64];
  s = round_bf(s);
  if (r < 49) dw[(long)r * C + c] += s;
  else db[c] += s;
}

// ---- row-wise helpers: a workgroup = 32 lane groups (256 channels) x 8 row slots --------------
constexpr int RS_SLOTS = 8;
constexpr int RS_BLOCKS = 256;

// r + g*y with the product and the sum each rounded to fp32 (torch: a mul kernel, then an add
// kernel).  hipcc contracts a*b + c to one fma by default, and __fmul_rn / __fadd_rn are plain
// operators in its headers, so contraction is switched off for these two statements.
__device__ __forceinline__ float mul_add2(float r, float g, float y) {
#pragma clang fp contract(off)
  const float p = g * y;
  return r + p;
}

__global__ __launch_bounds__(256) void layerscale_add_kernel(long rows, int C, const float* resid,
                                                             const float* __restrict__ gamma,
                                                             const bf16_t* __restrict__ y, long ld_y,
                                                             float* out) {
  const int G = C >> 3;
  const long n = rows * G;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / G;
    const int g = (int)(i - r * G);
    float yf[8];
    unpack8(*(const uint4*)(y + r * ld_y + g * 8), yf);
    const float4 g0 = *(const float4*)(gamma + g * 8), g1 = *(const float4*)(gamma + g * 8 + 4);
    const float4 r0 = *(const float4*)(resid + r * C + g * 8);
    const float4 r1 = *(const float4*)(resid + r * C + g * 8 + 4);
    const float4 o0 = make_float4(mul_add2(r0.x, g0.x, yf[0]), mul_add2(r0.y, g0.y, yf[1]),
                                  mul_add2(r0.z, g0.z, yf[2]), mul_add2(r0.w, g0.w, yf[3]));
    const float4 o1 = make_float4(mul_add2(r1.x, g1.x, yf[4]), mul_add2(r1.y, g1.y, yf[5]),
                                  mul_add2(r1.z, g1.z, yf[6]), mul_add2(r1.w, g1.w, yf[7]));
    *(float4*)(out + r * C + g * 8) = o0;
    *(float4*)(out + r * C + g * 8 + 4) = o1;
  }
}

// Sum over the slots of a workgroup in slot order, then hand 8 columns to the caller's store.
__device__ __forceinline__ void slot_sum(float (*red)[32][8], int slot, int gl, float* s) {
#pragma unroll
  for (int c = 0; c < 8; ++c) red[slot][gl][c] = s[c];
  __syncthreads();
  if (slot == 0)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float t = red[0][gl][c];
      for (int k = 1; k < RS_SLOTS; ++k) t += red[k][gl][c];
      s[c] = t;
    }
}

// dy = bf16(gamma * g); partial[blockIdx.y][c] = Σ_{this workgroup's rows} g * f32(y)
__global__ __launch_bounds__(256) void layerscale_bwd_kernel(long rows, int C, const float* __restrict__ gr,
                                                             const float* __restrict__ gamma,
                                                             const bf16_t* __restrict__ y, long ld_y,
                                                             bf16_t* dy, long ld_dy, float* partials) {
  __shared__ float red[RS_SLOTS][32][8];
  const int gl = threadIdx.x & 31, slot = threadIdx.x >> 5;
  const int g = blockIdx.x * 32 + gl, G = C >> 3;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (g < G) {
    float gm[8];
    ld8f(gamma + g * 8, gm);
    for (long r = (long)blockIdx.y * RS_SLOTS + slot; r < rows; r += (long)gridDim.y * RS_SLOTS) {
      float gv[8], yf[8], o[8];
      ld8f(gr + r * C + g * 8, gv);
      unpack8(*(const uint4*)(y + r * ld_y + g * 8), yf);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        o[c] = gm[c] * gv[c];
        s[c] = fmaf(gv[c], yf[c], s[c]);
      }
      *(uint4*)(dy + r * ld_dy + g * 8) = pack8(o);
    }
  }
  slot_sum(red, slot, gl, s);
  if (slot == 0 && g < G) {
    st8f(partials + (long)blockIdx.y * C + g * 8, s);
  }
}

__global__ __launch_bounds__(256) void colsum_partials_kernel(int C, int nb, const float* __restrict__ partials,
                                                              float* dst) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int n = 0; n < nb; ++n) s += partials[(long)n * C + c];
  dst[c] += s;
}

// ConvNextDropPath on the layer-scale residual: r + (g*y)*s with the two products and the sum
// each rounded to fp32 (torch: mul, div by the scalar keep_prob = a mul by s, add).
__device__ __forceinline__ float mul_mul_add3(float r, float g, float y, float s) {
#pragma clang fp contract(off)
  const float p = g * y;
  const float q = p * s;
  return r + q;
}
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  const float p = a * b;
  return p;
}

// One pass over the dense stream: a kept plane (slot[b] >= 0, its branch at compact plane slot[b])
// gets the rule above, a dropped plane is copied.
__global__ __launch_bounds__(256) void droppath_add_kernel(long rows, int rps, int C, int kept,
                                                           const float* resid,
                                                           const float* __restrict__ gamma,
                                                           const bf16_t* __restrict__ y, long ld_y,
                                                           const int* __restrict__ slot, float s,
                                                           float* out) {
  const int G = C >> 3;
  const long n = rows * G;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / G;
    const int g = (int)(i - r * G);
    const long b = r / rps;
    const int sl = slot[b];
    float o[8];
    ld8f(resid + r * C + g * 8, o);
    if (sl >= 0 && sl < kept) {
      const long ry = (long)sl * rps + (r - b * rps);
      float yf[8], gm[8];
      unpack8(*(const uint4*)(y + ry * ld_y + g * 8), yf);
      ld8f(gamma + g * 8, gm);
#pragma unroll
      for (int c = 0; c < 8; ++c) o[c] = mul_mul_add3(o[c], gm[c], yf[c], s);
    }
    st8f(out + r * C + g * 8, o);
  }
}

// layerscale_bwd_kernel over the kept samples: compact row r reads g at plane idx[r / rps], with
// g' = g*s (rounded to fp32) in the place of g.
__global__ __launch_bounds__(256) void droppath_bwd_kernel(long rows, int rps, int C, int planes,
                                                           const float* __restrict__ gr,
                                                           const int* __restrict__ idx,
                                                           const float* __restrict__ gamma,
                                                           const bf16_t* __restrict__ y, long ld_y,
                                                           float sc, bf16_t* dy, long ld_dy,
                                                           float* partials) {
  __shared__ float red[RS_SLOTS][32][8];
  const int gl = threadIdx.x & 31, slot = threadIdx.x >> 5;
  const int g = blockIdx.x * 32 + gl, G = C >> 3;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (g < G) {
    float gm[8];
    ld8f(gamma + g * 8, gm);
    for (long r = (long)blockIdx.y * RS_SLOTS + slot; r < rows; r += (long)gridDim.y * RS_SLOTS) {
      const long b = r / rps;
      const int bs = idx[b];
      if ((unsigned)bs >= (unsigned)planes) continue;
      const long rg = (long)bs * rps + (r - b * rps);
      float gv[8], yf[8], o[8];
      ld8f(gr + rg * C + g * 8, gv);
      unpack8(*(const uint4*)(y + r * ld_y + g * 8), yf);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float gp = mul_rn(gv[c], sc);
        o[c] = gm[c] * gp;
        s[c] = fmaf(gp, yf[c], s[c]);
      }
      *(uint4*)(dy + r * ld_dy + g * 8) = pack8(o);
    }
  }
  slot_sum(red, slot, gl, s);
  if (slot == 0 && g < G) {
    st8f(partials + (long)blockIdx.y * C + g * 8, s);
  }
}

// p[b][c] = (Σ_hw x[b][hw][c]) * (1 / HW): one workgroup per (256 channels, image).  The scale is
// the fp32 reciprocal, as torch's device mean (and its division by a scalar) applies it.
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(int HW, int C, const float* __restrict__ x,
                                                          float* p) {
  __shared__ float red[RS_SLOTS][32][8];
  const int gl = threadIdx.x & 31, slot = threadIdx.x >> 5;
  const int g = blockIdx.x * 32 + gl, G = C >> 3;
  const long b = blockIdx.y;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (g < G)
    for (int r = slot; r < HW; r += RS_SLOTS) {
      const float* q = x + (b * HW + r) * C + g * 8;
      const float4 lo = *(const float4*)q, hi = *(const float4*)(q + 4);
      s[0] += lo.x; s[1] += lo.y; s[2] += lo.z; s[3] += lo.w;
      s[4] += hi.x; s[5] += hi.y; s[6] += hi.z; s[7] += hi.w;
    }
  slot_sum(red, slot, gl, s);
  if (slot == 0 && g < G) {
    const float d = 1.0f / (float)HW;
    float* o = p + b * C + g * 8;
    *(float4*)o = make_float4(s[0] * d, s[1] * d, s[2] * d, s[3] * d);
    *(float4*)(o + 4) = make_float4(s[4] * d, s[5] * d, s[6] * d, s[7] * d);
  }
}

__global__ __launch_bounds__(256) void avgpool_bwd_kernel(long B, int HW, int C, const float* __restrict__ dp,
                                                          float* dx) {
  const int G4 = C >> 2;
  const long n = B * HW * G4;
  const float d = 1.0f / (float)HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / G4;
    const int q = (int)(i - r * G4);
    const float4 v = *(const float4*)(dp + (r / HW) * C + q * 4);
    *(float4*)(dx + r * C + q * 4) = make_float4(v.x * d, v.y * d, v.z * d, v.w * d);
  }
}

// rows[(b, oy, ox)][(ky*2 + kx)*C + c] = x[b][2 oy + ky][2 ox + kx][c], 16 B per thread.
// INV: the inverse, widening bf16 to fp32 (exact).
template <bool INV>
__global__ __launch_bounds__(256) void patchify2_kernel(long B, int H, int W, int C, const bf16_t* __restrict__ src,
                                                        bf16_t* dst16, float* dst32) {
  const int G = C >> 3;
  const long n = B * H * W * G;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int g = (int)(i % G);
    long p = i / G;  // NHWC pixel index
    const int xx = (int)(p % W);
    p /= W;
    const int yy = (int)(p % H);
    const long b = p / H;
    const long row = (b * (H >> 1) + (yy >> 1)) * (W >> 1) + (xx >> 1);
    const long er = row * 4 * C + (long)((yy & 1) * 2 + (xx & 1)) * C + g * 8;
    const long ex = i * 8;
    if (!INV) {
      *(uint4*)(dst16 + er) = *(const uint4*)(src + ex);
    } else {
      float f[8];
      unpack8(*(const uint4*)(src + er), f);
      st8f(dst32 + ex, f);
    }
  }
}

inline unsigned blocks_for(int64_t n) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192));
}

void dw_geometry(DwArgs& a, int64_t B, int64_t H, int64_t W, int64_t C) {
  a.B = (int)B; a.H = (int)H; a.W = (int)W; a.C = (int)C; a.G = (int)(C / 8);
  a.TH = (int)std::min<int64_t>(H, DW_T);
  a.TW = (int)std::min<int64_t>(W, DW_T);
  a.tiles_y = (a.H + a.TH - 1) / a.TH;
  a.tiles_x = (a.W + a.TW - 1) / a.TW;
  a.segs = (a.TW + 6) / 7;
  a.PW = a.segs * 7 + 6;
  a.PH = a.TH + 6;
}
inline int dw_chunks(const DwArgs& a) { return (a.G + 7) / 8; }
inline int64_t dw_nb(const DwArgs& a) {
  const int64_t items = (int64_t)a.B * a.tiles_y * a.tiles_x;
  return std::max<int64_t>(1, std::min<int64_t>(items, DW_WG_TARGET / dw_chunks(a)));
}

}  // namespace
}  // namespace mmpt

using namespace mmpt;

#define MMPT_CN_PLANE(what)                                                                      \
  MMPT_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && C <= 4096 &&                    \
                   H < ((int64_t)1 << 31) && W < ((int64_t)1 << 31) &&                           \
                   B < ((int64_t)1 << 31) && B * H < ((int64_t)1 << 31) &&                       \
                   B * H * W < ((int64_t)1 << 31),                                               \
               what ": B, H, W >= 1 with B*H*W < 2^31, C a positive multiple of 8 and <= 4096 " \
                    "(B %lld, H %lld, W %lld, C %lld)",                                          \
               (long long)B, (long long)H, (long long)W, (long long)C)
#define MMPT_CN_ROWS(what)                                                                      \
  MMPT_REQUIRE(rows > 0 && rows < ((int64_t)1 << 31) && C > 0 && C % 8 == 0 && C <= 4096,       \
               what ": rows in [1, 2^31), C a positive multiple of 8 and <= 4096 (rows %lld, " \
                    "C %lld)", (long long)rows, (long long)C)
#define MMPT_CN_LD(what, ld) \
  MMPT_REQUIRE((ld) >= C && (ld) % 8 == 0, what ": " #ld " must be a multiple of 8 and >= C")

extern "C" int mmpt_dwconv7_fwd(int64_t B, int64_t H, int64_t W, int64_t C, const float* x,
                                const void* w, const void* bias, void* c, void* stream) {
  MMPT_CN_PLANE("dwconv7_fwd");
  MMPT_REQUIRE(x && w && bias && c, "dwconv7_fwd: null pointer");
  MMPT_REQUIRE(al16(x) && al16(w) && al16(bias) && al16(c),
               "dwconv7_fwd: pointers must be 16-byte aligned");
  DwArgs a = {};
  dw_geometry(a, B, H, W, C);
  a.x32 = x; a.w = (const bf16_t*)w; a.bias = (const bf16_t*)bias; a.o16 = (bf16_t*)c;
  const dim3 grid((unsigned)(B * a.tiles_y * a.tiles_x), (unsigned)dw_chunks(a));
  const unsigned threads = (unsigned)((8 * a.TH * a.segs + 63) / 64 * 64);
  if (a.TH <= 7 && a.TW <= 7) dwconv7_kernel<false, 13><<<grid, threads, 0, (hipStream_t)stream>>>(a);
  else dwconv7_kernel<false, DW_P><<<grid, threads, 0, (hipStream_t)stream>>>(a);
  return check_launch("dwconv7_fwd");
}

extern "C" int mmpt_dwconv7_bwd_input(int64_t B, int64_t H, int64_t W, int64_t C, const void* dc,
                                      const void* w, const float* dx_in, float* dx_out,
                                      void* stream) {
  MMPT_CN_PLANE("dwconv7_bwd_input");
  MMPT_REQUIRE(dc && w && dx_out, "dwconv7_bwd_input: null pointer");
  MMPT_REQUIRE(al16(dc) && al16(w) && al16(dx_in) && al16(dx_out),
               "dwconv7_bwd_input: pointers must be 16-byte aligned");
  DwArgs a = {};
  dw_geometry(a, B, H, W, C);
  a.x16 = (const bf16_t*)dc; a.w = (const bf16_t*)w; a.r32 = dx_in; a.o32 = dx_out;
  const dim3 grid((unsigned)(B * a.tiles_y * a.tiles_x), (unsigned)dw_chunks(a));
  const unsigned threads = (unsigned)((8 * a.TH * a.segs + 63) / 64 * 64);
  if (a.TH <= 7 && a.TW <= 7) dwconv7_kernel<true, 13><<<grid, threads, 0, (hipStream_t)stream>>>(a);
  else dwconv7_kernel<true, DW_P><<<grid, threads, 0, (hipStream_t)stream>>>(a);
  return check_launch("dwconv7_bwd_input");
}

extern "C" int64_t mmpt_dwconv7_bwd_weight_workspace_bytes(int64_t B, int64_t H, int64_t W,
                                                           int64_t C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || B * H * W >= ((int64_t)1 << 31))
    return 0;
  DwArgs a = {};
  dw_geometry(a, B, H, W, C);
  return (int64_t)dw_chunks(a) * dw_nb(a) * 50 * 64 * (int64_t)sizeof(float);
}

extern "C" int mmpt_dwconv7_bwd_weight(int64_t B, int64_t H, int64_t W, int64_t C, const float* x,
                                       const void* dc, float* dw, float* db, void* workspace,
                                       void* stream) {
  MMPT_CN_PLANE("dwconv7_bwd_weight");
  MMPT_REQUIRE(x && dc && dw && db && workspace, "dwconv7_bwd_weight: null pointer");
  MMPT_REQUIRE(al16(x) && al16(dc) && al16(dw) && al16(db) && al16(workspace),
               "dwconv7_bwd_weight: pointers must be 16-byte aligned");
  DwArgs a = {};
  dw_geometry(a, B, H, W, C);
  a.x32 = x; a.x16 = (const bf16_t*)dc; a.partials = (float*)workspace; a.nb = (int)dw_nb(a);
  const dim3 grid((unsigned)a.nb, (unsigned)dw_chunks(a));
  if (a.TH <= 7 && a.TW <= 7)
    dwconv7_bwd_weight_kernel<13, 7><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  else
    dwconv7_bwd_weight_kernel<DW_P, DW_T><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  int rc = check_launch("dwconv7_bwd_weight");
  if (rc) return rc;
  dwconv7_reduce_kernel<<<(unsigned)((50 * C + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (int)C, a.nb, a.partials, dw, db);
  return check_launch("dwconv7_bwd_weight");
}

// ---- stochastic depth: the sample-indexed forms and the drop-path residual ---------------------
#define MMPT_CN_KEPT(what)                                                                    \
  MMPT_REQUIRE(Bk >= 1 && Bk <= B, what ": 1 <= Bk <= B (Bk %lld, B %lld)", (long long)Bk, \
               (long long)B)
#define MMPT_CN_P(what) \
  MMPT_REQUIRE(p >= 0.0 && p < 1.0, what ": p must lie in [0, 1), got %g", p)

extern "C" int mmpt_dwconv7_idx_fwd(int64_t B, int64_t Bk, int64_t H, int64_t W, int64_t C,
                                    const float* x, const void* idx, const void* w,
                                    const void* bias, void* c, void* stream) {
  MMPT_CN_PLANE("dwconv7_idx_fwd");
  MMPT_CN_KEPT("dwconv7_idx_fwd");
  MMPT_REQUIRE(x && idx && w && bias && c, "dwconv7_idx_fwd: null pointer");
  MMPT_REQUIRE(al16(x) && al16(w) && al16(bias) && al16(c) && al4(idx),
               "dwconv7_idx_fwd: pointers must be 16-byte aligned (idx: 4-byte)");
  DwArgs a = {};
  dw_geometry(a, Bk, H, W, C);
  a.x32 = x; a.w = (const bf16_t*)w; a.bias = (const bf16_t*)bias; a.o16 = (bf16_t*)c;
  a.idx = (const int*)idx; a.planes = (int)B;
  const dim3 grid((unsigned)(Bk * a.tiles_y * a.tiles_x), (unsigned)dw_chunks(a));
  const unsigned threads = (unsigned)((8 * a.TH * a.segs + 63) / 64 * 64);
  if (a.TH <= 7 && a.TW <= 7)
    dwconv7_kernel<false, 13, true><<<grid, threads, 0, (hipStream_t)stream>>>(a);
  else
    dwconv7_kernel<false, DW_P, true><<<grid, threads, 0, (hipStream_t)stream>>>(a);
  return check_launch("dwconv7_idx_fwd");
}

extern "C" int mmpt_dwconv7_idx_bwd_input(int64_t B, int64_t Bk, int64_t H, int64_t W, int64_t C,
                                          const void* dc, const void* idx, const void* w,
                                          const float* dx_in, float* dx_out, void* stream) {
  MMPT_CN_PLANE("dwconv7_idx_bwd_input");
  MMPT_CN_KEPT("dwconv7_idx_bwd_input");
  MMPT_REQUIRE(dc && idx && w && dx_out, "dwconv7_idx_bwd_input: null pointer");
  MMPT_REQUIRE(al16(dc) && al16(w) && al16(dx_in) && al16(dx_out) && al4(idx),
               "dwconv7_idx_bwd_input: pointers must be 16-byte aligned (idx: 4-byte)");
  DwArgs a = {};
  dw_geometry(a, Bk, H, W, C);
  a.x16 = (const bf16_t*)dc; a.w = (const bf16_t*)w; a.r32 = dx_in; a.o32 = dx_out;
  a.idx = (const int*)idx; a.planes = (int)B;
  const dim3 grid((unsigned)(Bk * a.tiles_y * a.tiles_x), (unsigned)dw_chunks(a));
  const unsigned threads = (unsigned)((8 * a.TH * a.segs + 63) / 64 * 64);
  if (a.TH <= 7 && a.TW <= 7)
    dwconv7_kernel<true, 13, true><<<grid, threads, 0, (hipStream_t)stream>>>(a);
  else
    dwconv7_kernel<true, DW_P, true><<<grid, threads, 0, (hipStream_t)stream>>>(a);
  return check_launch("dwconv7_idx_bwd_input");
}

extern "C" int mmpt_dwconv7_idx_bwd_weight(int64_t B, int64_t Bk, int64_t H, int64_t W, int64_t C,
                                           const float* x, const void* idx, const void* dc,
                                           float* dw, float* db, void* workspace, void* stream) {
  MMPT_CN_PLANE("dwconv7_idx_bwd_weight");
  MMPT_CN_KEPT("dwconv7_idx_bwd_weight");
  MMPT_REQUIRE(x && idx && dc && dw && db && workspace, "dwconv7_idx_bwd_weight: null pointer");
  MMPT_REQUIRE(al16(x) && al16(dc) && al16(dw) && al16(db) && al16(workspace) && al4(idx),
               "dwconv7_idx_bwd_weight: pointers must be 16-byte aligned (idx: 4-byte)");
  DwArgs a = {};
  dw_geometry(a, Bk, H, W, C);
  a.x32 = x; a.x16 = (const bf16_t*)dc; a.partials = (float*)workspace; a.nb = (int)dw_nb(a);
  a.idx = (const int*)idx; a.planes = (int)B;
  const dim3 grid((unsigned)a.nb, (unsigned)dw_chunks(a));
  if (a.TH <= 7 && a.TW <= 7)
    dwconv7_bwd_weight_kernel<13, 7, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  else
    dwconv7_bwd_weight_kernel<DW_P, DW_T, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  int rc = check_launch("dwconv7_idx_bwd_weight");
  if (rc) return rc;
  dwconv7_reduce_kernel<<<(unsigned)((50 * C + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (int)C, a.nb, a.partials, dw, db);
  return check_launch("dwconv7_idx_bwd_weight");
}

#define MMPT_CN_SAMPLES(what)                                                                    \
  MMPT_REQUIRE(B > 0 && rows_per_sample > 0 && B < ((int64_t)1 << 31) &&                         \
                   rows_per_sample < ((int64_t)1 << 31) &&                                       \
                   B * rows_per_sample < ((int64_t)1 << 31) && C > 0 && C % 8 == 0 && C <= 4096, \
               what ": B, rows_per_sample >= 1 with B*rows_per_sample < 2^31, C a positive "    \
                    "multiple of 8 and <= 4096 (B %lld, rows_per_sample %lld, C %lld)",          \
               (long long)B, (long long)rows_per_sample, (long long)C)

extern "C" int mmpt_droppath_add_fwd(int64_t B, int64_t Bk, int64_t rows_per_sample, int64_t C,
                                     const float* resid, const float* gamma, const void* y,
                                     int64_t ld_y, const void* slot, double p, float* out,
                                     void* stream) {
  MMPT_CN_SAMPLES("droppath_add_fwd");
  MMPT_REQUIRE(Bk >= 0 && Bk <= B, "droppath_add_fwd: 0 <= Bk <= B (Bk %lld, B %lld)",
               (long long)Bk, (long long)B);
  MMPT_CN_P("droppath_add_fwd");
  MMPT_REQUIRE(resid && gamma && slot && out && (y || Bk == 0), "droppath_add_fwd: null pointer");
  if (Bk > 0) MMPT_CN_LD("droppath_add_fwd", ld_y);
  MMPT_REQUIRE(al16(resid) && al16(gamma) && al16(y) && al16(out) && al4(slot),
               "droppath_add_fwd: pointers must be 16-byte aligned (slot: 4-byte)");
  const int64_t rows = B * rows_per_sample;
  droppath_add_kernel<<<blocks_for(rows * (C / 8)), 256, 0, (hipStream_t)stream>>>(
      rows, (int)rows_per_sample, (int)C, (int)Bk, resid, gamma, (const bf16_t*)y, ld_y,
      (const int*)slot, dropout_scale(p), out);
  return check_launch("droppath_add_fwd");
}

extern "C" int64_t mmpt_droppath_bwd_workspace_bytes(int64_t Bk, int64_t rows_per_sample,
                                                     int64_t C) {
  return mmpt_layerscale_bwd_workspace_bytes(Bk * rows_per_sample, C);
}

extern "C" int mmpt_droppath_bwd(int64_t B, int64_t Bk, int64_t rows_per_sample, int64_t C,
                                 const float* g, const void* idx, const float* gamma,
                                 const void* y, int64_t ld_y, double p, void* dy, int64_t ld_dy,
                                 float* dgamma, void* workspace, void* stream) {
  MMPT_CN_SAMPLES("droppath_bwd");
  MMPT_CN_KEPT("droppath_bwd");
  MMPT_CN_P("droppath_bwd");
  MMPT_CN_LD("droppath_bwd", ld_y);
  MMPT_CN_LD("droppath_bwd", ld_dy);
  MMPT_REQUIRE(g && idx && gamma && y && dy && dgamma && workspace, "droppath_bwd: null pointer");
  MMPT_REQUIRE(al16(g) && al16(gamma) && al16(y) && al16(dy) && al16(dgamma) && al16(workspace) &&
                   al4(idx),
               "droppath_bwd: pointers must be 16-byte aligned (idx: 4-byte)");
  const int64_t rows = Bk * rows_per_sample;
  const int nb = (int)std::min<int64_t>(RS_BLOCKS, (rows + RS_SLOTS - 1) / RS_SLOTS);
  const dim3 grid((unsigned)((C / 8 + 31) / 32), (unsigned)nb);
  droppath_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(
      rows, (int)rows_per_sample, (int)C, (int)B, g, (const int*)idx, gamma, (const bf16_t*)y,
      ld_y, dropout_scale(p), (bf16_t*)dy, ld_dy, (float*)workspace);
  int rc = check_launch("droppath_bwd");
  if (rc) return rc;
  colsum_partials_kernel<<<(unsigned)((C + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (int)C, nb, (const float*)workspace, dgamma);
  return check_launch("droppath_bwd");
}

extern "C" int mmpt_layerscale_add_fwd(int64_t rows, int64_t C, const float* resid,
                                       const float* gamma, const void* y, int64_t ld_y, float* out,
                                       void* stream) {
  MMPT_CN_ROWS("layerscale_add_fwd");
  MMPT_CN_LD("layerscale_add_fwd", ld_y);
  MMPT_REQUIRE(resid && gamma && y && out, "layerscale_add_fwd: null pointer");
  MMPT_REQUIRE(al16(resid) && al16(gamma) && al16(y) && al16(out),
               "layerscale_add_fwd: pointers must be 16-byte aligned");
  layerscale_add_kernel<<<blocks_for(rows * (C / 8)), 256, 0, (hipStream_t)stream>>>(
      rows, (int)C, resid, gamma, (const bf16_t*)y, ld_y, out);
  return check_launch("layerscale_add_fwd");
}

extern "C" int64_t mmpt_layerscale_bwd_workspace_bytes(int64_t rows, int64_t C) {
  const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(RS_BLOCKS, (rows + RS_SLOTS - 1) / RS_SLOTS));
  return nb * C * (int64_t)sizeof(float);
}

extern "C" int mmpt_layerscale_bwd(int64_t rows, int64_t C, const float* g, const float* gamma,
                                   const void* y, int64_t ld_y, void* dy, int64_t ld_dy,
                                   float* dgamma, void* workspace, void* stream) {
  MMPT_CN_ROWS("layerscale_bwd");
  MMPT_CN_LD("layerscale_bwd", ld_y);
  MMPT_CN_LD("layerscale_bwd", ld_dy);
  MMPT_REQUIRE(g && gamma && y && dy && dgamma && workspace, "layerscale_bwd: null pointer");
  MMPT_REQUIRE(al16(g) && al16(gamma) && al16(y) && al16(dy) && al16(dgamma) && al16(workspace),
               "layerscale_bwd: pointers must be 16-byte aligned");
  const int nb = (int)std::min<int64_t>(RS_BLOCKS, (rows + RS_SLOTS - 1) / RS_SLOTS);
  const dim3 grid((unsigned)((C / 8 + 31) / 32), (unsigned)nb);
  layerscale_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(
      rows, (int)C, g, gamma, (const bf16_t*)y, ld_y, (bf16_t*)dy, ld_dy, (float*)workspace);
  int rc = check_launch("layerscale_bwd");
  if (rc) return rc;
  colsum_partials_kernel<<<(unsigned)((C + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (int)C, nb, (const float*)workspace, dgamma);
  return check_launch("layerscale_bwd");
}

extern "C" int mmpt_avgpool_fwd(int64_t B, int64_t HW, int64_t C, const float* x, float* p,
                                void* stream) {
  MMPT_REQUIRE(B > 0 && B <= 65535 && HW > 0 && B * HW < ((int64_t)1 << 31) && C > 0 &&
                   C % 8 == 0 && C <= 4096,
               "avgpool_fwd: B in [1, 65535], HW >= 1, B*HW < 2^31, C a positive multiple of 8 "
               "and <= 4096 (B %lld, HW %lld, C %lld)", (long long)B, (long long)HW, (long long)C);
  MMPT_REQUIRE(x && p, "avgpool_fwd: null pointer");
  MMPT_REQUIRE(al16(x) && al16(p), "avgpool_fwd: pointers must be 16-byte aligned");
  const dim3 grid((unsigned)((C / 8 + 31) / 32), (unsigned)B);
  avgpool_fwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((int)HW, (int)C, x, p);
  return check_launch("avgpool_fwd");
}

extern "C" int mmpt_avgpool_bwd(int64_t B, int64_t HW, int64_t C, const float* dp, float* dx,
                                void* stream) {
  MMPT_REQUIRE(B > 0 && HW > 0 && B * HW < ((int64_t)1 << 31) && C > 0 && C % 8 == 0 && C <= 4096,
               "avgpool_bwd: B, HW >= 1, B*HW < 2^31, C a positive multiple of 8 and <= 4096 "
               "(B %lld, HW %lld, C %lld)", (long long)B, (long long)HW, (long long)C);
  MMPT_REQUIRE(dp && dx, "avgpool_bwd: null pointer");
  MMPT_REQUIRE(al16(dp) && al16(dx), "avgpool_bwd: pointers must be 16-byte aligned");
  avgpool_bwd_kernel<<<blocks_for(B * HW * (C / 4)), 256, 0, (hipStream_t)stream>>>(
      B, (int)HW, (int)C, dp, dx);
  return check_launch("avgpool_bwd");
}

extern "C" int mmpt_patchify2_nhwc(int64_t B, int64_t H, int64_t W, int64_t C, const void* x,
                                   void* rows, void* stream) {
  MMPT_CN_PLANE("patchify2_nhwc");
  MMPT_REQUIRE(H % 2 == 0 && W % 2 == 0, "patchify2_nhwc: H and W must be even (H %lld, W %lld)",
               (long long)H, (long long)W);
  MMPT_REQUIRE(x && rows, "patchify2_nhwc: null pointer");
  MMPT_REQUIRE(al16(x) && al16(rows), "patchify2_nhwc: pointers must be 16-byte aligned");
  patchify2_kernel<false><<<blocks_for(B * H * W * (C / 8)), 256, 0, (hipStream_t)stream>>>(
      B, (int)H, (int)W, (int)C, (const bf16_t*)x, (bf16_t*)rows, nullptr);
  return check_launch("patchify2_nhwc");
}

extern "C" int mmpt_unpatchify2_nhwc(int64_t B, int64_t H, int64_t W, int64_t C, const void* rows,
                                     float* dx, void* stream) {
  MMPT_CN_PLANE("unpatchify2_nhwc");
  MMPT_REQUIRE(H % 2 == 0 && W % 2 == 0, "unpatchify2_nhwc: H and W must be even (H %lld, W %lld)",
               (long long)H, (long long)W);
  MMPT_REQUIRE(rows && dx, "unpatchify2_nhwc: null pointer");
  MMPT_REQUIRE(al16(rows) && al16(dx), "unpatchify2_nhwc: pointers must be 16-byte aligned");
  patchify2_kernel<true><<<blocks_for(B * H * W * (C / 8)), 256, 0, (hipStream_t)stream>>>(
      B, (int)H, (int)W, (int)C, (const bf16_t*)rows, nullptr, dx);
  return check_launch("unpatchify2_nhwc");
}
