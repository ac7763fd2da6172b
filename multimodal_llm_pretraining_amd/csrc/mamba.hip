// K22: the Mamba mixer (tf:models/mamba/modeling_mamba.py MambaMixer) — the two recurrent ops the
// reference takes from hand-written CUDA (causal-conv1d and the mamba-ssm selective scan).  The
// five linears around them are GEMMs.
//
// Layout: rows are tokens (b, t), channels contiguous, explicit leading dimensions, so the kernels
// read the in_proj / x_proj GEMM outputs in place.  L is an argument and every index is taken
// inside its own sequence: a tap before t = 0 or a gradient tap past t = L-1 is zero and never
// loaded.
//
// Causal conv: a thread owns 8 channels (16-B accesses) and a strip of CV_S tokens, the four-row
// window kept in registers.  The backward recomputes c from x, forms dc = bf16(du * silu'(c)) (du:
// the fp32 sum of u's two gradients, the scan's and x_proj's) and dx = bf16(conv^T(dc)); dw / db
// are per-workgroup partials summed in workgroup order.
//
// Selective scan: lane = channel, the N states in registers, L cut into chunks of SC_CH tokens so
// the scan is parallel over (b, chunk, channel).  The decay over a chunk is exp(a * Σδ), so
//   forward   1. per chunk: the end state S from h = 0, and Σδ          (scan_fwd_kernel<N, false>)
//             2. a carry over chunks per (b, channel, n): entry states   (scan_carry_kernel)
//             3. per chunk from its entry state: y                       (scan_fwd_kernel<N, true>)
//   backward  the same three steps in reverse for the adjoint of h, then the main pass: for each
//             n it recomputes h_t of the chunk into registers and walks back.  h_{t-1} is always a
//             recomputed value, never h_t divided by the decay.
// Varlen forms (packed rows, T tokens of n_seq sequences laid end to end): the same kernels,
// instantiated with VAR = true.  The conv reads each token's position inside its sequence (pos,
// int32 [T]) and takes a tap only inside the sequence; the scan counts its chunks from each
// sequence's own start, a workgroup finding its sequence by a binary search over the chunk offsets
// (cu_chunks, int32 [n_seq + 1]), and the carries run per sequence.  The per-chunk and per-token
// arithmetic is the dense code, so a sequence's outputs have the bits of a dense run on it alone.
// No atomics: dB / dC (sums over channels) and dA_log / dD / ddt_bias (sums over tokens) are
// per-workgroup partials summed in a fixed order by a second kernel; bitwise reproducible.
#include <algorithm>

#include "common.h"

namespace mmpt {
namespace {

constexpr int CV_S = 16;       // tokens per strip (a multiple of 4: the window rotates by 4)
constexpr int CV_SLOTS = 8;    // strips per workgroup
constexpr int CV_BLOCKS = 256; // partial rows of the weight gradient at most
constexpr int SC_CH = MMPT_SCAN_CHUNK;
constexpr int SC_BLK = 128;    // channels per workgroup

__device__ __forceinline__ void st8f(float* p, const float* f) {
  *(float4*)p = make_float4(f[0], f[1], f[2], f[3]);
  *(float4*)(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
}

// library expf / log1pf (1 and 2 ulp), IEEE division: the tests' bounds count on them
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float silu_f(float x) { return x * sigmoid_f(x); }
__device__ __forceinline__ float silu_grad_f(float x) {
  const float s = sigmoid_f(x);
  return s * (1.0f + x * (1.0f - s));
}
// torch.nn.functional.softplus, beta 1, threshold 20
__device__ __forceinline__ float softplus_f(float x) { return x > 20.0f ? x : log1pf(expf(x)); }

// ------------------------------------------------------------------------------ causal conv
struct ConvArgs {
  int B, L, C, G, spl;         // G = C / 8 lane groups, spl = strips per sequence
  long nstrips;
  const bf16_t* x; long ld_x;
  const bf16_t* w;             // [4][C], tap-major
  const bf16_t* bias;          // [C]
  bf16_t* u; long ld_u;        // fwd
  const bf16_t* du; long ld_du;
  const bf16_t* du2; long ld_du2;  // a second gradient of u, summed in fp32 (nullable)
  bf16_t* dx; long ld_dx;
  float* partials;             // [nb][5][C]
  const int* pos;              // varlen: [L] positions inside the sequences (B = 1, L = T)
};

// c = bf16(Σ_k w[k] * x[l-3+k] + bias); the window slot of position p is p & 3, `i` = l & 3
__device__ __forceinline__ void conv_point(const float (*xr)[8], const float (*wf)[8],
                                           const float* bf, int i, float* c) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) s = fmaf(wf[k][e], xr[(i + 1 + k) & 3][e], s);
    c[e] = round_bf(s + bf[e]);
  }
}

// VAR: a row before the strip is loaded only if it lies in the sequence of the strip's first row
template <bool VAR>
__device__ __forceinline__ void conv_window(const ConvArgs& a, long row0, int s0, int g,
                                            float (*xr)[8]) {
  const int reach = VAR ? a.pos[row0 + s0] : 0;
#pragma unroll
  for (int p = 1; p < 4; ++p) {  // positions s0-4+p; s0 % 4 == 0, so their slots are p
    const int l = s0 - 4 + p;
#pragma unroll
    for (int e = 0; e < 8; ++e) xr[p][e] = 0.f;
    if (l >= 0 && (!VAR || reach >= 4 - p)) unpack8(*(const uint4*)(a.x + (row0 + l) * a.ld_x + g * 8), xr[p]);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) xr[0][e] = 0.f;
}

// VAR: row l (slot i) starts a sequence — the three older rows of the window are not its taps
__device__ __forceinline__ void conv_restart(float (*xr)[8], int i) {
#pragma unroll
  for (int d = 1; d < 4; ++d)
#pragma unroll
    for (int e = 0; e < 8; ++e) xr[(i + d) & 3][e] = 0.f;
}

template <bool VAR>
__global__ __launch_bounds__(256) void causal_conv_fwd_kernel(const ConvArgs a) {
  const int gl = threadIdx.x & 31, slot = threadIdx.x >> 5;
  const int g = blockIdx.x * 32 + gl;
  if (g >= a.G) return;
  float wf[4][8], bf[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) unpack8(*(const uint4*)(a.w + (long)k * a.C + g * 8), wf[k]);
  unpack8(*(const uint4*)(a.bias + g * 8), bf);
  for (long s = (long)blockIdx.y * CV_SLOTS + slot; s < a.nstrips; s += (long)gridDim.y * CV_SLOTS) {
    const int b = (int)(s / a.spl), s0 = (int)(s - (long)b * a.spl) * CV_S;
    const long row0 = (long)b * a.L;
    float xr[4][8];
    conv_window<VAR>(a, row0, s0, g, xr);
#pragma unroll 1
    for (int j = 0; j < CV_S; j += 4) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int l = s0 + j + i;
        if (l < a.L) {
          if (VAR && a.pos[row0 + l] == 0) conv_restart(xr, i);
          unpack8(*(const uint4*)(a.x + (row0 + l) * a.ld_x + g * 8), xr[i]);
          float c[8];
          conv_point(xr, wf, bf, i, c);
#pragma unroll
          for (int e = 0; e < 8; ++e) c[e] = silu_f(c[e]);
          *(uint4*)(a.u + (row0 + l) * a.ld_u + g * 8) = pack8(c);
        }
      }
    }
  }
}

// Sum over the strip slots of a workgroup in slot order; the result is in slot 0's s[]
__device__ __forceinline__ void slot_sum(float (*red)[32][8], int slot, int gl, float* s) {
  __syncthreads();  // the previous call's readers are done
#pragma unroll
  for (int e = 0; e < 8; ++e) red[slot][gl][e] = s[e];
  __syncthreads();
  if (slot == 0)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = red[0][gl][e];
      for (int k = 1; k < CV_SLOTS; ++k) t += red[k][gl][e];
      s[e] = t;
    }
}

template <bool VAR>
__global__ __launch_bounds__(256) void causal_conv_bwd_kernel(const ConvArgs a) {
  __shared__ float red[CV_SLOTS][32][8];
  const int gl = threadIdx.x & 31, slot = threadIdx.x >> 5;
  const int g = blockIdx.x * 32 + gl;
  const bool live = g < a.G;
  float acc[5][8];  // dw[0..3], db
#pragma unroll
  for (int r = 0; r < 5; ++r)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[r][e] = 0.f;
  if (live) {
    float wf[4][8], bf[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) unpack8(*(const uint4*)(a.w + (long)k * a.C + g * 8), wf[k]);
    unpack8(*(const uint4*)(a.bias + g * 8), bf);
    for (long s = (long)blockIdx.y * CV_SLOTS + slot; s < a.nstrips;
         s += (long)gridDim.y * CV_SLOTS) {
      const int b = (int)(s / a.spl), s0 = (int)(s - (long)b * a.spl) * CV_S;
      const long row0 = (long)b * a.L;
      float xr[4][8], dcw[4][8];
      int pw[4] = {0, 0, 0, 0};  // VAR: the positions of the rows whose dc is in the window
      conv_window<VAR>(a, row0, s0, g, xr);
      // dx[t] = Σ_k w[k] * dc[t+3-k] needs dc up to t+3: the walk runs 3 positions past the strip
      // (inside the sequence), and only the strip's own positions feed dw / db.  VAR: dc[t+j]
      // is a tap of dx[t] iff pos[t+j] >= j; a row past the strip that is no tap of the strip's
      // last row is in another sequence and is not loaded.
#pragma unroll 1
      for (int j = 0; j < CV_S + 4; j += 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int l = s0 + j + i;
#pragma unroll
          for (int e = 0; e < 8; ++e) dcw[i][e] = 0.f;
          bool on = l < a.L && j + i < CV_S + 3;
          if (VAR) {
            pw[i] = on ? a.pos[row0 + l] : 0;
            if (j >= CV_S && pw[i] <= j + i - CV_S) on = false;
            if (on && pw[i] == 0) conv_restart(xr, i);
          }
          if (on) {
            unpack8(*(const uint4*)(a.x + (row0 + l) * a.ld_x + g * 8), xr[i]);
            float c[8], d[8];
            conv_point(xr, wf, bf, i, c);
            unpack8(*(const uint4*)(a.du + (row0 + l) * a.ld_du + g * 8), d);
            if (a.du2 != nullptr) {
              float d2[8];
              unpack8(*(const uint4*)(a.du2 + (row0 + l) * a.ld_du2 + g * 8), d2);
#pragma unroll
              for (int e = 0; e < 8; ++e) d[e] += d2[e];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) dcw[i][e] = round_bf(d[e] * silu_grad_f(c[e]));
            if (j < CV_S) {
#pragma unroll
              for (int e = 0; e < 8; ++e) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                  acc[k][e] = fmaf(dcw[i][e], xr[(i + 1 + k) & 3][e], acc[k][e]);
                acc[4][e] += dcw[i][e];
              }
            }
          }
          const int t = l - 3;  // dc[t .. t+3] are in the window
          if (t >= s0 && t < s0 + CV_S && t < a.L) {
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              float v = 0.f;
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const bool tap = !VAR || k == 3 || pw[(i - k) & 3] >= 3 - k;
                v = fmaf(wf[k][e], tap ? dcw[(i - k) & 3][e] : 0.f, v);
              }
              o[e] = v;
            }
            *(uint4*)(a.dx + (row0 + t) * a.ld_dx + g * 8) = pack8(o);
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    slot_sum(red, slot, gl, acc[r]);
    if (slot == 0 && live) st8f(a.partials + ((long)blockIdx.y * 5 + r) * a.C + g * 8, acc[r]);
  }
}

// dw[k][c] += f32(bf16(Σ_n partial)), db[c] likewise, the partials summed in workgroup order
__global__ __launch_bounds__(256) void causal_conv_reduce_kernel(int C, int nb,
                                                                 const float* __restrict__ partials,
                                                                 float* dw, float* db) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= 5L * C) return;
  const int r = (int)(i / C), c = (int)(i - (long)r * C);
  float s = 0.f;
  for (int n = 0; n < nb; ++n) s += partials[((long)n * 5 + r) * C + c];
  s = round_bf(s);
  if (r < 4) dw[(long)r * C + c] += s;
  else db[c] += s;
}

// ------------------------------------------------------------------------------ selective scan
struct ScanArgs {
  int B, L, I, N, chunks, cblocks;
  const bf16_t* u; long ld_u;
  const bf16_t* dt; long ld_dt;
  const bf16_t* Bm; const bf16_t* Cm; long ld_bc;
  const bf16_t* z; long ld_z;
  const float* dt_bias; const float* A_log; const float* D;
  bf16_t* y; long ld_y;
  float* states;               // [B][chunks][I][N]: chunk-entry states
  float* sumd;                 // [B][chunks][I]
  // backward
  const bf16_t* dy; long ld_dy;
  const bf16_t* du_in; long ld_dui;
  bf16_t* du; long ld_du;
  bf16_t* dz; long ld_dz;
  bf16_t* ddt; long ld_ddt;
  bf16_t* dB; bf16_t* dC; long ld_dbc;
  float* dstates;              // [B][chunks][I][N]: the adjoint entering each chunk's end
  float* pbc;                  // [cblocks][B*L][2N]
  float* pch;                  // [B*chunks][N+2][I]
  float* dA_log; float* dD; float* ddt_bias;
  long rows;                   // B * L, or T
  // varlen: chunk c of sequence s is chunk cu_chunks[s] + c of `total`; B = n_seq
  const int* cu_seqlens; const int* cu_chunks;
  int total;
};

// The chunk a workgroup works on: the k-th of its sequence's nk, `len` tokens from row `row0`,
// the gc-th of all (the index of its states / Σδ / partials).
struct Chunk {
  int k, nk, len;
  long gc, row0;
};

// Dense: grid (channel blocks, chunks [- kofs], B).  VAR: grid (channel blocks, y, z) over the
// `total` chunks of all sequences; the sequence is found by a binary search over cu_chunks, the
// same for every lane (scalar loads).  False: no chunk for this workgroup.  The bounds taken from
// the tables are clamped to the buffers' rows, so a bad table cannot send an access outside them.
template <bool VAR>
__device__ __forceinline__ bool scan_chunk_of(const ScanArgs& a, int kofs, Chunk& c) {
  if (!VAR) {
    const int b = blockIdx.z;
    c.k = blockIdx.y + kofs;
    c.nk = a.chunks;
    const int t0 = c.k * SC_CH;
    c.len = min(SC_CH, a.L - t0);
    c.row0 = (long)b * a.L + t0;
    c.gc = (long)b * a.chunks + c.k;
    return true;
  }
  const long gc = (long)blockIdx.z * gridDim.y + blockIdx.y;
  if (gc >= a.total) return false;
  int lo = 0, hi = a.B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.cu_chunks[mid] <= gc) lo = mid;
    else hi = mid;
  }
  const int c0 = a.cu_chunks[lo];
  c.gc = gc;
  c.k = (int)(gc - c0);
  c.nk = a.cu_chunks[lo + 1] - c0;
  c.row0 = (long)a.cu_seqlens[lo] + (long)c.k * SC_CH;
  const long end = min((long)a.cu_seqlens[lo + 1], a.rows);
  c.len = (int)min((long)SC_CH, end - c.row0);
  return c.k >= 0 && c.k < c.nk && c.row0 >= 0 && c.len > 0;
}

// B (and C) of one chunk as fp32 in LDS; rows at and past `len` are zero, never loaded
template <int N>
__device__ __forceinline__ void stage_bc(const bf16_t* src, long ld, long row0, int len,
                                         float (*dst)[N]) {
  for (int i = threadIdx.x; i < SC_CH * (N / 8); i += SC_BLK) {
    const int t = i / (N / 8), q = i - t * (N / 8);
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (t < len) unpack8(*(const uint4*)(src + (row0 + t) * ld + q * 8), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[t][q * 8 + e] = f[e];
  }
}

// OUT = false: from h = 0, the chunk's end state and Σδ.  OUT = true: from the entry state, y.
// (VAR, OUT = false: a sequence's last chunk has no successor to hand a state to)
template <int N, bool OUT, bool VAR>
__global__ __launch_bounds__(SC_BLK) void scan_fwd_kernel(const ScanArgs a) {
  __shared__ float sB[SC_CH][N];
  __shared__ float sC[OUT ? SC_CH : 1][N];
  Chunk c;
  if (!scan_chunk_of<VAR>(a, 0, c) || (VAR && !OUT && c.k == c.nk - 1)) return;
  const int ch = blockIdx.x * SC_BLK + threadIdx.x, k = c.k, len = c.len;
  const long row0 = c.row0;
  stage_bc<N>(a.Bm, a.ld_bc, row0, len, sB);
  if (OUT) stage_bc<N>(a.Cm, a.ld_bc, row0, len, sC);
  __syncthreads();
  if (ch >= a.I) return;
  const long so = (c.gc * a.I + ch) * N;
  float an[N], h[N];
#pragma unroll
  for (int n = 0; n < N; ++n) {
    an[n] = -expf(a.A_log[(long)ch * N + n]);
    h[n] = (OUT && k > 0) ? a.states[so + n] : 0.f;
  }
  const float bias = a.dt_bias[ch], Dv = OUT ? a.D[ch] : 0.f;
  double sd = 0.0;  // Σδ in fp64, rounded once: exp(a * Σδ) then carries two roundings, not len
  for (int t = 0; t < len; ++t) {
    const long row = row0 + t;
    const float dl = softplus_f(bf2f(a.dt[row * a.ld_dt + ch]) + bias);
    const float uv = bf2f(a.u[row * a.ld_u + ch]);
    const float dlu = dl * uv;
    float acc = 0.f;
#pragma unroll
    for (int n = 0; n < N; ++n) {
      h[n] = fmaf(expf(dl * an[n]), h[n], dlu * sB[t][n]);
      if (OUT) acc = fmaf(sC[t][n], h[n], acc);
    }
    if (OUT) {
      const float zv = bf2f(a.z[row * a.ld_z + ch]);
      a.y[row * a.ld_y + ch] = f2bf(fmaf(Dv, uv, acc) * silu_f(zv));
    } else {
      sd += (double)dl;
    }
  }
  if (!OUT) {
#pragma unroll
    for (int n = 0; n < N; n += 4)
      *(float4*)(a.states + so + n) = make_float4(h[n], h[n + 1], h[n + 2], h[n + 3]);
    a.sumd[c.gc * a.I + ch] = (float)sd;
  }
}

// st[k] holds the local end state of chunk k (k < chunks-1); afterwards st[k] is the entry state
// of chunk k: E_0 = 0, E_{k+1} = exp(a Σδ_k) E_k + S_k.  REV: the adjoint, backwards —
// st[k] holds the local entry adjoint of chunk k (k >= 1); afterwards st[k] is the adjoint
// entering chunk k's end: M_last = 0, M_{k-1} = exp(a Σδ_k) M_k + G_k.
// VAR: b is a sequence, its chunks are cu_chunks[b] .. cu_chunks[b+1] of `total`: every carry
// starts from zero at a sequence's start (REV: end) and stops at its end.
template <bool REV, bool VAR>
__global__ __launch_bounds__(256) void scan_carry_kernel(int B, int I, int N, int chunks,
                                                         const float* __restrict__ A_log,
                                                         const float* __restrict__ sumd,
                                                         float* st, const int* cu_chunks,
                                                         int total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * I * N) return;
  const int n = (int)(i % N);
  const long bc = i / N;
  const int ch = (int)(bc % I), b = (int)(bc / I);
  long base = (long)b * chunks;
  if (VAR) {
    base = cu_chunks[b];
    chunks = min(cu_chunks[b + 1], total) - (int)base;
    if (base < 0 || chunks < 1) return;
  }
  const float an = -expf(A_log[(long)ch * N + n]);
  float carry = 0.f;
  for (int j = 0; j < chunks - 1; ++j) {
    const int k = REV ? chunks - 1 - j : j;
    const long o = (base + k) * I + ch;
    const float s = st[o * N + n];
    st[o * N + n] = carry;
    carry = fmaf(expf(an * sumd[o]), carry, s);
  }
  st[((base + (REV ? 0 : chunks - 1)) * I + ch) * N + n] = carry;
}

// The local entry adjoint of a chunk: G_n = Σ_t (Π_{s<=t} α_s) dp_t C_{t,n}, dp = dy silu(z),
// walked from the chunk's end; and Σδ.
// (Chunks 1 .. nk-1 of a sequence: its first chunk has no predecessor to hand an adjoint to.)
template <int N, bool VAR>
__global__ __launch_bounds__(SC_BLK) void scan_bwd_local_kernel(const ScanArgs a) {
  __shared__ float sC[SC_CH][N];
  Chunk c;
  if (!scan_chunk_of<VAR>(a, 1, c) || (VAR && c.k == 0)) return;
  const int ch = blockIdx.x * SC_BLK + threadIdx.x, len = c.len;
  const long row0 = c.row0;
  stage_bc<N>(a.Cm, a.ld_bc, row0, len, sC);
  __syncthreads();
  if (ch >= a.I) return;
  float an[N], gq[N];
#pragma unroll
  for (int n = 0; n < N; ++n) {
    an[n] = -expf(a.A_log[(long)ch * N + n]);
    gq[n] = 0.f;
  }
  const float bias = a.dt_bias[ch];
  double sd = 0.0;
  for (int t = len - 1; t >= 0; --t) {
    const long row = row0 + t;
    const float dl = softplus_f(bf2f(a.dt[row * a.ld_dt + ch]) + bias);
    const float dp = bf2f(a.dy[row * a.ld_dy + ch]) * silu_f(bf2f(a.z[row * a.ld_z + ch]));
#pragma unroll
    for (int n = 0; n < N; ++n) gq[n] = expf(dl * an[n]) * fmaf(dp, sC[t][n], gq[n]);
    sd += (double)dl;
  }
  const long o = c.gc * a.I + ch;
#pragma unroll
  for (int n = 0; n < N; n += 4)
    *(float4*)(a.dstates + o * N + n) = make_float4(gq[n], gq[n + 1], gq[n + 2], gq[n + 3]);
  a.sumd[o] = (float)sd;
}

// The main backward pass of one chunk.  Per-token values (δ, δu, dp) and the accumulators over n
// (q = Σ_n μ B, e = Σ_n μ a α h_{t-1}, p = Σ_n C h) live in registers, statically indexed; steps
// at and past `len` are identity steps (δ = 0, dp = 0, B = C = 0).  For each n: recompute h_t
// forward from the entry state into hs[], then walk back with μ_t = dp_t C_t + α_{t+1} μ_{t+1}.
// The per-channel terms of dB / dC go through an LDS tile and are summed over the workgroup's
// channels in channel order.
template <int N, bool VAR>
__global__ __launch_bounds__(SC_BLK) void scan_bwd_kernel(const ScanArgs a) {
  __shared__ float sB[SC_CH][N];
  __shared__ float sC[SC_CH][N];
  __shared__ float tB[SC_CH][SC_BLK + 1];
  __shared__ float tC[SC_CH][SC_BLK + 1];
  Chunk c;
  if (!scan_chunk_of<VAR>(a, 0, c)) return;
  const int tid = threadIdx.x;
  const int ch = blockIdx.x * SC_BLK + tid, k = c.k, len = c.len;
  const bool live = ch < a.I;
  const long row0 = c.row0;
  stage_bc<N>(a.Bm, a.ld_bc, row0, len, sB);
  stage_bc<N>(a.Cm, a.ld_bc, row0, len, sC);
  float dl[SC_CH], dlu[SC_CH], dpv[SC_CH], q[SC_CH], e[SC_CH], p[SC_CH], hs[SC_CH];
  const float bias = live ? a.dt_bias[ch] : 0.f, Dv = live ? a.D[ch] : 0.f;
#pragma unroll
  for (int t = 0; t < SC_CH; ++t) {
    dl[t] = dlu[t] = dpv[t] = q[t] = e[t] = p[t] = 0.f;
    if (live && t < len) {
      const long row = row0 + t;
      dl[t] = softplus_f(bf2f(a.dt[row * a.ld_dt + ch]) + bias);
      dlu[t] = dl[t] * bf2f(a.u[row * a.ld_u + ch]);
      dpv[t] = bf2f(a.dy[row * a.ld_dy + ch]) * silu_f(bf2f(a.z[row * a.ld_z + ch]));
    }
  }
  __syncthreads();
  const long so = (c.gc * a.I + ch) * N;
  float* pch = a.pch + c.gc * (N + 2) * a.I;
#pragma unroll 1
  for (int n = 0; n < N; ++n) {
    const float an = live ? -expf(a.A_log[(long)ch * N + n]) : 0.f;
    const float h0 = (live && k > 0) ? a.states[so + n] : 0.f;
    float h = h0;
#pragma unroll
    for (int t = 0; t < SC_CH; ++t) {
      h = fmaf(expf(dl[t] * an), h, dlu[t] * sB[t][n]);
      hs[t] = h;
      p[t] = fmaf(sC[t][n], h, p[t]);
      tC[t][tid] = dpv[t] * h;
    }
    float lam = (live && k < c.nk - 1) ? a.dstates[so + n] : 0.f;
    float da = 0.f;
#pragma unroll
    for (int t = SC_CH - 1; t >= 0; --t) {
      const float al = expf(dl[t] * an);
      const float mu = fmaf(dpv[t], sC[t][n], lam);
      const float hp = t > 0 ? hs[t > 0 ? t - 1 : 0] : h0;
      const float wv = mu * al * hp;
      q[t] = fmaf(mu, sB[t][n], q[t]);
      e[t] = fmaf(wv, an, e[t]);
      da = fmaf(wv, dl[t], da);
      tB[t][tid] = mu * dlu[t];
      lam = mu * al;
    }
    if (live) pch[(long)n * a.I + ch] = da * an;
    __syncthreads();
    if (tid < 2 * SC_CH) {
      const int t = tid & (SC_CH - 1);
      const float* src = tid < SC_CH ? tB[t] : tC[t];
      float s = 0.f;
      for (int i = 0; i < SC_BLK; ++i) s += src[i];
      if (t < len)
        a.pbc[((long)blockIdx.x * a.rows + row0 + t) * (2 * N) + (tid < SC_CH ? 0 : N) + n] = s;
    }
    __syncthreads();
  }
  if (!live) return;
  float sD = 0.f, sb = 0.f;
#pragma unroll
  for (int t = 0; t < SC_CH; ++t) {
    if (t < len) {
      const long row = row0 + t;
      const float uv = bf2f(a.u[row * a.ld_u + ch]);
      const float xv = bf2f(a.dt[row * a.ld_dt + ch]) + bias;
      const float zv = bf2f(a.z[row * a.ld_z + ch]);
      const float dyv = bf2f(a.dy[row * a.ld_dy + ch]);
      const float ddl = fmaf(q[t], uv, e[t]);
      const float ddt = ddl * (xv > 20.0f ? 1.0f : sigmoid_f(xv));
      float duv = fmaf(q[t], dl[t], dpv[t] * Dv);
      if (a.du_in != nullptr) duv += bf2f(a.du_in[row * a.ld_dui + ch]);
      a.ddt[row * a.ld_ddt + ch] = f2bf(ddt);
      a.du[row * a.ld_du + ch] = f2bf(duv);
      a.dz[row * a.ld_dz + ch] = f2bf(dyv * fmaf(Dv, uv, p[t]) * silu_grad_f(zv));
      sb += ddt;
      sD = fmaf(dpv[t], uv, sD);
    }
  }
  pch[(long)N * a.I + ch] = sD;
  pch[(long)(N + 1) * a.I + ch] = sb;
}

// dB / dC[row][n] = bf16(Σ_cb partial), channel blocks in order
__global__ __launch_bounds__(256) void scan_reduce_bc_kernel(long rows, int N, int cblocks,
                                                             const float* __restrict__ pbc,
                                                             bf16_t* dB, bf16_t* dC, long ld) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * 2 * N) return;
  const long row = i / (2 * N);
  const int j = (int)(i - row * 2 * N);
  float s = 0.f;
  for (int c = 0; c < cblocks; ++c) s += pbc[(long)c * rows * 2 * N + i];
  if (j < N) dB[row * ld + j] = f2bf(s);
  else dC[row * ld + (j - N)] = f2bf(s);
}

// dA_log[ch][n] += Σ_(b,chunk) partial, dD[ch], ddt_bias[ch] likewise, (b, chunk) in order
__global__ __launch_bounds__(256) void scan_reduce_ch_kernel(int I, int N, int nparts,
                                                             const float* __restrict__ pch,
                                                             float* dA_log, float* dD,
                                                             float* ddt_bias) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)(N + 2) * I) return;
  const int r = (int)(i / I), ch = (int)(i - (long)r * I);
  float s = 0.f;
  for (int j = 0; j < nparts; ++j) s += pch[(long)j * (N + 2) * I + i];
  if (r < N) dA_log[(long)ch * N + r] += s;
  else if (r == N) dD[ch] += s;
  else ddt_bias[ch] += s;
}

inline int64_t up64(int64_t bytes) { return (bytes + 255) / 256 * 256; }

inline bool conv_shape_ok(int64_t B, int64_t L, int64_t C) {
  return B > 0 && L > 0 && C > 0 && C % 8 == 0 && B < ((int64_t)1 << 31) &&
         L < ((int64_t)1 << 31) && B * L < ((int64_t)1 << 31) && C <= 65536;
}
void conv_geometry(ConvArgs& a, int64_t B, int64_t L, int64_t C) {
  a.B = (int)B; a.L = (int)L; a.C = (int)C; a.G = (int)(C / 8);
  a.spl = (int)((L + CV_S - 1) / CV_S);
  a.nstrips = B * a.spl;
}
inline int64_t conv_nb(const ConvArgs& a, int64_t cap) {
  return std::max<int64_t>(1, std::min<int64_t>(cap, (a.nstrips + CV_SLOTS - 1) / CV_SLOTS));
}

inline bool scan_shape_ok(int64_t B, int64_t L, int64_t I, int64_t N) {
  return B > 0 && B <= 65535 && L > 0 && I > 0 && I % 8 == 0 && (N == 8 || N == 16) &&
         L < ((int64_t)1 << 31) && B * L < ((int64_t)1 << 31) && I < ((int64_t)1 << 24) &&
         (L + SC_CH - 1) / SC_CH <= 65535;
}
inline int64_t scan_chunks(int64_t L) { return (L + SC_CH - 1) / SC_CH; }
inline int64_t scan_cblocks(int64_t I) { return (I + SC_BLK - 1) / SC_BLK; }

// Varlen: T tokens in n_seq sequences of at least one token, `total` chunks in all
// (Σ ceil(len / chunk), which the tables on the device must agree with).
inline bool scan_varlen_ok(int64_t T, int64_t n_seq, int64_t total, int64_t I, int64_t N) {
  return n_seq > 0 && n_seq <= 65535 && T >= n_seq && T < ((int64_t)1 << 31) && I > 0 &&
         I % 8 == 0 && I < ((int64_t)1 << 24) && (N == 8 || N == 16) &&
         total >= std::max(n_seq, scan_chunks(T)) && total <= std::min(T, T / SC_CH + n_seq);
}

// The launch sequences, dense (grid y = chunks, z = B) and varlen (y, z over all chunks).  nseq:
// the sequences the carries run over; nch: every chunk; multi: some sequence has two chunks.
template <bool VAR>
inline dim3 scan_grid(const ScanArgs& a, int drop) {
  if (!VAR) return dim3((unsigned)a.cblocks, (unsigned)(a.chunks - drop), (unsigned)a.B);
  const unsigned gy = (unsigned)std::min(a.total, 65535);
  return dim3((unsigned)a.cblocks, gy, (unsigned)((a.total + gy - 1) / gy));
}

template <bool VAR>
int scan_fwd_launch(const ScanArgs& a, const char* what, hipStream_t s) {
  const bool multi = VAR ? a.total > a.B : a.chunks > 1;
  int rc;
  if (multi) {
    const dim3 lgrid = scan_grid<VAR>(a, 1);
    if (a.N == 16) scan_fwd_kernel<16, false, VAR><<<lgrid, SC_BLK, 0, s>>>(a);
    else scan_fwd_kernel<8, false, VAR><<<lgrid, SC_BLK, 0, s>>>(a);
    if ((rc = check_launch(what))) return rc;
    scan_carry_kernel<false, VAR><<<(unsigned)(((int64_t)a.B * a.I * a.N + 255) / 256), 256, 0, s>>>(
        a.B, a.I, a.N, a.chunks, a.A_log, a.sumd, a.states, a.cu_chunks, a.total);
    if ((rc = check_launch(what))) return rc;
  }
  const dim3 grid = scan_grid<VAR>(a, 0);
  if (a.N == 16) scan_fwd_kernel<16, true, VAR><<<grid, SC_BLK, 0, s>>>(a);
  else scan_fwd_kernel<8, true, VAR><<<grid, SC_BLK, 0, s>>>(a);
  return check_launch(what);
}

template <bool VAR>
int scan_bwd_launch(const ScanArgs& a, const char* what, hipStream_t s) {
  const bool multi = VAR ? a.total > a.B : a.chunks > 1;
  const int64_t nch = VAR ? a.total : (int64_t)a.B * a.chunks;
  int rc;
  if (multi) {
    const dim3 lgrid = scan_grid<VAR>(a, 1);
    if (a.N == 16) scan_bwd_local_kernel<16, VAR><<<lgrid, SC_BLK, 0, s>>>(a);
    else scan_bwd_local_kernel<8, VAR><<<lgrid, SC_BLK, 0, s>>>(a);
    if ((rc = check_launch(what))) return rc;
    scan_carry_kernel<true, VAR><<<(unsigned)(((int64_t)a.B * a.I * a.N + 255) / 256), 256, 0, s>>>(
        a.B, a.I, a.N, a.chunks, a.A_log, a.sumd, a.dstates, a.cu_chunks, a.total);
    if ((rc = check_launch(what))) return rc;
  }
  const dim3 grid = scan_grid<VAR>(a, 0);
  if (a.N == 16) scan_bwd_kernel<16, VAR><<<grid, SC_BLK, 0, s>>>(a);
  else scan_bwd_kernel<8, VAR><<<grid, SC_BLK, 0, s>>>(a);
  if ((rc = check_launch(what))) return rc;
  scan_reduce_bc_kernel<<<(unsigned)((a.rows * 2 * a.N + 255) / 256), 256, 0, s>>>(
      a.rows, a.N, a.cblocks, a.pbc, a.dB, a.dC, a.ld_dbc);
  if ((rc = check_launch(what))) return rc;
  scan_reduce_ch_kernel<<<(unsigned)(((a.N + 2) * (int64_t)a.I + 255) / 256), 256, 0, s>>>(
      a.I, a.N, (int)nch, a.pch, a.dA_log, a.dD, a.ddt_bias);
  return check_launch(what);
}

}  // namespace
}  // namespace mmpt

using namespace mmpt;

#define MMPT_MB_CONV(what)                                                                       \
  MMPT_REQUIRE(conv_shape_ok(B, L, C),                                                           \
               what ": B, L >= 1 with B*L < 2^31, C a positive multiple of 8 and <= 65536 "     \
                    "(B %lld, L %lld, C %lld)", (long long)B, (long long)L, (long long)C);       \
  MMPT_REQUIRE(K == 4, what ": K must be 4 (K %lld)", (long long)K)
#define MMPT_MB_SCAN(what)                                                                        \
  MMPT_REQUIRE(scan_shape_ok(B, L, I, N),                                                         \
               what ": B in [1, 65535], L >= 1 with B*L < 2^31 and at most 65535 chunks, I a "   \
                    "positive multiple of 8, N 8 or 16 (B %lld, L %lld, I %lld, N %lld)",        \
               (long long)B, (long long)L, (long long)I, (long long)N)

extern "C" int64_t mmpt_selective_scan_chunk(void) { return SC_CH; }

// The dense entries and the varlen ones (pos != nullptr: B = 1, L = T) share everything below
// their argument lists.
#define MMPT_MB_POS(what)                                                                        \
  MMPT_REQUIRE(pos != nullptr && al4(pos), what ": pos must be a 4-byte aligned int32 [T] table")

static int conv_fwd(const char* what, int64_t B, int64_t L, int64_t C, const void* pos,
                    const void* x, int64_t ld_x, const void* w, const void* bias, void* u,
                    int64_t ld_u, void* stream) {
  MMPT_REQUIRE(ld_x >= C && ld_x % 8 == 0 && ld_u >= C && ld_u % 8 == 0,
               "%s: ld_x and ld_u must be multiples of 8 and >= C", what);
  MMPT_REQUIRE(x && w && bias && u, "%s: null pointer", what);
  MMPT_REQUIRE(al16(x) && al16(w) && al16(bias) && al16(u),
               "%s: pointers must be 16-byte aligned", what);
  ConvArgs a = {};
  conv_geometry(a, B, L, C);
  a.x = (const bf16_t*)x; a.ld_x = ld_x; a.w = (const bf16_t*)w; a.bias = (const bf16_t*)bias;
  a.u = (bf16_t*)u; a.ld_u = ld_u; a.pos = (const int*)pos;
  const dim3 grid((unsigned)((a.G + 31) / 32), (unsigned)conv_nb(a, 65535));
  if (pos) causal_conv_fwd_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  else causal_conv_fwd_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  return check_launch(what);
}

extern "C" int mmpt_causal_conv1d_fwd(int64_t B, int64_t L, int64_t C, int64_t K, const void* x,
                                      int64_t ld_x, const void* w, const void* bias, void* u,
                                      int64_t ld_u, void* stream) {
  MMPT_MB_CONV("causal_conv1d_fwd");
  return conv_fwd("causal_conv1d_fwd", B, L, C, nullptr, x, ld_x, w, bias, u, ld_u, stream);
}

extern "C" int mmpt_causal_conv1d_varlen_fwd(int64_t T, int64_t C, int64_t K, const void* pos,
                                             const void* x, int64_t ld_x, const void* w,
                                             const void* bias, void* u, int64_t ld_u,
                                             void* stream) {
  const int64_t B = 1, L = T;
  MMPT_MB_CONV("causal_conv1d_varlen_fwd");
  MMPT_MB_POS("causal_conv1d_varlen_fwd");
  return conv_fwd("causal_conv1d_varlen_fwd", B, L, C, pos, x, ld_x, w, bias, u, ld_u, stream);
}

extern "C" int64_t mmpt_causal_conv1d_bwd_workspace_bytes(int64_t B, int64_t L, int64_t C) {
  if (!conv_shape_ok(B, L, C)) return 0;
  ConvArgs a = {};
  conv_geometry(a, B, L, C);
  return conv_nb(a, CV_BLOCKS) * 5 * C * (int64_t)sizeof(float);
}

static int conv_bwd(const char* what, int64_t B, int64_t L, int64_t C, const void* pos,
                    const void* x, int64_t ld_x, const void* w, const void* bias, const void* du,
                    int64_t ld_du, const void* du2, int64_t ld_du2, void* dx, int64_t ld_dx,
                    float* dw, float* db, void* workspace, void* stream) {
  MMPT_REQUIRE(ld_x >= C && ld_x % 8 == 0 && ld_du >= C && ld_du % 8 == 0 && ld_dx >= C &&
                   ld_dx % 8 == 0 && (du2 == nullptr || (ld_du2 >= C && ld_du2 % 8 == 0)),
               "%s: ld_x, ld_du, ld_du2 and ld_dx must be multiples of 8 and >= C", what);
  MMPT_REQUIRE(x && w && bias && du && dx && dw && db && workspace, "%s: null pointer", what);
  MMPT_REQUIRE(al16(x) && al16(w) && al16(bias) && al16(du) && al16(du2) && al16(dx) && al16(dw) &&
                   al16(db) && al16(workspace),
               "%s: pointers must be 16-byte aligned", what);
  ConvArgs a = {};
  conv_geometry(a, B, L, C);
  a.x = (const bf16_t*)x; a.ld_x = ld_x; a.w = (const bf16_t*)w; a.bias = (const bf16_t*)bias;
  a.du = (const bf16_t*)du; a.ld_du = ld_du; a.du2 = (const bf16_t*)du2; a.ld_du2 = ld_du2;
  a.dx = (bf16_t*)dx; a.ld_dx = ld_dx;
  a.partials = (float*)workspace; a.pos = (const int*)pos;
  const int nb = (int)conv_nb(a, CV_BLOCKS);
  const dim3 grid((unsigned)((a.G + 31) / 32), (unsigned)nb);
  if (pos) causal_conv_bwd_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  else causal_conv_bwd_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  int rc = check_launch(what);
  if (rc) return rc;
  causal_conv_reduce_kernel<<<(unsigned)((5 * C + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (int)C, nb, a.partials, dw, db);
  return check_launch(what);
}

extern "C" int mmpt_causal_conv1d_bwd(int64_t B, int64_t L, int64_t C, int64_t K, const void* x,
                                      int64_t ld_x, const void* w, const void* bias,
                                      const void* du, int64_t ld_du, const void* du2,
                                      int64_t ld_du2, void* dx, int64_t ld_dx, float* dw,
                                      float* db, void* workspace, void* stream) {
  MMPT_MB_CONV("causal_conv1d_bwd");
  return conv_bwd("causal_conv1d_bwd", B, L, C, nullptr, x, ld_x, w, bias, du, ld_du, du2, ld_du2,
                  dx, ld_dx, dw, db, workspace, stream);
}

extern "C" int64_t mmpt_causal_conv1d_varlen_bwd_workspace_bytes(int64_t T, int64_t C) {
  return mmpt_causal_conv1d_bwd_workspace_bytes(1, T, C);
}

extern "C" int mmpt_causal_conv1d_varlen_bwd(int64_t T, int64_t C, int64_t K, const void* pos,
                                             const void* x, int64_t ld_x, const void* w,
                                             const void* bias, const void* du, int64_t ld_du,
                                             const void* du2, int64_t ld_du2, void* dx,
                                             int64_t ld_dx, float* dw, float* db, void* workspace,
                                             void* stream) {
  const int64_t B = 1, L = T;
  MMPT_MB_CONV("causal_conv1d_varlen_bwd");
  MMPT_MB_POS("causal_conv1d_varlen_bwd");
  return conv_bwd("causal_conv1d_varlen_bwd", B, L, C, pos, x, ld_x, w, bias, du, ld_du, du2,
                  ld_du2, dx, ld_dx, dw, db, workspace, stream);
}

extern "C" int64_t mmpt_selective_scan_states_bytes(int64_t B, int64_t L, int64_t I, int64_t N) {
  if (!scan_shape_ok(B, L, I, N)) return 0;
  return B * scan_chunks(L) * I * N * (int64_t)sizeof(float);
}

extern "C" int64_t mmpt_selective_scan_fwd_workspace_bytes(int64_t B, int64_t L, int64_t I,
                                                           int64_t N) {
  if (!scan_shape_ok(B, L, I, N)) return 0;
  return up64(B * scan_chunks(L) * I * (int64_t)sizeof(float)) +
         mmpt_selective_scan_states_bytes(B, L, I, N);
}

// The geometry of a scan call: dense (B sequences of L rows, cu_chunks null) or varlen (B = n_seq
// sequences over `rows` = T rows, `nch` = total chunks, the two device tables).
struct ScanGeo {
  int64_t B, L, rows, nch;
  const void* cu_seqlens;
  const void* cu_chunks;
};
static void scan_geometry(ScanArgs& a, const ScanGeo& g, int64_t I, int64_t N) {
  a.B = (int)g.B; a.L = (int)g.L; a.I = (int)I; a.N = (int)N;
  a.chunks = g.cu_chunks ? 0 : (int)scan_chunks(g.L);
  a.cblocks = (int)scan_cblocks(I);
  a.rows = g.rows; a.total = (int)g.nch;
  a.cu_seqlens = (const int*)g.cu_seqlens; a.cu_chunks = (const int*)g.cu_chunks;
}
#define MMPT_MB_VARLEN(what)                                                                      \
  MMPT_REQUIRE(scan_varlen_ok(T, n_seq, total_chunks, I, N),                                      \
               what ": n_seq in [1, 65535], n_seq <= T < 2^31, total_chunks the sum of "         \
                    "ceil(len / chunk), I a positive multiple of 8, N 8 or 16 (T %lld, n_seq "   \
                    "%lld, total_chunks %lld, I %lld, N %lld)", (long long)T, (long long)n_seq,   \
               (long long)total_chunks, (long long)I, (long long)N);                              \
  MMPT_REQUIRE(cu_seqlens && cu_chunks && al4(cu_seqlens) && al4(cu_chunks),                      \
               what ": cu_seqlens and cu_chunks must be 4-byte aligned int32 [n_seq + 1] tables")

static int scan_fwd(const char* what, const ScanGeo& g, int64_t I, int64_t N, const void* u,
                    int64_t ld_u, const void* dt_raw, int64_t ld_dt, const float* dt_bias,
                    const float* A_log, const void* Bm, const void* Cm, int64_t ld_bc,
                    const float* D, const void* z, int64_t ld_z, void* y, int64_t ld_y,
                    float* states, void* workspace, void* stream) {
  MMPT_REQUIRE(ld_u >= I && ld_dt >= I && ld_z >= I && ld_y >= I,
               "%s: ld_u, ld_dt, ld_z, ld_y must be >= I", what);
  MMPT_REQUIRE(ld_bc >= N && ld_bc % 8 == 0, "%s: ld_bc must be a multiple of 8 and >= N", what);
  MMPT_REQUIRE(u && dt_raw && dt_bias && A_log && Bm && Cm && D && z && y && workspace,
               "%s: null pointer", what);
  MMPT_REQUIRE(al16(Bm) && al16(Cm) && al16(A_log) && al16(states) && al16(workspace) &&
                   al4(dt_bias) && al4(D),
               "%s: B, C, A_log, states and the workspace must be 16-byte aligned", what);
  MMPT_REQUIRE((((uintptr_t)u | (uintptr_t)dt_raw | (uintptr_t)z | (uintptr_t)y) & 1) == 0,
               "%s: bf16 pointers must be 2-byte aligned", what);
  ScanArgs a = {};
  scan_geometry(a, g, I, N);
  a.u = (const bf16_t*)u; a.ld_u = ld_u; a.dt = (const bf16_t*)dt_raw; a.ld_dt = ld_dt;
  a.Bm = (const bf16_t*)Bm; a.Cm = (const bf16_t*)Cm; a.ld_bc = ld_bc;
  a.z = (const bf16_t*)z; a.ld_z = ld_z; a.dt_bias = dt_bias; a.A_log = A_log; a.D = D;
  a.y = (bf16_t*)y; a.ld_y = ld_y;
  a.sumd = (float*)workspace;
  a.states = states ? states
                    : (float*)((char*)workspace + up64(g.nch * I * (int64_t)sizeof(float)));
  return g.cu_chunks ? scan_fwd_launch<true>(a, what, (hipStream_t)stream)
                     : scan_fwd_launch<false>(a, what, (hipStream_t)stream);
}

extern "C" int mmpt_selective_scan_fwd(int64_t B, int64_t L, int64_t I, int64_t N, const void* u,
                                       int64_t ld_u, const void* dt_raw, int64_t ld_dt,
                                       const float* dt_bias, const float* A_log, const void* Bm,
                                       const void* Cm, int64_t ld_bc, const float* D,
                                       const void* z, int64_t ld_z, void* y, int64_t ld_y,
                                       float* states, void* workspace, void* stream) {
  MMPT_MB_SCAN("selective_scan_fwd");
  const ScanGeo g = {B, L, B * L, B * scan_chunks(L), nullptr, nullptr};
  return scan_fwd("selective_scan_fwd", g, I, N, u, ld_u, dt_raw, ld_dt, dt_bias, A_log, Bm, Cm,
                  ld_bc, D, z, ld_z, y, ld_y, states, workspace, stream);
}

extern "C" int64_t mmpt_selective_scan_varlen_states_bytes(int64_t total_chunks, int64_t I,
                                                           int64_t N) {
  if (total_chunks <= 0 || total_chunks >= ((int64_t)1 << 31) || I <= 0 || I % 8 ||
      I >= ((int64_t)1 << 24) || (N != 8 && N != 16))
    return 0;
  return total_chunks * I * N * (int64_t)sizeof(float);
}

extern "C" int64_t mmpt_selective_scan_varlen_fwd_workspace_bytes(int64_t total_chunks, int64_t I,
                                                                  int64_t N) {
  const int64_t st = mmpt_selective_scan_varlen_states_bytes(total_chunks, I, N);
  return st ? up64(total_chunks * I * (int64_t)sizeof(float)) + st : 0;
}

extern "C" int mmpt_selective_scan_varlen_fwd(int64_t T, int64_t n_seq, int64_t total_chunks,
                                              const void* cu_seqlens, const void* cu_chunks,
                                              int64_t I, int64_t N, const void* u, int64_t ld_u,
                                              const void* dt_raw, int64_t ld_dt,
                                              const float* dt_bias, const float* A_log,
                                              const void* Bm, const void* Cm, int64_t ld_bc,
                                              const float* D, const void* z, int64_t ld_z, void* y,
                                              int64_t ld_y, float* states, void* workspace,
                                              void* stream) {
  MMPT_MB_VARLEN("selective_scan_varlen_fwd");
  const ScanGeo g = {n_seq, 0, T, total_chunks, cu_seqlens, cu_chunks};
  return scan_fwd("selective_scan_varlen_fwd", g, I, N, u, ld_u, dt_raw, ld_dt, dt_bias, A_log, Bm,
                  Cm, ld_bc, D, z, ld_z, y, ld_y, states, workspace, stream);
}

extern "C" int64_t mmpt_selective_scan_bwd_workspace_bytes(int64_t B, int64_t L, int64_t I,
                                                           int64_t N) {
  if (!scan_shape_ok(B, L, I, N)) return 0;
  const int64_t chunks = scan_chunks(L), f = (int64_t)sizeof(float);
  return up64(B * chunks * I * f) + up64(B * chunks * I * N * f) +
         up64(scan_cblocks(I) * B * L * 2 * N * f) + up64(B * chunks * (N + 2) * I * f);
}

static int scan_bwd(const char* what, const ScanGeo& g, int64_t I, int64_t N, const void* u,
                    int64_t ld_u, const void* dt_raw, int64_t ld_dt, const float* dt_bias,
                    const float* A_log, const void* Bm, const void* Cm, int64_t ld_bc,
                    const float* D, const void* z, int64_t ld_z, const float* states,
                    const void* dy, int64_t ld_dy, const void* du_in, int64_t ld_du_in, void* du,
                    int64_t ld_du, void* dz, int64_t ld_dz, void* ddt_raw, int64_t ld_ddt,
                    void* dB, void* dC, int64_t ld_dbc, float* dA_log, float* dD, float* ddt_bias,
                    void* workspace, void* stream) {
  MMPT_REQUIRE(ld_u >= I && ld_dt >= I && ld_z >= I && ld_dy >= I && ld_du >= I && ld_dz >= I &&
                   ld_ddt >= I && (du_in == nullptr || ld_du_in >= I),
               "%s: every channel leading dimension must be >= I", what);
  MMPT_REQUIRE(ld_bc >= N && ld_bc % 8 == 0, "%s: ld_bc must be a multiple of 8 and >= N", what);
  MMPT_REQUIRE(ld_dbc >= N, "%s: ld_dbc must be >= N", what);
  MMPT_REQUIRE(u && dt_raw && dt_bias && A_log && Bm && Cm && D && z && dy && du && dz &&
                   ddt_raw && dB && dC && dA_log && dD && ddt_bias && workspace,
               "%s: null pointer", what);
  MMPT_REQUIRE(g.nch == g.B || states != nullptr,
               "%s: more than one chunk in a sequence needs the forward's states", what);
  MMPT_REQUIRE(al16(Bm) && al16(Cm) && al16(A_log) && al16(states) && al16(workspace) &&
                   al4(dt_bias) && al4(D) && al4(dA_log) && al4(dD) && al4(ddt_bias),
               "%s: B, C, A_log, states and the workspace must be 16-byte aligned", what);
  MMPT_REQUIRE((((uintptr_t)u | (uintptr_t)dt_raw | (uintptr_t)z | (uintptr_t)dy |
                 (uintptr_t)du_in | (uintptr_t)du | (uintptr_t)dz | (uintptr_t)ddt_raw |
                 (uintptr_t)dB | (uintptr_t)dC) & 1) == 0,
               "%s: bf16 pointers must be 2-byte aligned", what);
  ScanArgs a = {};
  scan_geometry(a, g, I, N);
  a.u = (const bf16_t*)u; a.ld_u = ld_u; a.dt = (const bf16_t*)dt_raw; a.ld_dt = ld_dt;
  a.Bm = (const bf16_t*)Bm; a.Cm = (const bf16_t*)Cm; a.ld_bc = ld_bc;
  a.z = (const bf16_t*)z; a.ld_z = ld_z; a.dt_bias = dt_bias; a.A_log = A_log; a.D = D;
  a.states = (float*)states;
  a.dy = (const bf16_t*)dy; a.ld_dy = ld_dy; a.du_in = (const bf16_t*)du_in; a.ld_dui = ld_du_in;
  a.du = (bf16_t*)du; a.ld_du = ld_du; a.dz = (bf16_t*)dz; a.ld_dz = ld_dz;
  a.ddt = (bf16_t*)ddt_raw; a.ld_ddt = ld_ddt; a.dB = (bf16_t*)dB; a.dC = (bf16_t*)dC;
  a.ld_dbc = ld_dbc; a.dA_log = dA_log; a.dD = dD; a.ddt_bias = ddt_bias;
  const int64_t f = (int64_t)sizeof(float);
  char* ws = (char*)workspace;
  a.sumd = (float*)ws; ws += up64(g.nch * I * f);
  a.dstates = (float*)ws; ws += up64(g.nch * I * N * f);
  a.pbc = (float*)ws; ws += up64((int64_t)a.cblocks * g.rows * 2 * N * f);
  a.pch = (float*)ws;
  return g.cu_chunks ? scan_bwd_launch<true>(a, what, (hipStream_t)stream)
                     : scan_bwd_launch<false>(a, what, (hipStream_t)stream);
}

extern "C" int mmpt_selective_scan_bwd(int64_t B, int64_t L, int64_t I, int64_t N, const void* u,
                                       int64_t ld_u, const void* dt_raw, int64_t ld_dt,
                                       const float* dt_bias, const float* A_log, const void* Bm,
                                       const void* Cm, int64_t ld_bc, const float* D,
                                       const void* z, int64_t ld_z, const float* states,
                                       const void* dy, int64_t ld_dy, const void* du_in,
                                       int64_t ld_du_in, void* du, int64_t ld_du, void* dz,
                                       int64_t ld_dz, void* ddt_raw, int64_t ld_ddt, void* dB,
                                       void* dC, int64_t ld_dbc, float* dA_log, float* dD,
                                       float* ddt_bias, void* workspace, void* stream) {
  MMPT_MB_SCAN("selective_scan_bwd");
  const ScanGeo g = {B, L, B * L, B * scan_chunks(L), nullptr, nullptr};
  return scan_bwd("selective_scan_bwd", g, I, N, u, ld_u, dt_raw, ld_dt, dt_bias, A_log, Bm, Cm,
                  ld_bc, D, z, ld_z, states, dy, ld_dy, du_in, ld_du_in, du, ld_du, dz, ld_dz,
                  ddt_raw, ld_ddt, dB, dC, ld_dbc, dA_log, dD, ddt_bias, workspace, stream);
}

extern "C" int64_t mmpt_selective_scan_varlen_bwd_workspace_bytes(int64_t T, int64_t total_chunks,
                                                                  int64_t I, int64_t N) {
  if (!mmpt_selective_scan_varlen_states_bytes(total_chunks, I, N) || T < total_chunks ||
      T >= ((int64_t)1 << 31))
    return 0;
  const int64_t f = (int64_t)sizeof(float);
  return up64(total_chunks * I * f) + up64(total_chunks * I * N * f) +
         up64(scan_cblocks(I) * T * 2 * N * f) + up64(total_chunks * (N + 2) * I * f);
}

extern "C" int mmpt_selective_scan_varlen_bwd(int64_t T, int64_t n_seq, int64_t total_chunks,
                                              const void* cu_seqlens, const void* cu_chunks,
                                              int64_t I, int64_t N, const void* u, int64_t ld_u,
                                              const void* dt_raw, int64_t ld_dt,
                                              const float* dt_bias, const float* A_log,
                                              const void* Bm, const void* Cm, int64_t ld_bc,
                                              const float* D, const void* z, int64_t ld_z,
                                              const float* states, const void* dy, int64_t ld_dy,
                                              const void* du_in, int64_t ld_du_in, void* du,
                                              int64_t ld_du, void* dz, int64_t ld_dz,
                                              void* ddt_raw, int64_t ld_ddt, void* dB, void* dC,
                                              int64_t ld_dbc, float* dA_log, float* dD,
                                              float* ddt_bias, void* workspace, void* stream) {
  MMPT_MB_VARLEN("selective_scan_varlen_bwd");
  const ScanGeo g = {n_seq, 0, T, total_chunks, cu_seqlens, cu_chunks};
  return scan_bwd("selective_scan_varlen_bwd", g, I, N, u, ld_u, dt_raw, ld_dt, dt_bias, A_log, Bm,
                  Cm, ld_bc, D, z, ld_z, states, dy, ld_dy, du_in, ld_du_in, du, ld_du, dz, ld_dz,
                  ddt_raw, ld_ddt, dB, dC, ld_dbc, dA_log, dD, ddt_bias, workspace, stream);
}
