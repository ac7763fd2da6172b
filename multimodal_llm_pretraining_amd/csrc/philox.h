// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel Random Numbers: As Easy as 1, 2, 3",
// SC'11; the Random123 constants), host and device: the counter-based generator behind the
// hidden-dropout kernels (dropout.hip) and the attention-probability dropout of the
// flash-attention kernels (attention.hip; the addressing further down), and the embedding noise
// of the gather kernels (misc.hip, postln.hip).  A stand-alone header (no HIP include) so that a plain
// C++ program can check it against the published known answers.
//
// The dropout addressing (include/mmpt.h "K16"): logical element e = row*h + col of a
// dropout site draws output word e % 4 of
//   philox4x32_10(counter = {lo32(e/4), hi32(e/4), lo32(site), hi32(site)},
//                 key     = {lo32(seed), hi32(seed)})
// and is kept iff word >= floor(p * 2^32) (dropout_threshold, host arithmetic in double).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MMPT_PHILOX_HD __host__ __device__ inline
#else
#define MMPT_PHILOX_HD inline
#endif

namespace mmpt {

struct philox4 {
  uint32_t w[4];
};

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

MMPT_PHILOX_HD philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                     uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += PHILOX_W0;  // the key schedule (the bump after the last round is unused)
    k1 += PHILOX_W1;
  }
  return philox4{{c0, c1, c2, c3}};
}

// The four words of elements 4*q .. 4*q + 3 of dropout site `site` under `seed`.
MMPT_PHILOX_HD philox4 dropout_words(uint64_t q, uint64_t site, uint64_t seed) {
  return philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)site, (uint32_t)(site >> 32),
                       (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Host side of the keep rule: keep iff word >= floor(p * 2^32), 0 <= p < 1 (p = 0 keeps all).
inline uint32_t dropout_threshold(double p) { return (uint32_t)(uint64_t)(p * 4294967296.0); }
// 1 / (1 - p) rounded once to fp32: the factor kept elements are multiplied by.
inline float dropout_scale(double p) { return (float)(1.0 / (1.0 - p)); }

// ---- embedding noise (NEFTune; include/mmpt.h "K8") ----
// Logical element e = row*h + col of noise site `site` takes word e % 4 of
// dropout_words(e / 4, site, seed) (the hidden-dropout addressing) and adds
//   noise = fmul_rn(s, mag),   s = (float)(2k + 1) * 2^-23 - 1,   k = word >> 9 (23 bits)
// to its value: out = fadd_rn(value, noise), two separately rounded fp32 operations (never one
// fma, so a numpy float32 restatement gives the same bits).  2k + 1 < 2^24 converts exactly,
// the scaling by 2^-23 and the subtraction are exact, so s is an odd multiple of 2^-23 in
// (-1, 1): symmetric about 0 and never 0.
// Contraction is switched off where the two operations meet (hipcc honours the pragma under its
// default -ffp-contract; HIP's __fmul_rn / __fadd_rn are plain operators without OCML's rounded
// operations and would be fused).
// s of one Philox word
MMPT_PHILOX_HD float embed_noise_unit(uint32_t word) {
  return (float)(int32_t)(2u * (word >> 9) + 1u) * 1.1920928955078125e-07f - 1.0f;
}
// noise = fmul_rn(s, mag) for one word
MMPT_PHILOX_HD float embed_noise_of(uint32_t word, float mag) {
#if defined(__clang__)
#pragma clang fp contract(off)
  return embed_noise_unit(word) * mag;
#else
  volatile float r = embed_noise_unit(word) * mag;  // rounded here, whatever the flags
  return r;
#endif
}
// value + noise for one word
MMPT_PHILOX_HD float embed_noise_add(float value, uint32_t word, float mag) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float n = embed_noise_of(word, mag);
  return value + n;
}
// The noise of logical element e alone (the tests' and mmpt_embed_noise's view).
MMPT_PHILOX_HD float embed_noise_at(uint64_t e, uint64_t site, uint64_t seed, float mag) {
  return embed_noise_of(dropout_words(e >> 2, site, seed).w[e & 3], mag);
}
// Host side: mag = alpha / sqrt(seq_in * hidden) in double, rounded once to fp32.
inline float embed_noise_mag(double alpha, int64_t seq_in, int64_t hidden) {
  return (float)(alpha / __builtin_sqrt((double)seq_in * (double)hidden));
}

// ---- attention-probability dropout (include/mmpt.h "K19") ----
// The keep bit of probability (batch b, query head h, query position q, key position k) — positions
// inside their sequence — is one byte of a 4 x 4 block (4 queries x 4 keys) drawn by one call:
//   W = philox4x32_10(ctr = {(q>>2) | ((k>>2) << 16), b*heads + h, lo32(site), hi32(site)},
//                     key = {lo32(seed), hi32(seed)})
//   byte = (W.w[q & 3] >> (8 * (k & 3))) & 0xFF,   keep iff byte >= t8 = floor(p * 256)
// so a lane holding 4 consecutive keys of one query (forward, dQ) and a lane holding 4 consecutive
// queries of one key (dK/dV) both pay one call per 4 elements.
constexpr int64_t ATTN_DROPOUT_MAX_SEQ = 262144;  // q >> 2 and k >> 2 are 16 bits each

// The words of the block (q >> 2, k >> 2) = (qb, kb) of batch-head bh = b*heads + h.
MMPT_PHILOX_HD philox4 attn_dropout_words(uint32_t qb, uint32_t kb, uint32_t bh, uint64_t site,
                                          uint64_t seed) {
  return philox4x32_10(qb | (kb << 16), bh, (uint32_t)site, (uint32_t)(site >> 32), (uint32_t)seed,
                       (uint32_t)(seed >> 32));
}
// The keep bit of (q, k) given its block's words.
MMPT_PHILOX_HD bool attn_dropout_keep(const philox4& w, uint32_t q, uint32_t k, uint32_t t8) {
  return ((w.w[q & 3] >> (8 * (k & 3))) & 0xFFu) >= t8;
}
MMPT_PHILOX_HD bool attn_dropout_keep_at(uint32_t q, uint32_t k, uint32_t bh, uint64_t site,
                                         uint64_t seed, uint32_t t8) {
  return attn_dropout_keep(attn_dropout_words(q >> 2, k >> 2, bh, site, seed), q, k, t8);
}
// Host side: the 8-bit threshold, the probability it realises, and the fp32 factor of the kept
// probabilities (from p_eff, so the estimator stays unbiased).  t8 == 0 (p < 1/256) is p = 0.
inline uint32_t attn_dropout_t8(double p) { return (uint32_t)(p * 256.0); }
inline double attn_dropout_p_eff(double p) { return attn_dropout_t8(p) / 256.0; }
inline float attn_dropout_scale(double p) { return (float)(1.0 / (1.0 - attn_dropout_p_eff(p))); }

}  // namespace mmpt
