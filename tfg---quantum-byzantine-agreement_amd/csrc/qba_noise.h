// qba_noise.h -- the qubit-flip noise model: every
// measured bit of an entry flips independently with probability k / 65536.
// Shared by the noisy fused Monte-Carlo kernels (qba_mc_kern.h) and
// qba_k_noise_apply (qba_noise.hip); montecarlo.noise_masks is the host
// restatement.
//
// Entry e of the instance keyed `key` draws word(t) = output word t % 4 of
//   philox(ctr = {e_lo, e_hi, t / 4, QBA_NOISE_CTR_TAG}, key = {key_lo, key_hi})
// and folds the bits of k from its lowest set bit j0 upwards into 64 bits r:
//   x = word(2s) | word(2s+1) << 32;  r = bit (j0 + s) of k ? r | x : r & x
// for s = 0 .. 15 - j0.  One step maps a bit's probability q to (bit + q) / 2,
// so every bit of r is 1 with probability exactly k / 65536.  Group g of the
// entry is XORed with (r >> 4g) & (w - 1).
#pragma once
#include "qba_internal.h"

// counter word 3: the sampler's is 0 or 1, the protocol's QBA_PROTO_CTR_TAG
#define QBA_NOISE_CTR_TAG 0x4E4F4953u

// The flip probability as the kernels take it (wave-uniform scalars).
struct QbaNoise {
  uint32_t bits;   // k >> ctz(k): bit s decides step s (bit 0 is set)
  uint32_t steps;  // 16 - ctz(k), one to sixteen; two steps per Philox block
};

inline QbaNoise qba_noise_of(uint32_t flip_q16) {
  int j0 = 0;
  while (!((flip_q16 >> j0) & 1u)) ++j0;  // callers pass 1 <= flip_q16 <= 65535
  return QbaNoise{flip_q16 >> j0, (uint32_t)(16 - j0)};
}

// r of entry (elo, ehi) under the key (k0, k1); nz is wave-uniform, so the
// loop and both selects are.
__device__ __forceinline__ uint64_t qba_noise_r(uint32_t elo, uint32_t ehi, uint32_t k0, uint32_t k1,
                                                const QbaNoise &nz) {
  uint64_t r = 0;
  for (uint32_t s = 0; s < nz.steps; s += 2) {
    const QbaU4 y = qba_philox(elo, ehi, s >> 1, QBA_NOISE_CTR_TAG, k0, k1);
    const uint64_t a = (uint64_t)y.x | (uint64_t)y.y << 32, b = (uint64_t)y.z | (uint64_t)y.w << 32;
    r = (nz.bits >> s) & 1u ? r | a : r & a;
    if (s + 1 < nz.steps) r = (nz.bits >> (s + 1)) & 1u ? r | b : r & b;
  }
  return r;
}

// the four nibbles of x (16 bits) to the low nibbles of four bytes
__device__ __forceinline__ uint32_t qba_noise_spread(uint32_t x) {
  x = (x | x << 8) & 0x00FF00FFu;
  return (x | x << 4) & 0x0F0F0F0Fu;
}

// bytes of byte-layout word i that hold a group g <= n, each as w - 1
__host__ __device__ constexpr uint32_t qba_noise_keep(int G, int w, int i) {
  uint32_t m = 0;
  for (int b = 0; b < 4; ++b)
    if (4 * i + b < G) m |= (uint32_t)(w - 1) << (8 * b);
  return m;
}

// XOR the masks into an entry in the byte layout of qba_entry_d (group g =
// byte g % 4 of D[g / 4]); words past the last group stay 0
template <int G, int W>
__device__ __forceinline__ void qba_noise_d(uint64_t r, uint32_t (&D)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (4 * i < G) D[i] ^= qba_noise_spread((uint32_t)(r >> (16 * i)) & 0xFFFFu) & qba_noise_keep(G, W, i);
}

// qba_noise_apply_batched behind its checks (qba_noise.hip)
int qba_launch_noise_apply(int n, uint64_t seed_base, int64_t n_inst, uint64_t count, uint32_t flip_q16,
                           uint8_t *lists, uint64_t ld, uint64_t inst_stride, hipStream_t stream);
