// qba_noise_profile.h -- noise profiles: a flip rate
// per list row and depolarised entries.  Shared by the profile Monte-Carlo
// kernels (qba_k_nprof_sampled, qba_mc_kern.h; qba_k_nprof_lists,
// qba_proto_nprof.hip) and qba_k_nprof_apply; montecarlo.noise_masks_profile
// is the host restatement.
//
// A profile is rate[0..n] (uint16, one per list row: row 0 the commander's
// list, row 1 Lc, row g >= 2 lieutenant g) and depol_q16.  With word(t) as in
// qba_noise.h, entry e of the instance keyed `key` folds the bits of all
// rates at once, from j0 = the lowest set bit of any rate upwards:
//   x = word(2s) | word(2s+1) << 32
//   r = ((r | x) & M_s) | ((r & x) & ~M_s)          s = 0 .. 15 - j0
// where nibble g of M_s is 0xF when bit (j0 + s) of rate[g] is set.  Nibble g
// of r thus goes through qba_noise.h's ladder for rate[g], preceded by ANDs
// into 0 for the steps below its own lowest bit: every bit of nibble g is 1
// with probability exactly rate[g] / 65536, and with all rates equal r is
// qba_noise_r's, bit for bit.  Then, when depol_q16 != 0, one more block
//   d = philox(ctr = {e_lo, e_hi, 8, QBA_NOISE_CTR_TAG}, key)
// (counter word 2 = 8: the ladder's are 0..7) depolarises the entry when
// (d.x & 0xFFFF) < depol_q16: r ^= d.z | d.w << 32, a uniform value into every
// group at once.  Group g is XORed with (r >> 4g) & (w - 1), as in qba_noise.h.
#pragma once
#include "qba_noise.h"

#define QBA_NPROF_DEPOL_CTR 8u

// The profile as the kernels take it, by value in the kernel arguments: every
// field is wave-uniform, so the masks are read into SGPRs.
struct QbaNoiseProfile {
  uint64_t m[16];   // M_s; entries from `steps` on are 0 and never read
  uint32_t steps;   // 16 - j0; 0: every rate is 0 and the ladder draws nothing
  uint32_t j0;      // the lowest set bit of any rate (0 when steps == 0)
  uint32_t depol;   // depol_q16; 0: no depolarisation block
};

// rates[0..n], each <= 65535 (the C entry points check), and depol_q16 <= 65535
inline QbaNoiseProfile qba_nprof_of(const uint16_t *rates, int n_rates, uint32_t depol_q16) {
  QbaNoiseProfile p{};
  p.depol = depol_q16;
  uint32_t any = 0;
  for (int g = 0; g < n_rates; ++g) any |= rates[g];
  if (!any) return p;
  while (!((any >> p.j0) & 1u)) ++p.j0;
  p.steps = 16u - p.j0;
  for (uint32_t s = 0; s < p.steps; ++s)
    for (int g = 0; g < n_rates; ++g)
      if ((rates[g] >> (p.j0 + s)) & 1u) p.m[s] |= (uint64_t)0xF << (4 * g);
  return p;
}

// one ladder step on a 32-bit half: (r | x) where m is set, (r & x) elsewhere.
// That is the bitwise majority of r, x and m, truth table 0xE8, which gfx950
// does in one v_bitop3_b32; written as an OR, an AND and a select the
// compiler emits three instructions per half (two bitop3 and a v_and_or_b32,
// no v_bfi_b32).
__device__ __forceinline__ uint32_t qba_nprof_sel(uint32_t r, uint32_t x, uint32_t m) {
  return __builtin_amdgcn_bitop3_b32(r, x, m, 0xE8);
}

// r of entry (elo, ehi) under the key (k0, k1); np is wave-uniform, so the
// loop, the masks and both branches are.  The masks are read from the kernel
// arguments at a uniform index: scalar loads, no register array.
__device__ __forceinline__ uint64_t qba_nprof_r(uint32_t elo, uint32_t ehi, uint32_t k0, uint32_t k1,
                                                const QbaNoiseProfile &np) {
  uint32_t lo = 0, hi = 0;
  for (uint32_t s = 0; s < np.steps; s += 2) {
    const QbaU4 y = qba_philox(elo, ehi, s >> 1, QBA_NOISE_CTR_TAG, k0, k1);
    const uint64_t m0 = np.m[s];
    lo = qba_nprof_sel(lo, y.x, (uint32_t)m0);
    hi = qba_nprof_sel(hi, y.y, (uint32_t)(m0 >> 32));
    if (s + 1 < np.steps) {
      const uint64_t m1 = np.m[s + 1];
      lo = qba_nprof_sel(lo, y.z, (uint32_t)m1);
      hi = qba_nprof_sel(hi, y.w, (uint32_t)(m1 >> 32));
    }
  }
  if (np.depol) {
    const QbaU4 d = qba_philox(elo, ehi, QBA_NPROF_DEPOL_CTR, QBA_NOISE_CTR_TAG, k0, k1);
    const bool hit = (d.x & 0xFFFFu) < np.depol;
    lo ^= hit ? d.z : 0u;
    hi ^= hit ? d.w : 0u;
  }
  return (uint64_t)lo | (uint64_t)hi << 32;
}

// qba_noise_d for a run-time n: XOR the masks into an entry in the byte layout
// (group g = byte g % 4 of D[g / 4]); bytes past group n stay as they are
__device__ __forceinline__ void qba_nprof_d(uint64_t r, uint32_t (&D)[4], int G, int w) {
  const uint32_t full = 0x01010101u * (uint32_t)(w - 1);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int nb = G - 4 * i;  // groups in word i
    const uint32_t keep = nb >= 4 ? full : nb > 0 ? full & ((1u << (8 * nb)) - 1u) : 0u;
    D[i] ^= qba_noise_spread((uint32_t)(r >> (16 * i)) & 0xFFFFu) & keep;
  }
}

// What is wrong with a profile's arguments (NULL: nothing), for qba_mc_check's
// envelope: checked right after `adv` and before ctx
inline const char *qba_nprof_bad(int n, const uint16_t *rates, int n_rates, uint32_t depol_q16) {
  if (n_rates != n + 1) return "n_rates must be n_parties + 1";
  if (!rates) return "rates_host is NULL";
  return depol_q16 > 65535u ? "depol_q16 must be <= 65535" : nullptr;
}

// the lists curve kernel under a profile (qba_proto_nprof.hip)
void qba_launch_nprof_lists(dim3 grid, size_t lds, hipStream_t stream, int n, int n_dis, uint64_t seed_base,
                            int64_t first, int64_t n_inst, const uint8_t *lists, uint64_t ld, uint64_t inst_stride,
                            int32_t *out, const QbaMcCounts &cv, uint32_t adv, const QbaNoiseProfile &np);
// qba_noise_profile_apply behind its checks (qba_proto_nprof.hip)
int qba_launch_nprof_apply(int n, uint64_t seed_base, int64_t n_inst, uint64_t count, const QbaNoiseProfile &np,
                           uint8_t *lists, uint64_t ld, uint64_t inst_stride, hipStream_t stream);
