// qba_lists_step.h -- the thread-steps of both row layouts and the kernels of
// qba_lists_kern.h: list (plain, deferred, pair-bin), batched and the slab
// reductions.  Samples with qba_lists_sample.h (qba_sample_quad, qba_stage)
// and counts with qba_lists_count.h (the queue, qba_count_quad, qba_pb_flush).
#pragma once
#include "qba_lists_count.h"
#include "qba_noise.h"

// 4x4 byte transpose: r_i byte j = input j byte i (an involution).
__device__ __forceinline__ void qba_t4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t &r0,
                                       uint32_t &r1, uint32_t &r2, uint32_t &r3) {
  const uint32_t t0 = qba_perm_b(b, a, 0x06020400u), t1 = qba_perm_b(b, a, 0x07030501u);
  const uint32_t t2 = qba_perm_b(d, c, 0x06020400u), t3 = qba_perm_b(d, c, 0x07030501u);
  r0 = qba_perm_b(t2, t0, 0x05040100u);
  r1 = qba_perm_b(t3, t1, 0x05040100u);
  r2 = qba_perm_b(t2, t0, 0x07060302u);
  r3 = qba_perm_b(t3, t1, 0x07060302u);
}

// The qubit-flip noise of a sampled quad (qba_noise.h; the noisy batched
// kernels): entry c0 + j of the instance keyed (k0, k1) takes its mask before
// anything looks at it.  The entries past `valid` of a partial quad stay 0.
template <int NP>
__device__ __forceinline__ void qba_noise_quad(uint32_t c0, int valid, uint32_t k0, uint32_t k1, const QbaNoise &nz,
                                               uint32_t (&D)[4][CF<NP>::ND]) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j >= valid) continue;
    uint32_t T[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < ND; ++i) T[i] = D[j][i];
    qba_noise_d<C::G, C::W>(qba_noise_r(c0 + (uint32_t)j, 0u, k0, k1, nz), T);
#pragma unroll
    for (int i = 0; i < ND; ++i) D[j][i] = T[i];
  }
}

// One thread-step over QPT consecutive quads: entries [c0, c0 + 4 QPT) of the
// launch (columns of `lists`).  Each list row is stored / loaded as one
// 4*QPT-byte vector per thread (16 B at QPT = 4: a wave moves 1 KiB per row).
// MODE 0: sample -> lists;  MODE 1: sample -> lists + counts;  MODE 2: lists -> counts
// TAIL (QPT = 1 only): the last, partial quad, byte by byte.
template <int NP, int MODE, int SAMP, int QPT, bool TAIL, bool WQ = false, int CNT = 0, int PW = QBA_PAIRWISE,
          bool NZ = false>
__device__ __forceinline__ void qba_step(uint32_t c0, uint32_t count, uint64_t first, uint32_t k0,
                                         uint32_t k1, const QbaProgramSet *__restrict__ ps,
                                         const uint64_t *pat, const uint64_t *apat,
                                         const uint64_t *thr, const uint32_t *pl,
                                         uint8_t *__restrict__ lists, uint64_t ld, uint32_t *hist,
                                         QbaWaveQ *wq = nullptr, bool act = true, QbaNoise nz = QbaNoise{}) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  static_assert(QPT == 1 || QPT == 2 || QPT == 4, "QPT");
  static_assert(!NZ || (MODE == 1 && CNT == 0), "noise: the batched kernels' sample + check only");
  static_assert(!TAIL || QPT == 1, "tail quads are single");
  static_assert(CNT == 0 || MODE == 1, "pair bins count the fused kernel's own lists only");
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  using V = typename std::conditional<QPT == 4, u32x4, typename std::conditional<QPT == 2, u32x2, uint32_t>::type>::type;
  const int valid = !TAIL ? 4 : ((count - c0) >= 4 ? 4 : (int)(count - c0));
  uint32_t row[QPT][4 * ND];
  uint32_t D[4][ND];
  const uint32_t am = act ? 0xffu : 0u;
  if constexpr (MODE == 2) {
#pragma unroll
    for (int k = 0; k < QPT; ++k)
#pragma unroll
      for (int g = 0; g < 4 * ND; ++g) row[k][g] = 0;
    if (!TAIL && act) {
#pragma unroll
      for (int g = 0; g < C::G; ++g) {
        const V v = __builtin_nontemporal_load(reinterpret_cast<const V *>(lists + (uint64_t)g * ld + c0));
        const uint32_t *pv = reinterpret_cast<const uint32_t *>(&v);
#pragma unroll
        for (int k = 0; k < QPT; ++k) row[k][g] = pv[k];
      }
    } else if (TAIL) {
      for (int g = 0; g < C::G; ++g)
        for (int j = 0; j < valid; ++j) row[0][g] |= (uint32_t)lists[(uint64_t)g * ld + c0 + j] << (8 * j);
    }
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
#pragma unroll
      for (int i = 0; i < ND; ++i)
        qba_t4(row[k][4 * i], row[k][4 * i + 1], row[k][4 * i + 2], row[k][4 * i + 3], D[0][i],
               D[1][i], D[2][i], D[3][i]);
      if constexpr (WQ) {  // the caller's queue (never null)
#pragma unroll
        for (int j = 0; j < 4; ++j) qba_q_push<NP, MODE == 1>(*wq, D[j], qba_isq_d<NP>(D[j], am), hist);
      } else {
        qba_count_quad<NP>(D, valid, hist, row[k]);
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
      qba_sample_quad<NP, SAMP, TAIL, PW>(c0 + 4 * k, valid, first, k0, k1, ps, pat, apat, thr, pl, D);
      if constexpr (NZ) qba_noise_quad<NP>(c0 + 4 * k, valid, k0, k1, nz, D);
#pragma unroll
      for (int i = 0; i < ND; ++i)
        qba_t4(D[0][i], D[1][i], D[2][i], D[3][i], row[k][4 * i], row[k][4 * i + 1],
               row[k][4 * i + 2], row[k][4 * i + 3]);
      if constexpr (MODE == 1) {
        if constexpr (WQ) {  // the caller's queue (never null)
          // L0 != L1 (tfg.py:327) of the quad's 4 entries at once: byte j of
          // row 0 XOR row 1 is nonzero iff entry j is Q-correlated
          const uint32_t xq = (row[k][0] ^ row[k][1]) & (act ? 0xffffffffu : 0u);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            qba_push<NP, MODE == 1, CNT>(*wq, D[j], (xq & (0xffu << (8 * j))) != 0u, hist);
        } else if constexpr (CNT == 1) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < valid) qba_count_one<NP, 1>(D[j], hist);
        } else {
          qba_count_quad<NP>(D, valid, hist, row[k]);
        }
      }
    }
    if (!TAIL && act)
    {
#pragma unroll
      for (int g = 0; g < C::G; ++g) {
        V v;
        uint32_t *pv = reinterpret_cast<uint32_t *>(&v);
#pragma unroll
        for (int k = 0; k < QPT; ++k) pv[k] = row[k][g];
        // row base opaque in SGPRs (an empty asm: no instruction is emitted),
        // so the store is `global_store v_c0, v_data, s[row]` with a 32-bit
        // lane offset -- otherwise the compiler shares lists + c0 as a 64-bit
        // VGPR and pays a 64-bit VALU add per row
        uint64_t rb = reinterpret_cast<uint64_t>(lists) + (uint64_t)g * ld;
        asm("" : "+s"(rb));
        typedef __attribute__((address_space(1))) V GV;  // global, not flat
        GV *dst = reinterpret_cast<GV *>(rb + c0);
        // the rows are streamed out once: nontemporal stores move the 12 rows of
        // 1.25e8 entries in 0.313 ms instead of 0.356 (tools/ubench/stores2)
        __builtin_nontemporal_store(v, dst);
      }
    } else if (TAIL) {
      for (int g = 0; g < C::G; ++g)
        for (int j = 0; j < valid; ++j) lists[(uint64_t)g * ld + c0 + j] = (uint8_t)(row[0][g] >> (8 * j));
    }
  }
}

// The same thread-step over NIBBLE rows (qba.h, "packed lists"): byte b of
// row g holds columns 2b (low nibble) and 2b+1 (high nibble), half the bytes
// of the byte layout.  Every value is < w <= 16, so two entries' byte-layout
// words fold into one word -- D[2p] | D[2p+1] << 4, byte g' = the packed pair
// of group 4i+g' -- BEFORE the transpose: one 4x4 transpose per 8 entries
// (QPT = 2, one 4-B store per row) instead of two, and half the HBM writes,
// which keeps the chip's clock up in the driver's cold window
// (profiles/r3/ab32_microopts_and_stores.txt: 12-row packed stores 375-381 us vs 421-424 us).
// QPT = 1 (unaligned starts, the tail quads): 2 bytes per row, stored as bytes
// (a chunk may start at an odd byte).  MODE 2 reads the same layout; an
// unpacked quad's entries come out permuted (counting is order-free).
template <int NP, int MODE, int SAMP, int QPT, bool TAIL, bool WQ = false, int CNT = 0, int PW = QBA_PAIRWISE,
          bool NZ = false>
__device__ __forceinline__ void qba_step_pk(uint32_t c0, uint32_t count, uint64_t first, uint32_t k0,
                                            uint32_t k1, const QbaProgramSet *__restrict__ ps,
                                            const uint64_t *pat, const uint64_t *apat,
                                            const uint64_t *thr, const uint32_t *pl,
                                            uint8_t *__restrict__ lists, uint64_t ld, uint32_t *hist,
                                            QbaWaveQ *wq, bool act, QbaNoise nz = QbaNoise{}) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  static_assert(QPT == 1 || QPT == 2, "packed rows: QPT 1 or 2");
  static_assert(!NZ || (MODE == 1 && CNT == 0), "noise: the batched kernels' sample + check only");
  static_assert(!TAIL || QPT == 1, "tail quads are single");
  static_assert(CNT == 0 || MODE != 0, "pair bins count");
  static_assert(C::W <= 16, "a value must fit a nibble");
  typedef __attribute__((address_space(1))) uint32_t GU;
  const int valid = !TAIL ? 4 : ((count - c0) >= 4 ? 4 : (int)(count - c0));
  const uint64_t cb = c0 >> 1;  // byte column of the step's first entry
  uint32_t D[4][ND];
  if constexpr (MODE == 2) {
    uint32_t row[QPT][4 * ND];
#pragma unroll
    for (int k = 0; k < QPT; ++k)
#pragma unroll
      for (int g = 0; g < 4 * ND; ++g) row[k][g] = 0;
    if (!TAIL && act) {
#pragma unroll
      for (int g = 0; g < C::G; ++g) {
        if constexpr (QPT == 2) {
          uint64_t rb = reinterpret_cast<uint64_t>(lists) + (uint64_t)g * ld;
          asm("" : "+s"(rb));
          const uint32_t v = __builtin_nontemporal_load(reinterpret_cast<const GU *>(rb + cb));
          row[0][g] = v & 0x0f0f0f0fu;         // columns 0, 2, 4, 6
          row[1][g] = (v >> 4) & 0x0f0f0f0fu;  // columns 1, 3, 5, 7
        } else {
          const uint8_t *r = lists + (uint64_t)g * ld + cb;
          const uint32_t h = (uint32_t)r[0] | ((uint32_t)r[1] << 8);
          row[0][g] = (h & 0x0f0fu) | ((h & 0xf0f0u) << 12);  // columns 0, 2, 1, 3
        }
      }
    } else if (TAIL) {
      for (int g = 0; g < C::G; ++g)
        for (int j = 0; j < valid; ++j)
          row[0][g] |= (uint32_t)((lists[(uint64_t)g * ld + cb + (j >> 1)] >> (4 * (j & 1))) & 15) << (8 * j);
    }
    const uint32_t am = act ? 0xffu : 0u;
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
#pragma unroll
      for (int i = 0; i < ND; ++i)
        qba_t4(row[k][4 * i], row[k][4 * i + 1], row[k][4 * i + 2], row[k][4 * i + 3], D[0][i],
               D[1][i], D[2][i], D[3][i]);
      if constexpr (WQ) {  // the caller's queue (never null)
#pragma unroll
        for (int j = 0; j < 4; ++j) qba_push<NP, false, CNT>(*wq, D[j], qba_isq_d<NP>(D[j], am), hist);
      } else if constexpr (CNT == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < (TAIL ? valid : 4)) qba_count_one<NP, 1>(D[j], hist);
      } else {
        qba_count_quad<NP>(D, TAIL ? valid : 4, hist, row[k]);
      }
    }
  } else {
    uint32_t Dp[2 * QPT][ND];  // pair p: entries 2p, 2p+1 of the step
    const uint32_t am = act ? 0xffu : 0u;
    const uint64_t actm = __ballot(act);  // the step's active lanes
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
      qba_sample_quad<NP, SAMP, TAIL, PW>(c0 + 4 * k, valid, first, k0, k1, ps, pat, apat, thr, pl, D);
      if constexpr (NZ) qba_noise_quad<NP>(c0 + 4 * k, valid, k0, k1, nz, D);
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        Dp[2 * k][i] = D[0][i] | (D[1][i] << 4);
        Dp[2 * k + 1][i] = D[2][i] | (D[3][i] << 4);
      }
      if constexpr (MODE == 1) {
        if constexpr (WQ) {  // the caller's queue (never null)
          if constexpr (CNT == 1) {
            // L0 != L1 (tfg.py:327) of each entry: one SDWA compare of byte 0
            // with byte 1 of its word 0, the step's active lanes ANDed in on
            // the scalar unit
#pragma unroll
            for (int j = 0; j < 4; ++j) qba_q_push_pb_m<NP>(*wq, D[j], qba_isq_mask(D[j][0], actm));
          } else {
            // ... of a pair at once: nibble 0 / 1 of (byte 0 ^ byte 1) of its
            // packed word 0 is entry 2p / 2p+1's test
#pragma unroll
            for (int p = 0; p < 2; ++p) {
              const uint32_t w0 = Dp[2 * k + p][0];
              const uint32_t x = (w0 ^ (w0 >> 8)) & am;
              qba_push<NP, true, CNT>(*wq, D[2 * p], (x & 0x0fu) != 0u, hist);
              qba_push<NP, true, CNT>(*wq, D[2 * p + 1], x > 0x0fu, hist);
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < valid) qba_count_one<NP, CNT>(D[j], hist);
        }
      }
    }
    if (!TAIL && act) {
      uint64_t rbl = 0;  // the running row base
      (void)rbl;
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        uint32_t r[4];
        if constexpr (QPT == 2)
          qba_t4(Dp[0][i], Dp[1][i], Dp[2][i], Dp[3][i], r[0], r[1], r[2], r[3]);
        else
          qba_t4(Dp[0][i], Dp[1][i], 0u, 0u, r[0], r[1], r[2], r[3]);
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
          const int g = 4 * i + gg;
          if (g >= C::G) continue;
          // row base opaque in SGPRs, 32-bit lane offset (as qba_step)
          // one running row pointer (s_add_u32 / s_addc_u32 per row) instead
          // of n+1 loop-invariant 64-bit bases
          if (g == 0) {
            rbl = reinterpret_cast<uint64_t>(lists);
            asm volatile("" : "+s"(rbl));
          } else {
            rbl += ld;
            asm volatile("" : "+s"(rbl));
          }
          const uint64_t rb = rbl;
          if constexpr (QPT == 2) {
            __builtin_nontemporal_store(r[gg], reinterpret_cast<GU *>(rb + cb));
          } else if (!((reinterpret_cast<uintptr_t>(lists) | ld) & 1)) {  // uniform: rows 2-byte aligned (cb is even)
            typedef __attribute__((address_space(1))) uint16_t GH;
            *reinterpret_cast<GH *>(rb + cb) = (uint16_t)r[gg];
          } else {
            uint8_t *d = reinterpret_cast<uint8_t *>(rb + cb);
            d[0] = (uint8_t)r[gg];
            d[1] = (uint8_t)(r[gg] >> 8);
          }
        }
      }
    } else if (TAIL) {
      // the call's last, partial quad: its bytes (a missing entry's nibble is 0)
      for (int i = 0; i < ND; ++i)
        for (int gg = 0; gg < 4; ++gg) {
          const int g = 4 * i + gg;
          if (g >= C::G) continue;
          for (int b = 0; 2 * b < valid; ++b)
            lists[(uint64_t)g * ld + cb + b] = (uint8_t)(Dp[b][i] >> (8 * gg));
        }
    }
  }
}

template <int NP, int MODE, int SAMP, int QPT, bool TAIL, int PK, bool WQ = false, int CNT = 0, int PW = QBA_PAIRWISE,
          bool NZ = false>
__device__ __forceinline__ void qba_step_l(uint32_t c0, uint32_t count, uint64_t first, uint32_t k0,
                                           uint32_t k1, const QbaProgramSet *__restrict__ ps,
                                           const uint64_t *pat, const uint64_t *apat,
                                           const uint64_t *thr, const uint32_t *pl,
                                           uint8_t *__restrict__ lists, uint64_t ld, uint32_t *hist,
                                           QbaWaveQ *wq = nullptr, bool act = true, QbaNoise nz = QbaNoise{}) {
  if constexpr (PK)
    qba_step_pk<NP, MODE, SAMP, QPT, TAIL, WQ, CNT, PW, NZ>(c0, count, first, k0, k1, ps, pat, apat, thr, pl, lists, ld, hist, wq, act, nz);
  else
    qba_step<NP, MODE, SAMP, QPT, TAIL, WQ, CNT, PW, NZ>(c0, count, first, k0, k1, ps, pat, apat, thr, pl, lists, ld, hist, wq, act, nz);
}

// One of the quads that remain after a launch's whole thread-steps (< 4 QPT
// entries, a quad per thread): a whole quad, or the call's last, partial one.
template <int NP, int MODE, int SAMP, int PK, int CNT = 0, int PW = QBA_PAIRWISE, bool NZ = false>
__device__ __forceinline__ void qba_leftover(uint32_t c0, uint32_t count, uint64_t first, uint32_t k0, uint32_t k1,
                                             const QbaProgramSet *__restrict__ ps, const uint64_t *pat,
                                             const uint64_t *apat, const uint64_t *thr, const uint32_t *pl,
                                             uint8_t *__restrict__ lists, uint64_t ld, uint32_t *hist,
                                             QbaNoise nz = QbaNoise{}) {
  if (c0 + 4 <= count)
    qba_step_l<NP, MODE, SAMP, 1, false, PK, false, CNT, PW, NZ>(c0, count, first, k0, k1, ps, pat, apat, thr, pl, lists, ld, hist,
                                                                 nullptr, true, nz);
  else
    qba_step_l<NP, MODE, SAMP, 1, true, PK, false, CNT, PW, NZ>(c0, count, first, k0, k1, ps, pat, apat, thr, pl, lists, ld, hist,
                                                                nullptr, true, nz);
}

// The outputs of a counting launch start at zero unless the call accumulates:
// the list kernel's workgroup 0 clears them before the reduction adds in.
struct QbaZero {
  int64_t *H, *C, *P, *stats;
  uint32_t flags;  // bit 0: clear H, C, P; bit 1: clear the stats
};
template <int NP>
__device__ __forceinline__ void qba_zero_outputs(const QbaZero &z, int tid, int bs) {
  using C = QCfg<NP>;
  if (z.flags & 1) {
    for (int i = tid; i < C::HB; i += bs) z.H[i] = 0;
    for (int i = tid; i < C::CB; i += bs) z.C[i] = 0;
    for (int i = tid; i < C::W; i += bs) z.P[i] = 0;
  }
  if ((z.flags & 2) && z.stats && tid < C::STATS) z.stats[tid] = 0;
}

// Waves per SIMD the list kernels are compiled for.  The closed-form sampler
// runs 2 workgroups of 1024 threads per CU = 8 waves per SIMD (the CDNA4
// maximum): with its quads sampled pair by pair (QBA_PAIRWISE) and the round
// keys / row bases re-derived on the scalar unit (QBA_SGPR_LEAN) it fits the
// 64 VGPRs and the SGPR budget that needs, and the extra waves hide the LDS
// latency of the histogram atomics: -3 % cycles per launch against 6 waves
// of 768 threads (profiles/r3/r3k).  The table samplers (n > 11) need more
// registers and keep the compiler's choice.
#define QBA_LISTS_BOUNDS \
  __attribute__((amdgpu_flat_work_group_size(1, QBA_LBLOCK), amdgpu_waves_per_eu(SAMP == QBA_S_CLOSED ? 8 : 1)))
#define QBA_LISTS_BOUNDS_PB \
  __attribute__((amdgpu_flat_work_group_size(1, QBA_LBLOCK), amdgpu_waves_per_eu(8)))
// PK = 1: nibble rows (qba_step_pk), ld in bytes of packed row.
// The body of the list kernel; its workgroups are those after the first
// `red` (qba_k_lists: 0; qba_k_lists_def: its reduce workgroups).
template <int NP, int MODE, int SAMP, int QPT, int PK, int BS = QBA_LBLOCK, int CNT = 0, int PW = QBA_PAIRWISE>
__device__ __forceinline__ void qba_lists_body(const QbaProgramSet *__restrict__ ps, uint32_t k0, uint32_t k1,
                                               uint64_t first, uint32_t count, uint8_t *__restrict__ lists,
                                               uint64_t ld, uint32_t *__restrict__ slab, QbaZero zero,
                                               uint32_t red, uint32_t tail = 0) {
  using C = QCfg<NP>;
  extern __shared__ __align__(16) uint64_t lds[];
  // list workgroups: [red, gridDim.x - tail) (reduce workgroups of a
  // deferred reduction after them, qba_k_lists_def and
  // qba_k_lists_pbdef)
  const uint32_t bid = blockIdx.x - red, nblk = gridDim.x - red - tail;
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *hist = qba_stage<NP, MODE, SAMP, BS>(ps, lds, pat, apat, thr, pl);
  // the launcher sizes what follows the tables: qba_count_lds, CNT: qba_pb_lds
  static_assert(!CNT || C::NBP <= QbaPB::AREA, "a wrapped workgroup recounts into classic bins in the pair bins' place");
  if constexpr (CNT) {  // pair bins: array A 1-KiB aligned (qba_count_pb ORs 64 u into its address)
    const uint32_t h = (uint32_t)(uintptr_t)(qba_lds_u32 *)hist;
    hist += (((h + 1023u) & ~1023u) - h) / 4;
  }
  if (MODE != 0) {
    constexpr int NZ = CNT ? QbaPB::AREA : C::NBP;
    for (int i = threadIdx.x; i < NZ; i += BS) hist[i] = 0u;
  }
  __syncthreads();
  const uint32_t nunits = count / (4 * QPT);
  // the grid stride in an SGPR, read once: reloading gridDim in the loop is a
  // scalar load whose s_waitcnt lgkmcnt(0) also drains every LDS atomic the
  // wave has in flight (-2% step time)
  const uint32_t ustride = __builtin_amdgcn_readfirstlane(nblk * BS);
  // unit u of a step: wave-major over the grid (wave w of workgroup b takes
  // units [(w nblk + b) 64, +64)), so a launch with fewer units than threads
  // spreads them over every workgroup instead of filling the first ones;
  // a wave's 64 units stay consecutive (one 256-B / 512-B store per row)
  const uint32_t u0 = ((threadIdx.x >> 6) * nblk + bid) * 64u + (threadIdx.x & 63u);
  // the wave's index in an SGPR: the code after the main loop rebuilds the
  // thread index from it and the lane id instead of keeping threadIdx.x (and
  // what derives from it) live across the loop -- at 64 VGPRs those values
  // were spilled to scratch, and a kernel with scratch waits ~6 us longer for
  // its dispatch after the previous kernel (profiles/r5/slab_event)
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if constexpr (MODE != 0) {
    QbaWaveQ wq;
    if constexpr (CNT) {  // 8-B slots after the pair bins, each ring aligned to its size
      const uint32_t h = (uint32_t)(uintptr_t)(qba_lds_u32 *)hist + QbaPB::AREA * 4;
      wq.base = __builtin_amdgcn_readfirstlane(((h + QBA_QCAP * 8 - 1) & ~(uint32_t)(QBA_QCAP * 8 - 1)) +
                                               (threadIdx.x >> 6) * (QBA_QCAP * 8));
    } else {
      wq.base = qba_queue_base<NP>(hist) + (threadIdx.x >> 6) * (CF<NP>::ND * QBA_QCAP * 4);
    }
    wq.tail = 0;
    wq.qn = 0;
    wq.hoff = (uint32_t)(uintptr_t)(qba_lds_u32 *)hist;
    asm("" : "+v"(wq.hoff));  // held in a VGPR (no instruction is emitted)
    // wave-uniform trip count: pushes and drains always run with the whole wave
    for (uint32_t u = u0;; u += ustride) {
      const bool act = u < nunits;
      if (!__any(act)) break;
      qba_step_l<NP, MODE, SAMP, QPT, false, PK, true, CNT, PW>(u * (4 * QPT), count, first, k0, k1, ps, pat, apat, thr,
                                                            pl, lists, ld, hist, &wq, act);
    }
    while (wq.qn) {  // wave-uniform
      if constexpr (CNT)
        qba_q_drain_pb<NP>(wq, wq.qn < 64 ? wq.qn : 64u);
      else
        qba_q_drain<NP, MODE == 1>(wq, hist, wq.qn < 64 ? wq.qn : 64u);
    }
  } else {
    for (uint32_t u = u0; u < nunits; u += ustride)
      qba_step_l<NP, MODE, SAMP, QPT, false, PK, false, 0, PW>(u * (4 * QPT), count, first, k0, k1, ps, pat, apat,
                                                            thr, pl, lists, ld, hist);
  }
  const uint32_t tid = (wv << 6) | __lane_id();  // == threadIdx.x (above)
  // the remaining < 4 QPT entries: whole quads, then the partial one
  const uint32_t r0 = nunits * (4 * QPT), rq = (count - r0 + 3) >> 2;
  if (bid == nblk - 1 && tid < rq)
    qba_leftover<NP, MODE, SAMP, PK, CNT, PW>(r0 + 4 * tid, count, first, k0, k1, ps, pat, apat, thr, pl, lists, ld, hist);
  if (MODE != 0) {
    __syncthreads();
    uint32_t *row = slab + (size_t)bid * C::NBP;
    bool classic = !CNT;
    if constexpr (CNT) {
      if (qba_pb_flush<NP, BS>(hist, row, (int)tid)) {
        // a pair-bin lane wrapped (never for sampled lists at QBA_PB_BUDGET
        // entries per workgroup): recount this workgroup's entries -- the
        // same units and tail as above -- from the rows it stored, into the
        // classic 32-bit bins (qba_count_quad: exact, order-free)
        __syncthreads();
        for (int i = tid; i < C::NBP; i += BS) hist[i] = 0u;
        __threadfence();  // this workgroup's list stores are complete and visible to its loads
        __syncthreads();
        for (uint32_t u = ((wv * nblk + bid) << 6) | __lane_id(); u < nunits; u += ustride)
          qba_step_l<NP, 2, QBA_S_GENERAL, QPT, false, PK>(u * (4 * QPT), count, first, k0, k1, ps, pat, apat, thr,
                                                         pl, lists, ld, hist);
        if (bid == nblk - 1 && tid < rq)
          qba_leftover<NP, 2, QBA_S_GENERAL, PK>(r0 + 4 * tid, count, first, k0, k1, ps, pat, apat, thr, pl, lists, ld, hist);
        __syncthreads();
        if (tid == 0) hist[C::HBL + C::CBL + 1] += 1u;  // stats[1]: recounting workgroups
        classic = true;
      }
    }
    if (classic) {
      uint4 *dst = reinterpret_cast<uint4 *>(row);
      const uint4 *src = reinterpret_cast<const uint4 *>(hist);
      for (int i = tid; i < C::NBP / 4; i += BS) dst[i] = src[i];
    }
    // any point of this kernel precedes the reduction; at the end it leaves
    // the main loop's code placement alone
    if (bid == nblk - 1) qba_zero_outputs<NP>(zero, tid, BS);
  }
}

// CNT 1: pair-bin counting (QbaUsePB kernels only; the launcher picks it for
// launches of at least ctx->pb_min entries).
template <int NP, int MODE, int SAMP, int QPT, int PK, int CNT = 0>
__global__ void QBA_LISTS_BOUNDS
    qba_k_lists(const QbaProgramSet *__restrict__ ps, uint32_t k0, uint32_t k1, uint64_t first,
                uint32_t count, uint8_t *__restrict__ lists, uint64_t ld,
                uint32_t *__restrict__ slab, QbaZero zero) {
  static_assert(!CNT || QbaUsePB<NP, MODE, SAMP, PK>::value, "pair bins: the n = 11 kernels of QbaUsePB only");
  qba_lists_body<NP, MODE, SAMP, QPT, PK, QBA_LBLOCK, CNT>(ps, k0, k1, first, count, lists, ld, slab, zero, 0u);
}

// ---------------------------------------------------------------------------
// Deferred slab reduction (qba_sample_check_deferred / _packed_deferred, qba.h).
// A launch that has few list workgroups (configs[1]: 163 of 512 slots) leaves
// CUs idle, and its separate reduce launch costs a kernel boundary per call.
// A deferred call instead runs the PREVIOUS deferred call's reduction in W
// extra workgroups of its own list kernel (qba_k_lists_def), on two
// alternating slab buffers; qba_flush_deferred reduces the last one
// (qba_k_reduce_def).  Reduce workgroup u owns everything of bin row u:
// H[u][*][*], the pair bins C[u][*] (and, for u = 0, the stats), so it writes
// every output word of u exactly once (plain stores, no atomics, no zeroing
// pass): out = (acc ? out : 0) + the column sum over the slab rows, with the
// derived words (|P_u| = sum_x H[u][0][x] -> P[u], C[u][g][g], H[u][1][u])
// from the same sums.  Bitwise identical to qba_k_reduce's result.
// ---------------------------------------------------------------------------
struct QbaDefer {
  const uint32_t *slab;  // the pending call's slab rows (NBP words apart)
  int rows;              // its list workgroups
  int red;               // reduce workgroups after the list workgroups: W, or 0 (none pending)
  int acc;               // the pending call accumulates into its outputs
  int sacc;              // ... and into the stats (a later chunk of one call)
  int64_t *H, *C, *P, *stats;
};

template <int NP>
__host__ __device__ constexpr int qba_def_cols(int u) {  // slab columns of bin row u
  using C = QCfg<NP>;
  return C::G * C::WP + C::CP + (u == 0 ? C::STATS : 0);
}
// Workgroups per bin row: part 0 owns columns [0, 2 WP) at least (groups 0
// and 1: |P_u| and every word derived from it), the other parts split the rest.
template <int NP>
__host__ __device__ constexpr int qba_def_parts() {
  using C = QCfg<NP>;
  return qba_def_cols<NP>(1) >= 8 * C::WP ? 4 : 1;
}
template <int NP>
__host__ __device__ constexpr int qba_def_wgs() {  // reduce workgroups of one deferred reduction
  return QCfg<NP>::W * qba_def_parts<NP>();
}

// LDS bytes of qba_reduce_u's scratch for a workgroup of bs threads
template <int NP>
__host__ __device__ constexpr size_t qba_reduce_lds(int bs) {
  return (size_t)(bs + qba_def_cols<NP>(0)) * sizeof(uint32_t);
}
// The reduce of part `part` of bin row u by one workgroup of bs threads; sh:
// LDS scratch of (bs + qba_def_cols(0)) words (qba_reduce_lds).
template <int NP>
__device__ __forceinline__ void qba_reduce_u(const QbaDefer &d, int u, int part, int tid, int bs, uint32_t *sh) {
  using C = QCfg<NP>;
  typedef unsigned long long u64;
  constexpr int NH = C::G * C::WP, NP4 = qba_def_parts<NP>();
  static_assert(qba_def_cols<NP>(0) <= QBA_DBLOCK && QBA_DBLOCK <= QBA_LBLOCK, "one column per thread at least");
  const int ncu = qba_def_cols<NP>(u);
  constexpr int SPAN = (qba_def_cols<NP>(1) + NP4 - 1) / NP4;
  constexpr int SPAN0 = NP4 == 1 ? qba_def_cols<NP>(0) : (SPAN > 2 * C::WP ? SPAN : 2 * C::WP);
  constexpr int REST = NP4 == 1 ? 1 : (qba_def_cols<NP>(1) - SPAN0 + NP4 - 2) / (NP4 - 1);
  const int c0 = part == 0 ? 0 : SPAN0 + (part - 1) * REST;
  const int c1 = part == 0 ? (SPAN0 < ncu ? SPAN0 : ncu) : (part == NP4 - 1 ? ncu : c0 + REST);
  const int nc = c1 - c0;
  const int S = bs / nc;  // row classes: thread (col, sub) sums rows sub, sub + S, ...
  const int col = c0 + tid % nc, sub = tid / nc;
  if (sub < S) {
    const int w = col < NH ? u * NH + col
                           : col < NH + C::CP ? C::HBL + u * C::CP + (col - NH) : C::HBL + C::CBL + (col - NH - C::CP);
    const uint32_t *src = d.slab + w;
    uint32_t s = 0;
    int r = sub;
    // 16 rows in flight per thread (the rows were written by the previous
    // kernel and come from beyond this XCD's L2)
    for (; r + 15 * S < d.rows; r += 16 * S) {
      uint32_t v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = src[(size_t)(r + k * S) * C::NBP];
#pragma unroll
      for (int k = 0; k < 16; ++k) s += v[k];
    }
    for (; r < d.rows; r += S) s += src[(size_t)r * C::NBP];
    sh[sub * nc + (col - c0)] = s;
  }
  __syncthreads();
  uint32_t *tot = sh + S * nc;  // tot[c - c0]
  if (tid < nc) {
    uint32_t t = 0;
    for (int k = 0; k < S; ++k) t += sh[k * nc + tid];
    tot[tid] = t;  // <= the entries of one launch (< 2^32)
  }
  __syncthreads();
  u64 psz = 0;  // |P_u|: group 0's bins (columns [0, W), part 0)
  if (part == 0) {
#pragma unroll
    for (int x = 0; x < C::W; ++x) psz += tot[x];
  }
  const bool acc = d.acc != 0;
  for (int c = c0 + tid; c < c1; c += bs) {
    if (c < NH) {
      const int g = c / C::WP, x = c - g * C::WP;
      if (x >= C::W) continue;  // row padding
      const u64 v = g == 1 ? (x == u ? psz : 0ull) : (u64)tot[c - c0];  // group 1: part 0 (c < 2 WP)
      int64_t *o = &d.H[(u * C::G + g) * C::W + x];
      *o = (acc ? *o : 0) + (int64_t)v;
    } else if (c < NH + C::CP) {
      int p = c - NH, g = 0;
      while (p >= C::G - 1 - g) p -= C::G - 1 - g++;  // pidx(g, h) inverted
      const int h = g + 1 + p;
      int64_t *o1 = &d.C[(u * C::G + g) * C::G + h], *o2 = &d.C[(u * C::G + h) * C::G + g];
      *o1 = (acc ? *o1 : 0) + (int64_t)tot[c - c0];
      *o2 = (acc ? *o2 : 0) + (int64_t)tot[c - c0];
    } else if (d.stats) {
      int64_t *o = &d.stats[c - NH - C::CP];
      *o = (d.sacc ? *o : 0) + (int64_t)tot[c - c0];
    }
  }
  if (part == 0) {
    for (int g = tid; g < C::G; g += bs) {
      int64_t *o = &d.C[(u * C::G + g) * C::G + g];
      *o = (acc ? *o : 0) + (int64_t)psz;
    }
    if (tid == 0) d.P[u] = (acc ? d.P[u] : 0) + (int64_t)psz;
  }
}
// The prologue of a list kernel that carries the pending reduction in its last
// d.red workgroups: true (workgroup-uniform) in those, which have then done it.
template <int NP>
__device__ __forceinline__ bool qba_reduce_tail(const QbaDefer &d, int bs) {
  extern __shared__ __align__(16) uint64_t lds[];
  const uint32_t nl = gridDim.x - (uint32_t)d.red;
  if (blockIdx.x >= nl) {  // workgroup-uniform
    constexpr int NP4 = qba_def_parts<NP>();
    const int r = (int)(blockIdx.x - nl);
    qba_reduce_u<NP>(d, r / NP4, r % NP4, (int)threadIdx.x, bs, reinterpret_cast<uint32_t *>(lds));
    return true;
  }
  return false;
}

// Sample + check (MODE 1) with the pending deferred call's reduction in the
// LAST d.red workgroups: the list workgroups (slab row = their index) are
// dispatched first, the reduce workgroups into the CUs they leave idle
// (configs[1]: 9.42-9.47 vs 9.68-10.27 us per pass with the reduction ahead,
// profiles/r5/c1)
template <int NP, int SAMP, int QPT, int PK>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, QBA_DBLOCK),
                               amdgpu_waves_per_eu(SAMP == QBA_S_CLOSED ? QBA_DEF_WAVES : 1)))
    qba_k_lists_def(const QbaProgramSet *__restrict__ ps, uint32_t k0, uint32_t k1, uint64_t first,
                    uint32_t count, uint8_t *__restrict__ lists, uint64_t ld, uint32_t *__restrict__ slab,
                    QbaZero zero, QbaDefer d) {
  if (qba_reduce_tail<NP>(d, QBA_DBLOCK)) return;
  qba_lists_body<NP, 1, SAMP, QPT, PK, QBA_DBLOCK, 0, QBA_DEF_PAIRWISE>(ps, k0, k1, first, count, lists,
                                                                                   ld, slab, zero, 0u, (uint32_t)d.red);
}

// qba_flush_deferred: the last pending reduction on its own.
template <int NP>
__global__ void __launch_bounds__(QBA_LBLOCK) qba_k_reduce_def(QbaDefer d) {
  extern __shared__ __align__(16) uint64_t lds[];
  constexpr int NP4 = qba_def_parts<NP>();
  qba_reduce_u<NP>(d, (int)blockIdx.x / NP4, (int)blockIdx.x % NP4, (int)threadIdx.x, QBA_LBLOCK,
                   reinterpret_cast<uint32_t *>(lds));
}

// The pair-bin kernel with a deferred reduction in its TAIL: the pending
// call's reduce workgroups come after the list workgroups, so they are
// dispatched as list workgroups finish -- into the slots of the ~20 % that
// run one thread-step fewer (1.25e8 entries over 512 x 1024 threads is 29.8
// steps) -- instead of a separate reduce launch after the list kernel.
template <int NP, int QPT, int PK>
__global__ void QBA_LISTS_BOUNDS_PB
    qba_k_lists_pbdef(const QbaProgramSet *__restrict__ ps, uint32_t k0, uint32_t k1, uint64_t first,
                      uint32_t count, uint8_t *__restrict__ lists, uint64_t ld, uint32_t *__restrict__ slab,
                      QbaZero zero, QbaDefer d) {
  if (qba_reduce_tail<NP>(d, QBA_LBLOCK)) return;
  qba_lists_body<NP, 1, QBA_S_CLOSED, QPT, PK, QBA_LBLOCK, 1>(ps, k0, k1, first, count, lists, ld, slab, zero, 0u,
                                                              (uint32_t)d.red);
}

// Batched independent instances (BASELINE configs[3]): instance i is its own
// run with Philox key seed_base + i over entries [0, count).  A workgroup
// owns whole instances, so its LDS histogram IS the instance's final count
// and is written out directly (no slab, no reduce launch).
// Compiled for 8 waves per SIMD on the closed sampler (configs[3]: 0.743 ->
// 0.728 ms/step, profiles/r5/batched; 53 VGPRs once the per-instance output
// addresses are no longer hoisted across the main loop)
template <int NP, int SAMP, int QPT, int PK>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, QBA_BLOCK),
                               amdgpu_waves_per_eu(SAMP == QBA_S_CLOSED ? 8 : 1)))
    qba_k_batched(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, int64_t n_inst,
                  uint64_t count, uint8_t *__restrict__ lists, uint64_t ld, uint64_t inst_stride,
                  int64_t *__restrict__ H, int64_t *__restrict__ Cc, int64_t *__restrict__ P) {
  using C = QCfg<NP>;
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *hist = qba_stage<NP, 1, SAMP, QBA_BLOCK>(ps, lds, pat, apat, thr, pl);
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t inst = blockIdx.x; inst < n_inst; inst += gridDim.x) {
    for (int i = (int)((wv << 6) | __lane_id()); i < C::NBINS; i += QBA_BLOCK) hist[i] = 0u;
    __syncthreads();
    const uint64_t key = seed_base + (uint64_t)inst;
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    uint8_t *L = lists + (uint64_t)inst * inst_stride;
    // QPT quads per thread-step, Q entries counted 64 at a time from the
    // per-wave LDS queue (as qba_k_lists), then the < 4 QPT remaining entries
    const uint32_t nunits = (uint32_t)count / (4 * QPT);
    QbaWaveQ wq;
    wq.base = qba_queue_base<NP>(hist) + wv * (CF<NP>::ND * QBA_QCAP * 4);
    wq.tail = 0;
    wq.qn = 0;
    wq.hoff = (uint32_t)(uintptr_t)(qba_lds_u32 *)hist;
    asm("" : "+v"(wq.hoff));
    for (uint32_t u = (wv << 6) | __lane_id();; u += QBA_BLOCK) {  // wave-uniform trip count
      const bool act = u < nunits;
      if (!__any(act)) break;
      qba_step_l<NP, 1, SAMP, QPT, false, PK, true>(u * (4 * QPT), (uint32_t)count, 0, k0, k1, ps, pat, apat, thr, pl,
                                              L, ld, hist, &wq, act);
    }
    while (wq.qn) qba_q_drain<NP, true>(wq, hist, wq.qn < 64 ? wq.qn : 64u);  // wave-uniform
    // the thread index rebuilt (as in qba_lists_body): nothing derived from
    // threadIdx.x stays live across the main loop to be spilled
    int tid = (int)((wv << 6) | __lane_id());
    asm volatile("" : "+v"(tid));  // opaque: the addresses built from it are not hoisted out of the instance loop
    const uint32_t r0 = nunits * (4 * QPT), rq = ((uint32_t)count - r0 + 3) >> 2;
    if ((uint32_t)tid < rq)
      qba_leftover<NP, 1, SAMP, PK>(r0 + 4 * (uint32_t)tid, (uint32_t)count, 0, k0, k1, ps, pat, apat, thr, pl, L, ld, hist);
    __syncthreads();
    int64_t *h = H + inst * C::HB, *c = Cc + inst * C::CB, *p = P + inst * C::W;
    for (int i = tid; i < C::HB; i += QBA_BLOCK) h[i] = qba_hval<NP>(hist, i);
    for (int r = tid; r < C::CB; r += QBA_BLOCK) {
      const int u = r / (C::G * C::G), g = (r / C::G) % C::G, k = r % C::G;
      const int64_t v = g < k ? hist[C::HBL + u * C::CP + C::pidx(g, k)]
                              : g > k ? hist[C::HBL + u * C::CP + C::pidx(k, g)]
                                      : qba_psize<NP>(hist, u);
      c[r] = v;
    }
    for (int u = tid; u < C::W; u += QBA_BLOCK) p[u] = qba_psize<NP>(hist, u);
    __syncthreads();
  }
}

// Waves per SIMD the noisy closed-form batched kernel is compiled for.  The
// flips are 64 more live bits per entry: up to n = 7 (two words per entry) the
// step still fits the 64 VGPRs of 8 waves, from n = 8 (three words) it spills
// at 8 and at 7 waves and is built for 6 (80 VGPRs, no scratch): DESIGN.md
// section 13.6.
#ifndef QBA_BATCHED_NOISY_WAVES_SMALL
#define QBA_BATCHED_NOISY_WAVES_SMALL 8  // an A/B build asks for 6
#endif
template <int NP>
constexpr int qba_batched_noisy_waves() {
  return CF<NP>::ND <= 2 ? QBA_BATCHED_NOISY_WAVES_SMALL : 6;
}

// qba_k_batched under qubit-flip noise (qba_sample_check_batched_noisy,
// DESIGN.md section 13.6): entry e of instance `inst` takes the mask
// qba_noise_r(e, 0, key of inst) right after it is sampled (the NZ flag of the
// thread-steps), so the rows stored and the tables counted are those of the
// noisy entries.  Noise takes no LDS: launch shape, LDS and grid are
// qba_k_batched's.  A text of its own, instantiated by
// qba_lists_noise_inst.hip into code objects of its own: one body shared with
// qba_k_batched changed the code of the closed-form noiseless kernels.
template <int NP, int SAMP, int QPT, int PK>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, QBA_BLOCK),
                               amdgpu_waves_per_eu(SAMP == QBA_S_CLOSED ? qba_batched_noisy_waves<NP>() : 1)))
    qba_k_batched_noisy(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, int64_t n_inst,
                        uint64_t count, uint8_t *__restrict__ lists, uint64_t ld, uint64_t inst_stride,
                        int64_t *__restrict__ H, int64_t *__restrict__ Cc, int64_t *__restrict__ P, QbaNoise nz) {
  using C = QCfg<NP>;
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *hist = qba_stage<NP, 1, SAMP, QBA_BLOCK>(ps, lds, pat, apat, thr, pl);
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t inst = blockIdx.x; inst < n_inst; inst += gridDim.x) {
    for (int i = (int)((wv << 6) | __lane_id()); i < C::NBINS; i += QBA_BLOCK) hist[i] = 0u;
    __syncthreads();
    const uint64_t key = seed_base + (uint64_t)inst;
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    uint8_t *L = lists + (uint64_t)inst * inst_stride;
    const uint32_t nunits = (uint32_t)count / (4 * QPT);
    QbaWaveQ wq;
    wq.base = qba_queue_base<NP>(hist) + wv * (CF<NP>::ND * QBA_QCAP * 4);
    wq.tail = 0;
    wq.qn = 0;
    wq.hoff = (uint32_t)(uintptr_t)(qba_lds_u32 *)hist;
    asm("" : "+v"(wq.hoff));
    for (uint32_t u = (wv << 6) | __lane_id();; u += QBA_BLOCK) {  // wave-uniform trip count
      const bool act = u < nunits;
      if (!__any(act)) break;
      qba_step_l<NP, 1, SAMP, QPT, false, PK, true, 0, QBA_PAIRWISE, true>(u * (4 * QPT), (uint32_t)count, 0, k0, k1, ps, pat,
                                                                           apat, thr, pl, L, ld, hist, &wq, act, nz);
    }
    while (wq.qn) qba_q_drain<NP, true>(wq, hist, wq.qn < 64 ? wq.qn : 64u);  // wave-uniform
    int tid = (int)((wv << 6) | __lane_id());
    asm volatile("" : "+v"(tid));  // opaque: the addresses built from it are not hoisted out of the instance loop
    const uint32_t r0 = nunits * (4 * QPT), rq = ((uint32_t)count - r0 + 3) >> 2;
    if ((uint32_t)tid < rq)
      qba_leftover<NP, 1, SAMP, PK, 0, QBA_PAIRWISE, true>(r0 + 4 * (uint32_t)tid, (uint32_t)count, 0, k0, k1, ps, pat, apat,
                                                           thr, pl, L, ld, hist, nz);
    __syncthreads();
    int64_t *h = H + inst * C::HB, *c = Cc + inst * C::CB, *p = P + inst * C::W;
    for (int i = tid; i < C::HB; i += QBA_BLOCK) h[i] = qba_hval<NP>(hist, i);
    for (int r = tid; r < C::CB; r += QBA_BLOCK) {
      const int u = r / (C::G * C::G), g = (r / C::G) % C::G, k = r % C::G;
      const int64_t v = g < k ? hist[C::HBL + u * C::CP + C::pidx(g, k)]
                              : g > k ? hist[C::HBL + u * C::CP + C::pidx(k, g)]
                                      : qba_psize<NP>(hist, u);
      c[r] = v;
    }
    for (int u = tid; u < C::W; u += QBA_BLOCK) p[u] = qba_psize<NP>(hist, u);
    __syncthreads();
  }
}

// Slab reduction straight into the int64 outputs (see qba.h for shapes).
// Workgroup (x, y) sums slab rows [y*RP, (y+1)*RP) for 1024 bins (4 per
// thread, 16-B loads) and adds each nonzero partial to the output word(s) the
// bin maps to with integer atomics (order-independent: bitwise
// reproducible): H as counted; a pair bin to C[u][g][h] and C[u][h][g]; group
// 0's bins also to |P_u| -- summed per workgroup in LDS first -- which is P[u],
// every C[u][g][g] and H[u][1][u] (group 1's bins are derived, see
// qba_psize); the stats bins to the stats.  The list kernel of the same
// launch zeroed the outputs unless the call accumulates, so no finalize pass
// or accumulator is needed.
template <int NP>
__global__ void __launch_bounds__(256)
    qba_k_reduce(const uint32_t *__restrict__ slab, int nrows, int64_t *__restrict__ H,
                 int64_t *__restrict__ Cc, int64_t *__restrict__ P, int64_t *__restrict__ stats) {
  using C = QCfg<NP>;
  typedef unsigned long long u64;
  __shared__ u64 psz[C::W];
  if (threadIdx.x < C::W) psz[threadIdx.x] = 0ull;
  __syncthreads();
  const int q = blockIdx.x * 256 + threadIdx.x;  // bin quad
  if (4 * q < C::NBP) {
    const int b0 = blockIdx.y * QBA_RED_ROWS;
    const int b1 = b0 + QBA_RED_ROWS < nrows ? b0 + QBA_RED_ROWS : nrows;
    u64 s[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll 8
    for (int b = b0; b < b1; ++b) {
      const uint4 v = reinterpret_cast<const uint4 *>(slab + (size_t)b * C::NBP)[q];
      s[0] += v.x;
      s[1] += v.y;
      s[2] += v.z;
      s[3] += v.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!s[j]) continue;
      const int b = 4 * q + j;
      if (b < C::HBL) {
        const int u = b / (C::G * C::WP), r = b - u * C::G * C::WP, g = r / C::WP, x = r - g * C::WP;
        if (x >= C::W || g == 1) continue;  // row padding / never counted
        atomicAdd(reinterpret_cast<u64 *>(&H[(u * C::G + g) * C::W + x]), s[j]);
        if (g == 0) atomicAdd(&psz[u], s[j]);
      } else if (b < C::HBL + C::CBL) {
        const int u = (b - C::HBL) / C::CP;
        int p = b - C::HBL - u * C::CP, g = 0;
        while (p >= C::G - 1 - g) p -= C::G - 1 - g++;  // pidx(g, h) inverted
        const int h = g + 1 + p;
        atomicAdd(reinterpret_cast<u64 *>(&Cc[(u * C::G + g) * C::G + h]), s[j]);
        atomicAdd(reinterpret_cast<u64 *>(&Cc[(u * C::G + h) * C::G + g]), s[j]);
      } else if (b < C::NBINS && stats) {
        atomicAdd(reinterpret_cast<u64 *>(&stats[b - C::HBL - C::CBL]), s[j]);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C::W * (C::G + 2); i += 256) {
    const int u = i / (C::G + 2), k = i - u * (C::G + 2);
    const u64 v = psz[u];
    if (!v) continue;
    int64_t *dst = k < C::G ? &Cc[(u * C::G + k) * C::G + k] : k == C::G ? &P[u] : &H[(u * C::G + 1) * C::W + u];
    atomicAdd(reinterpret_cast<u64 *>(dst), v);
  }
}
