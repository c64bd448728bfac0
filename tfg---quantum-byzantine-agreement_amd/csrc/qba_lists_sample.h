// qba_lists_sample.h -- the samplers of the list kernels (qba_lists_kern.h):
// the measured shapes and QCfg, an entry's random words, the table samplers,
// the closed form, one entry / one quad into the byte layout (qba_entry_d,
// qba_sample_quad) and the staging of a program's tables in LDS (qba_stage).
// Needs nothing from qba_lists_count.h or qba_lists_step.h.
#pragma once
#include <type_traits>

#include "qba_lists.h"

// Measured shapes of the list kernels (the rejected
// alternatives and the attribution probes live in tools/exp/probes.patch)
constexpr int QBA_WIDE_QPT = 2;      // quads per thread-step of the wide kernels (one 8-B / 4-B row vector)
constexpr int QBA_PAIRWISE = 1;      // closed sampler: a quad's two pairs one after the other (fewer live VGPRs)
constexpr int QBA_DEF_PAIRWISE = 0;  // ... in the deferred (configs[1]) kernel: interleaved, more ILP at 6 waves
constexpr int QBA_DEF_WAVES = 6;     // deferred kernel: waves per SIMD it is compiled for
constexpr int QBA_GRID_QPT = 2;      // quads per thread the grid is sized for
constexpr int QBA_RED_ROWS = 32;     // slab rows per reduce workgroup

template <int NP>
struct QCfg {
  static constexpr int G = NP + 1;  // measured groups (n parties + the commander's extra)
  static constexpr int NQ = (G <= 2) ? 1 : (G <= 4) ? 2 : (G <= 8) ? 3 : 4;
  static constexpr int N = G * NQ;  // qubits of the circuit (tfg.py:44)
  static constexpr int W = 1 << NQ;  // |W| (tfg.py:318)
  static constexpr int HB = W * G * W;    // H as returned: [u][g][x]
  static constexpr int WP = W + 1;        // LDS row stride of H: +1 word spreads banks
  static constexpr int HBL = W * G * WP;  // H as counted in LDS / the slab
  static constexpr int CB = W * G * G;      // C as returned: [u][g][h]
  static constexpr int CP = G * (G - 1) / 2; // pairs g < h, as counted
  static constexpr int CBL = W * CP;
  static constexpr int STATS = 2;  // [0] Q entries with a value >= W (invalid), [1] spare
  static constexpr int NBINS = HBL + CBL + STATS;
  static constexpr int NBP = (NBINS + 3) & ~3;  // slab row stride (16-B rows)
  // counted index of the pair g < h
  __host__ __device__ static constexpr int pidx(int g, int h) { return g * (2 * G - g - 1) / 2 + (h - g - 1); }
  __host__ __device__ static constexpr int hidx(int u, int g, int x) { return (u * G + g) * WP + x; }
  // number of not-Q table bytes of the canonical program (ceil(n*nQ/8))
  static constexpr int NFB = (NP * NQ + 7) / 8;
  static constexpr int LASTB = NP * NQ - 8 * (NFB - 1);
  using Out = typename std::conditional<(N <= 32), uint32_t, uint64_t>::type;
  static constexpr Out M = (Out)(W - 1);
  __host__ __device__ static constexpr int shift(int g) { return N - (g + 1) * NQ; }
  __host__ __device__ static constexpr Out identity() {
    Out p = 0;
    for (int g = 1; g <= NP; ++g) p |= (Out)g << shift(g);
    return p;
  }
};

// ---------------------------------------------------------------------------
// random words of one entry (schedule documented in qba_internal.h)
// ---------------------------------------------------------------------------
// Words beyond block 0 (only programs with many or non-uniform factors):
// kept out of line so the common path stays small.
__device__ __attribute__((noinline)) uint32_t qba_word_ext(int kk, uint32_t elo, uint32_t ehi,
                                                           uint32_t k0, uint32_t k1) {
  const QbaU4 y = qba_philox(elo, ehi, 1u + (uint32_t)(kk >> 2), 0u, k0, k1);
  const int s = kk & 3;
  return s == 0 ? y.x : (s == 1 ? y.y : (s == 2 ? y.z : y.w));
}

// Word k of the table stream (k is wave-uniform).  Block-0 words are picked
// with uniform masks so the selection stays in registers.
__device__ __forceinline__ uint32_t qba_word(int kind, int k, const QbaU4 &x, uint32_t elo,
                                             uint32_t ehi, uint32_t k0, uint32_t k1) {
  k = __builtin_amdgcn_readfirstlane(k);
  const int base = kind ? 1 : 3;
  if (k >= base) return qba_word_ext(k - base, elo, ehi, k0, k1);
  const uint32_t m0 = k == 0 ? ~0u : 0u, m1 = k == 1 ? ~0u : 0u, m2 = k == 2 ? ~0u : 0u;
  return (x.y & m0) | (x.z & m1) | (x.w & m2);
}

template <typename Out>
__device__ __forceinline__ Out qba_draw(const QbaProgram &P, int kind, const QbaU4 &x,
                                        uint32_t elo, uint32_t ehi, uint32_t k0, uint32_t k1,
                                        const uint64_t *pat, const uint64_t *apat,
                                        const uint64_t *thr) {
  Out out = 0;
  const int nf = P.nfac;
  for (int f = 0; f < nf; ++f) {
    const QbaFactor F = P.fac[f];
    const uint32_t wv = qba_word(kind, F.col_word, x, elo, ehi, k0, k1);
    const uint32_t col = (wv >> F.col_shift) & ((1u << F.bits) - 1u);
    uint64_t p = pat[F.offset + col];
    if (!F.uniform) {
      const uint32_t u = qba_word(kind, F.u_word, x, elo, ehi, k0, k1);
      if ((uint64_t)u >= thr[F.offset + col]) p = apat[F.offset + col];
    }
    out ^= (Out)p;
  }
  return out;
}

// Uniform permutation pi of 1..n in the outcome layout (field g = pi(g)):
// mixed-radix digits of floor(F * n! / 2^64) drive Fisher-Yates; Lemire's
// test on the final fraction makes it exactly uniform.
template <int NP>
__device__ __forceinline__ bool qba_perm(uint64_t F, uint64_t t, typename QCfg<NP>::Out &mask) {
  using C = QCfg<NP>;
  using Out = typename C::Out;
  Out P = C::identity();
#pragma unroll
  for (int i = NP; i >= 2; --i) {
    const uint64_t lo = (F & 0xffffffffull) * (uint64_t)i;
    const uint64_t hi = (F >> 32) * (uint64_t)i + (lo >> 32);
    const uint32_t d = (uint32_t)(hi >> 32);
    F = (hi << 32) | (lo & 0xffffffffull);
    const int si = C::shift(i);
    const int sj = C::N - (int)(d + 2) * C::NQ;  // field j = 1 + d
    const Out a = (P >> si) & C::M;
    const Out b = (P >> sj) & C::M;
    const Out tt = a ^ b;
    P ^= (tt << si) | (tt << sj);
  }
  mask = P;
  return F >= t;
}

template <int NP>
__device__ __forceinline__ typename QCfg<NP>::Out qba_sample_entry(
    uint64_t e, uint32_t k0, uint32_t k1, const QbaProgramSet *__restrict__ ps,
    const uint64_t *pat, const uint64_t *apat, const uint64_t *thr) {
  using Out = typename QCfg<NP>::Out;
  const uint32_t elo = (uint32_t)e, ehi = (uint32_t)(e >> 32);
  const QbaU4 x = qba_philox(elo, ehi, 0u, 0u, k0, k1);
  Out out;
  if (x.x & 1u) {  // Q-correlated shot (tfg.py:69, 74)
    const uint64_t t = ps->prog[1].perm_t;
    Out mask;
    bool ok = qba_perm<NP>((uint64_t)x.z | ((uint64_t)x.w << 32), t, mask);
    for (uint32_t a = 1; !ok; ++a) {  // probability ~ n!/2^64 per entry
      const QbaU4 y = qba_philox(elo, ehi, 0x80000000u + a, 0u, k0, k1);
      ok = qba_perm<NP>((uint64_t)y.x | ((uint64_t)y.y << 32), t, mask);
    }
    out = qba_draw<Out>(ps->prog[1], 1, x, elo, ehi, k0, k1, pat, apat, thr) ^ mask;
  } else {  // not-Q-correlated shot (tfg.py:72)
    out = qba_draw<Out>(ps->prog[0], 0, x, elo, ehi, k0, k1, pat, apat, thr);
  }
  return out;
}

// Canonical programs (QbaProgramSet::canonical): every table column is a byte
// of the stream, so the factor loop is fully unrolled at compile time.
template <int NP>
__device__ __forceinline__ typename QCfg<NP>::Out qba_sample_entry_fast(
    uint64_t e, uint32_t k0, uint32_t k1, uint64_t perm_t, int qoff, const uint64_t *pat) {
  using C = QCfg<NP>;
  using Out = typename C::Out;
  const uint32_t elo = (uint32_t)e, ehi = (uint32_t)(e >> 32);
  const QbaU4 x = qba_philox(elo, ehi, 0u, 0u, k0, k1);
  Out out;
  if (x.x & 1u) {
    Out mask;
    bool ok = qba_perm<NP>((uint64_t)x.z | ((uint64_t)x.w << 32), perm_t, mask);
    for (uint32_t a = 1; !ok; ++a) {
      const QbaU4 y = qba_philox(elo, ehi, 0x80000000u + a, 0u, k0, k1);
      ok = qba_perm<NP>((uint64_t)y.x | ((uint64_t)y.y << 32), perm_t, mask);
    }
    out = (Out)pat[qoff + (x.y & (uint32_t)C::M)] ^ mask;
  } else {
    out = 0;
#pragma unroll
    for (int f = 0; f < C::NFB; ++f) {
      const uint32_t w = f < 4 ? x.y : (f < 8 ? x.z : x.w);
      const uint32_t bits = f < C::NFB - 1 ? 8 : C::LASTB;
      const uint32_t col = (w >> (8 * (f & 3))) & ((1u << bits) - 1u);
      out ^= (Out)pat[256 * f + col];
    }
  }
  return out;
}

// ---------------------------------------------------------------------------
// Closed-form sampler (QbaProgramSet::closed; n <= 11).  Entries come in
// pairs: entry e uses half h = e & 1 of block
//   x = philox(ctr = {p_lo, p_hi, 0, 0}, key = seed),  p = e >> 1,
// i.e. the 64 bits w0 = x[2h], w1 = x[2h+1].  isQ = w0 & 1.
//   not-Q: values v_0..v_10 = the nQ low bits of the nibbles at bits
//          {8,16,24, 4,12,20,28} of w1 then {4,12,20,28} of w0;
//          group g >= 1 takes v_{g-1}, group 0 takes v_0 (= group 1,
//          tfg.py:15-22).
//   Q:     r = (w0 >> 1) & (W-1).  The rank word F is w1 if
//          F * n! mod 2^32 >= 2^32 mod n!, else w0 & ~31 (bits 5..31, a
//          27-bit fraction) if F * n! mod 2^32 >= (2^27 mod n!) << 5 (Lemire on
//          27 bits), else the words of philox(ctr = {p_lo, p_hi, 0x80000000 + a,
//          h}) for a = 1, 2, ... in order (32-bit test): exactly uniform.
//          (iA, iB, iC) = the mixed-radix digits of floor(F * n! / 2^32) in
//          radices (RA, RB, RC) [F * RA = iA:F1, F1 * RB = iB:F2, F2 * RC =
//          iC:F3], pi = stage A[iA] with its window permuted by B[iB] then
//          C[iC]; group g = r ^ pi(g) (tfg.py:25-40).
// Values are produced as bytes, group g in byte g % 4 of word g / 4.
// ---------------------------------------------------------------------------

template <int NP>
struct CF {
  using C = QCfg<NP>;
  static constexpr int G = NP + 1;
  static constexpr int ND = (G + 3) / 4;          // words per entry
  static constexpr int WIN = NP >= 8 ? 1 : 0;      // first word of the 8-byte window
  static constexpr int K = NP >= 8 ? NP - 3 : NP;  // window positions that move
  static constexpr uint32_t fact(int a, int b) {   // a * (a-1) * ... * b
    uint32_t x = 1;
    for (int i = a; i >= b; --i) x *= (uint32_t)i;
    return x;
  }
  static constexpr uint32_t RA = NP >= 8 ? fact(NP, NP - 2) : 1u;
  static constexpr uint32_t RB = K >= 2 ? fact(K, (K - 3 > 2 ? K - 3 : 2)) : 1u;
  static constexpr uint32_t RC = K >= 6 ? fact(K - 4, 2) : 1u;
  static constexpr uint32_t NFACT = fact(NP, 2);
  static constexpr uint32_t T32 = (uint32_t)((1ull << 32) % NFACT);
  static constexpr uint32_t T27 = (uint32_t)(((1ull << 27) % NFACT) << 5);  // 27-bit test, scaled
  static constexpr int OFFB = 4 * (int)RA;            // in words
  static constexpr int OFFC = OFFB + 2 * (int)RB;
  static constexpr int WORDS = OFFC + (int)RC;  // C keeps only its hi selector
  static constexpr uint32_t M4 = (uint32_t)(C::W - 1) * 0x01010101u;
};

__device__ __forceinline__ uint32_t qba_perm_b(uint32_t hi, uint32_t lo, uint32_t sel) {
  return __builtin_amdgcn_perm(hi, lo, sel);
}

// Lemire acceptance of a 32-bit rank word against threshold T (scaled)
template <int NP>
__device__ __forceinline__ bool qba_accept(uint32_t F, uint32_t T) {
  return F * CF<NP>::NFACT >= T;
}

// One entry from its 64 random bits (w0, w1), in two phases so that a quad's
// table reads are issued together: qba_closed_rank (not-Q words, Lemire rank;
// (p, h) identify the entry for the rare retry) then qba_closed_finish.
struct QbaClosed {
  uint32_t nqr[4];  // not-Q words before the nibble mask (word 0 already masked)
  uint32_t rank, w0;
};

template <int NP>
__device__ __forceinline__ void qba_closed_rank(uint32_t w0, uint32_t w1, uint64_t p, uint32_t h,
                                                uint32_t k0, uint32_t k1, QbaClosed &c) {
  using F = CF<NP>;
  // group g >= 1 = nibble g of (w1 low nibbles, w1 high nibbles, w0 high
  // nibbles) in byte order, group 0 = group 1: the masked words ARE the byte
  // layout, one v_perm in all (w0's low nibbles carry isQ and r); unmasked:
  // qba_closed_finish masks every not-Q word with ~qm & M4 anyway
  c.nqr[0] = qba_perm_b(w1, w1, 0x03020101u);
  c.nqr[1] = w1 >> 4;
  c.nqr[2] = w0 >> 4;
  c.nqr[3] = 0u;
  c.w0 = w0;
  // w1 is the rank word unless its Lemire test fails (P = (2^32 mod n!) /
  // 2^32, 0.56 % at n = 11): the fallback words are chosen inside the rare
  // branch, not by a select on every entry.  The branch is tested for the
  // whole wave first (some lane fails in ~30 % of the entries): the common
  // path is one compare and one scalar branch, not the divergent branch's
  // exec-mask bookkeeping on every entry (-2.5 % cycles, VALU 77.6 -> 75.3
  // per entry, profiles/r5/uniform_branch)
  uint32_t rank = w1;
  const bool bad = !qba_accept<NP>(w1, F::T32);
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(bad) != 0, 0))
  if (bad) {
    rank = w0 & ~31u;
    // both tests failed (P = 6e-4 per entry at n = 11): words of further
    // Philox blocks, in order.  A not-Q entry's rank is discarded, so only
    // Q-correlated entries retry.  (Done lane by lane on the scalar unit
    // instead, the retry freed the loop of a scratch reload but cost SGPRs
    // and 2 % more cycles: profiles/r5/ab_retry.)
    if (!qba_accept<NP>(rank, F::T27) && (w0 & 1u)) {
      bool ok = false;
      for (uint32_t t = 1; !ok; ++t) {
        const QbaU4 y = qba_philox((uint32_t)p, (uint32_t)(p >> 32), 0x80000000u + t, h, k0, k1);
        const uint32_t cand[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (!ok && qba_accept<NP>(cand[i], F::T32)) {
            ok = true;
            rank = cand[i];
          }
      }
    }
  }
  // a not-Q entry discards its table words (qba_closed_finish selects its
  // nibbles): rank 0 sends its three reads to one address per table, served
  // as an LDS broadcast, so only the Q lanes' random reads meet bank conflicts
  rank &= (uint32_t)__builtin_amdgcn_sbfe((int)w0, 0, 1);
  c.rank = rank;
}

template <int NP>
__device__ __forceinline__ void qba_closed_finish(const QbaClosed &c, const uint4 &A, const uint2 &sB,
                                                  uint32_t sC, uint32_t (&D)[CF<NP>::ND]) {
  using F = CF<NP>;
  // A.w (zero in the table) is kept alive by an empty asm, so the read stays
  // one ds_read_b128 (4 LDS cycles, a ds_read_b96 takes 8) without an OR
  uint32_t q[4] = {A.x, A.y, A.z, A.w};
  asm volatile("" ::"v"(A.w));
  const uint32_t y0 = qba_perm_b(q[F::WIN + 1], q[F::WIN], sB.x);
  uint32_t y1 = qba_perm_b(q[F::WIN + 1], q[F::WIN], sB.y);
  if constexpr (F::RC > 1) y1 = qba_perm_b(y1, y0, sC);  // stage C moves window bytes 4..7 only
  q[F::WIN] = y0;
  q[F::WIN + 1] = y1;
  // r in every byte: one v_perm (byte 0 to all four) instead of a quarter-rate
  // v_mul_lo_u32 by 0x01010101
  const uint32_t R = qba_perm_b(0u, (c.w0 >> 1) & (uint32_t)(QCfg<NP>::W - 1), 0u);
  // all ones for a Q-correlated entry: one v_bfe_i32, opaque so that each
  // word's select stays one v_bitop3 (qm ? q ^ R : nq) instead of and + cmp
  // for a mask plus a v_cndmask per word
  uint32_t qm = (uint32_t)__builtin_amdgcn_sbfe((int)c.w0, 0, 1);
  asm("" : "+v"(qm));
  // not-Q words masked by ONE shared ~qm & M4, then one v_and_or per word:
  // D = (nq_raw & nqm) | (qm & (q ^ R))  (-0.2 VALU/entry, profiles/r3/ab32_microopts_and_stores.txt)
  uint32_t nqm = ~qm & F::M4;
  asm("" : "+v"(nqm));
#pragma unroll
  for (int i = 0; i < F::ND; ++i) {
    uint32_t t = qm & (q[i] ^ R);
    asm("" : "+v"(t));
    D[i] = (c.nqr[i] & nqm) | t;
  }
}

// Stage table indices of a rank and the LDS reads.
template <int NP>
__device__ __forceinline__ void qba_closed_tables(uint32_t rank, const uint32_t *__restrict__ pl,
                                                  uint4 &A, uint2 &sB, uint32_t &sC) {
  using F = CF<NP>;
  // Each digit is the high word of one v_mad_u64_u32; the empty asm makes
  // it opaque so its table offset is ONE v_lshl_add (without it the compiler
  // rebuilt digit * stride from the 64-bit product: alignbit + and + shift).
  uint32_t iA = 0, rem = rank;
  if constexpr (F::RA > 1) {
    const uint64_t pa = (uint64_t)rem * F::RA;
    iA = (uint32_t)(pa >> 32);
    rem = (uint32_t)pa;
    asm("" : "+v"(iA));
  }
  const uint64_t pb = (uint64_t)rem * F::RB;
  uint32_t iB = (uint32_t)(pb >> 32);
  asm("" : "+v"(iB));
  uint32_t iC = F::RC > 1 ? (uint32_t)(((uint64_t)(uint32_t)pb * F::RC) >> 32) : 0u;
  if constexpr (F::RC > 1) asm("" : "+v"(iC));
  A = *reinterpret_cast<const uint4 *>(pl + 4 * iA);
  sB = *reinterpret_cast<const uint2 *>(pl + F::OFFB + 2 * iB);
  sC = F::RC > 1 ? pl[F::OFFC + iC] : 0u;
}

template <int NP>
__device__ __forceinline__ void qba_closed_half(uint32_t w0, uint32_t w1, uint64_t p, uint32_t h,
                                                uint32_t k0, uint32_t k1,
                                                const uint32_t *__restrict__ pl,
                                                uint32_t (&D)[CF<NP>::ND]) {
  QbaClosed c;
  qba_closed_rank<NP>(w0, w1, p, h, k0, k1, c);
  uint4 A;
  uint2 sB;
  uint32_t sC;
  qba_closed_tables<NP>(c.rank, pl, A, sB, sC);
  qba_closed_finish<NP>(c, A, sB, sC, D);
}

// Entry e on its own (odd pair alignment, tails): the half of its pair's block.
template <int NP>
__device__ __forceinline__ void qba_closed_entry(uint64_t e, uint32_t k0, uint32_t k1,
                                                 const uint32_t *__restrict__ pl,
                                                 uint32_t (&D)[CF<NP>::ND]) {
  const uint64_t p = e >> 1;
  const uint32_t h = (uint32_t)e & 1u;
  const QbaU4 x = qba_philox((uint32_t)p, (uint32_t)(p >> 32), 0u, 0u, k0, k1);
  qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, p, h, k0, k1, pl, D);
}

// Outcome word of the table samplers -> byte layout.
template <int NP>
__device__ __forceinline__ void qba_out_to_d(typename QCfg<NP>::Out o, uint32_t (&D)[CF<NP>::ND]) {
  using C = QCfg<NP>;
#pragma unroll
  for (int i = 0; i < CF<NP>::ND; ++i) D[i] = 0;
#pragma unroll
  for (int g = 0; g < C::G; ++g)
    D[g / 4] |= ((uint32_t)(o >> C::shift(g)) & (uint32_t)C::M) << (8 * (g % 4));
}

// Samplers of one entry into the byte layout
enum { QBA_S_GENERAL = 0, QBA_S_FAST = 1, QBA_S_CLOSED = 2 };

template <int NP, int SAMP>
__device__ __forceinline__ void qba_entry_d(uint64_t e, uint32_t k0, uint32_t k1,
                                            const QbaProgramSet *__restrict__ ps,
                                            const uint64_t *pat, const uint64_t *apat,
                                            const uint64_t *thr, const uint32_t *pl,
                                            uint32_t (&D)[CF<NP>::ND]) {
  if constexpr (SAMP == QBA_S_CLOSED) {
    qba_closed_entry<NP>(e, k0, k1, pl, D);
  } else if constexpr (SAMP == QBA_S_FAST) {
    qba_out_to_d<NP>(qba_sample_entry_fast<NP>(e, k0, k1, ps->prog[1].perm_t, ps->prog[0].table_len, pat), D);
  } else {
    qba_out_to_d<NP>(qba_sample_entry<NP>(e, k0, k1, ps, pat, apat, thr), D);
  }
}

// Sample one quad (entries [c0, c0+4) of the launch) into the byte layout.
template <int NP, int SAMP, bool TAIL, int PW = QBA_PAIRWISE>
__device__ __forceinline__ void qba_sample_quad(uint32_t c0, int valid, uint64_t first, uint32_t k0,
                                                uint32_t k1, const QbaProgramSet *__restrict__ ps,
                                                const uint64_t *pat, const uint64_t *apat,
                                                const uint64_t *thr, const uint32_t *pl,
                                                uint32_t (&D)[4][CF<NP>::ND]) {
  constexpr int ND = CF<NP>::ND;
  if constexpr (SAMP == QBA_S_CLOSED && !TAIL) {
    // PW: each pair's table reads and finish before the next pair's Philox
    // (fewer live VGPRs: the 8-wave list kernel); else the quad's two Philox
    // blocks interleaved (more ILP: the deferred kernel's low-occupancy step)
    if (PW && !(first & 1)) {
      const uint32_t phi = (uint32_t)(first >> 33);
      const uint32_t plo = (uint32_t)(first >> 1) + (c0 >> 1);
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        QbaClosed cl[2];
        const uint64_t p = ((uint64_t)phi << 32) | (uint64_t)(plo + (uint32_t)jp);
        // the 20 round keys loop-invariant in SGPRs (SGPR budget allows them
        // since round 5: 108 instead of 158 SALU per thread-step, cycles -1 %,
        // profiles/r5/keys_sgpr)
        const QbaU4 x = qba_philox_k<false>(plo + (uint32_t)jp, phi, 0u, 0u, k0, k1);
        qba_closed_rank<NP>(x.x, x.y, p, 0u, k0, k1, cl[0]);
        qba_closed_rank<NP>(x.z, x.w, p, 1u, k0, k1, cl[1]);
        uint4 A[2];
        uint2 sB[2];
        uint32_t sC[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) qba_closed_tables<NP>(cl[j].rank, pl, A[j], sB[j], sC[j]);
#pragma unroll
        for (int j = 0; j < 2; ++j) qba_closed_finish<NP>(cl[j], A[j], sB[j], sC[j], D[2 * jp + j]);
      }
      return;
    }
    if (!(first & 1)) {  // wave-uniform: the quad is two whole pairs
      QbaClosed cl[4];
      // A launch never crosses a multiple of 2^33 entries (dispatch splits
      // there), so the pair counter's high word is the launch's and the low
      // word never carries: p_hi stays in an SGPR, Philox's round 1 and half
      // of round 2 are scalar.
      const uint32_t phi = (uint32_t)(first >> 33);
      const uint32_t plo = (uint32_t)(first >> 1) + (c0 >> 1);
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        const uint64_t p = ((uint64_t)phi << 32) | (uint64_t)(plo + (uint32_t)jp);
        const QbaU4 x = qba_philox(plo + (uint32_t)jp, phi, 0u, 0u, k0, k1);
        qba_closed_rank<NP>(x.x, x.y, p, 0u, k0, k1, cl[2 * jp]);
        qba_closed_rank<NP>(x.z, x.w, p, 1u, k0, k1, cl[2 * jp + 1]);
      }
      uint4 A[4];
      uint2 sB[4];
      uint32_t sC[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) qba_closed_tables<NP>(cl[j].rank, pl, A[j], sB[j], sC[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) qba_closed_finish<NP>(cl[j], A[j], sB[j], sC[j], D[j]);
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < valid) {
      qba_entry_d<NP, SAMP>(first + c0 + j, k0, k1, ps, pat, apat, thr, pl, D[j]);
    } else {
#pragma unroll
      for (int i = 0; i < ND; ++i) D[j][i] = 0;
    }
  }
}

// Stage the program's tables in LDS; returns the histogram base after them
// (their bytes on the host: table_lds, qba_lists_launch.h).
template <int NP, int MODE, int SAMP, int BS>
__device__ __forceinline__ uint32_t *qba_stage(const QbaProgramSet *__restrict__ ps, uint64_t *lds,
                                               const uint64_t *&pat, const uint64_t *&apat,
                                               const uint64_t *&thr, const uint32_t *&pl) {
  pat = apat = thr = lds;
  pl = reinterpret_cast<const uint32_t *>(lds);
  uint32_t *hist = reinterpret_cast<uint32_t *>(lds);
  if constexpr (MODE != 2 && SAMP == QBA_S_CLOSED) {
    // at a compile-time offset: the loads issue without reading the header
    const uint32_t *src = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(ps) + QBA_PERM_OFF);
    uint32_t *dst = reinterpret_cast<uint32_t *>(lds);
    // 16-B buffer loads, all issued before the first LDS write: one memory
    // round trip per workgroup (the image pads the tables to whole 16-B
    // words, qba_plan_image).  A buffer load past the tables' W4 words returns
    // zero, so every lane loads unconditionally at a 32-bit offset; only the
    // LDS writes are guarded.  (Plain loads with a guard were serialised by
    // the compiler -- load, wait, write, per word -- or went to scratch.)
    constexpr int W4 = (CF<NP>::WORDS + 3) / 4, PER = (W4 + BS - 1) / BS;
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(src), (short)0, W4 * 16, 0x00020000);
    v4u v[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, (threadIdx.x + k * BS) * 16u, 0, 0);
    // the guarded writes' loads are not sunk into their branches
#pragma unroll
    for (int k = 0; k < PER; ++k) asm volatile("" ::"v"(v[k]));
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (threadIdx.x + k * BS < W4) d4[threadIdx.x + k * BS] = make_uint4(v[k].x, v[k].y, v[k].z, v[k].w);
    hist = dst + ((CF<NP>::WORDS + 3) & ~3);
  } else if constexpr (MODE != 2) {
    const int T = ps->table_total;
    const uint64_t *tab = reinterpret_cast<const uint64_t *>(reinterpret_cast<const char *>(ps) + ps->tab_off);
    const int ntab = ps->any_nonuniform ? 3 * T : T;
    for (int i = threadIdx.x; i < ntab; i += BS) lds[i] = tab[i];
    apat = lds + T;
    thr = lds + 2 * T;
    hist = reinterpret_cast<uint32_t *>(lds + ((ntab + 1) & ~1));  // 16-B aligned
  }
  return hist;
}
