// qba_lists_count.h -- counting for the list kernels (qba_lists_kern.h): one
// entry into the classic 32-bit bins (qba_count_d), the wave-level Q-entry
// queue, the pair bins of the fused n = 11 kernel and their flush
// (qba_pb_flush).  Takes QCfg, CF, qba_perm_b and the byte layout from
// qba_lists_sample.h; needs nothing from qba_lists_step.h.
#pragma once
#include "qba_lists_sample.h"

// |P_u| = sum_x H[u][0][x]; H[u][1][x] = [x == u] |P_u| (group 1's own bin is
// never counted: L1 = u by definition of the bin).
template <int NP, typename T>
__device__ __forceinline__ int64_t qba_psize(const T *bins, int u) {
  using C = QCfg<NP>;
  int64_t s = 0;
  for (int x = 0; x < C::W; ++x) s += (int64_t)bins[C::hidx(u, 0, x)];
  return s;
}
template <int NP, typename T>
__device__ __forceinline__ int64_t qba_hval(const T *bins, int i) {  // i indexes H[u][g][x]
  using C = QCfg<NP>;
  const int u = i / (C::G * C::W), g = (i / C::W) % C::G, x = i % C::W;
  if (g == 1) return x == u ? qba_psize<NP>(bins, u) : 0;
  return (int64_t)bins[C::hidx(u, g, x)];
}

// Inline asm in this file (here and qba_add_byte below) reads and writes
// VGPRs only: no SGPR operand is written by VALU inside an asm block, so the
// VALU-writes-SGPR -> VMEM-reads-SGPR hazard the compiler cannot see through
// asm (the cause of the faulting saddr-store experiment)
// does not arise.  Keep any new asm VGPR-only.
// v_pk_lshlrev_b16: each 16-bit half of `one` shifted by the low 4 bits of
// the same half of `amt` (the upper bits of the half are ignored by the ALU).
__device__ __forceinline__ uint32_t qba_pk_onehot(uint32_t amt, uint32_t one) {
  uint32_t r;
  asm("v_pk_lshlrev_b16 %0, %1, %2" : "=v"(r) : "v"(amt), "v"(one));
  return r;
}

// lo | hi of a word's two 16-bit halves in ONE op (an SDWA v_or with the
// upper half zeroed): the union of two 16-bit one-hot sets
__device__ __forceinline__ uint32_t qba_fold16(uint32_t u) {
  uint32_t r;
  asm("v_or_b32_sdwa %0, %1, %1 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1"
      : "=v"(r) : "v"(u));
  return r;
}

typedef __attribute__((address_space(3))) uint32_t qba_lds_u32;  // LDS word (32-bit address)

// base + byte b of x in one VALU op (v_add_u32 with an SDWA byte select)
__device__ __forceinline__ uint32_t qba_add_byte(uint32_t base, uint32_t x, int b) {
  uint32_t r;
  switch (b) {
    case 0: asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(base), "v"(x)); break;
    case 1: asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(base), "v"(x)); break;
    case 2: asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(base), "v"(x)); break;
    default: asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(r) : "v"(base), "v"(x)); break;
  }
  return r;
}

// value of group g (runtime g) of an entry whose byte-layout words are w0..w3
__device__ __forceinline__ uint32_t qba_byte_of(int g, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
  const int i = g >> 2;
  const uint32_t w = i == 0 ? w0 : i == 1 ? w1 : i == 2 ? w2 : w3;
  return (w >> (8 * (g & 3))) & 0xffu;
}

// ---------------------------------------------------------------------------
// count one entry (group g = byte g % 4 of D[g / 4])
//   Q-correlated iff L0 != L1 (tfg.py:327); u = L1 (tfg.py:182);
//   H[u][g][L_g] += 1 for every g; C[u][g][h] += 1 for every equal pair --
//   every counted entry is tested (its distinct-value count: the union of
//   16-bit one-hots), the pair loop runs only when that count is below n+1.
// ---------------------------------------------------------------------------
template <int NP>
__device__ __forceinline__ void qba_count_d(const uint32_t (&D)[CF<NP>::ND], uint32_t one,
                                            uint32_t *hist, bool in_range, bool known_q = false,
                                            uint32_t hoff = 0xffffffffu) {
  using C = QCfg<NP>;
  using F = CF<NP>;
  const uint32_t l0 = D[0] & 0xffu, l1 = (D[0] >> 8) & 0xffu;
  if (!known_q && l0 == l1) return;  // the Q-entry queue holds only entries with L0 != L1
  uint32_t bad = 0;
#pragma unroll
  for (int i = 0; i < F::ND; ++i) {
    uint32_t vm = 0;  // bits that must be clear: value bits >= W of the real groups
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (4 * i + b < C::G) vm |= (0xffu & ~(uint32_t)(C::W - 1)) << (8 * b);
    bad |= D[i] & vm;
  }
  if (in_range) bad = 0;  // the caller's quad-level test found no value >= W
  if (bad) {
    atomicAdd(&hist[C::HBL + C::CBL + 0], 1u);
    return;
  }
  // hoff: the histogram's LDS byte address held in a VGPR by the caller (the
  // row base is then one v_mad_u32_u24 with the stride in an SGPR).  The row
  // index is taken to nq bits (the same single v_bfe): a trusted value is
  // < W already, and whatever the bytes hold the address stays inside this
  // workgroup's histogram + queue area (x < 256 adds at most 1 KiB).  An
  // experiment build that fed unmasked words here once indexed rows up to
  // 255 * 816 B past the histogram, beyond the LDS allocation, and faulted.
  const uint32_t l1r = (D[0] >> 8) & (uint32_t)(C::W - 1);
  if (hoff == 0xffffffffu) hoff = (uint32_t)(uintptr_t)(qba_lds_u32 *)hist;
  const uint32_t hb = hoff + l1r * (uint32_t)(C::G * C::WP * 4);
#pragma unroll
  for (int i = 0; i < F::ND; ++i) {
    const uint32_t E = D[i] << 2;  // byte b = 4 * value (< 64: no carry into the next byte)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int g = 4 * i + b;
      if (g < C::G && g != 1) {  // H[u][1][x] = [x == u] |P_u|, derived when reduced
        const uint32_t a = qba_add_byte(hb, E, b);
        atomicAdd((uint32_t *)((qba_lds_u32 *)(uintptr_t)a + g * C::WP), 1u);
      }
    }
  }
  // Cond3 (tfg.py:96-98): distinct iff the union of the values' 16-bit
  // one-hots (two per v_pk_lshlrev_b16) has n+1 bits
  uint32_t U = 0;
#pragma unroll
  for (int i = 0; i < F::ND; ++i) {
    uint32_t mp = 0, mq = 0;
    if (4 * i + 0 < C::G) mp |= 0x0000ffffu;
    if (4 * i + 2 < C::G) mp |= 0xffff0000u;
    if (4 * i + 1 < C::G) mq |= 0x0000ffffu;
    if (4 * i + 3 < C::G) mq |= 0xffff0000u;
    U |= (qba_pk_onehot(D[i], one) & mp) | (qba_pk_onehot(D[i] >> 8, one) & mq);
  }
  if (__popc(qba_fold16(U)) != C::G) {  // some pair collides: exact slow path
    // a compact loop (values picked by selects, no private array): this
    // path is rare and unrolling it would multiply the kernel's code size
    uint32_t *c = hist + C::HBL + l1r * C::CP;
    const uint32_t w0 = D[0], w1 = F::ND > 1 ? D[F::ND > 1 ? 1 : 0] : 0u,
                   w2 = F::ND > 2 ? D[F::ND > 2 ? 2 : 0] : 0u, w3 = F::ND > 3 ? D[F::ND > 3 ? 3 : 0] : 0u;
    int pi = 0;
#pragma nounroll
    for (int g = 0; g < C::G; ++g) {
      const uint32_t lg = qba_byte_of(g, w0, w1, w2, w3);
#pragma nounroll
      for (int k = g + 1; k < C::G; ++k, ++pi)
        if (lg == qba_byte_of(k, w0, w1, w2, w3)) atomicAdd(&c[pi], 1u);
    }
  }
}

// Every value of a quad of entries < W?  One OR over the quad's transposed
// row words (about 2 VALU per entry) instead of a range test per entry; a
// wave with any out-of-range value takes the per-entry test.
template <int NP>
__device__ __forceinline__ bool qba_rows_in_range(const uint32_t *row) {
  using C = QCfg<NP>;
  uint32_t o = 0;
#pragma unroll
  for (int g = 0; g < C::G; ++g) o |= row[g];
  return !__any((o & (0xffu & ~(uint32_t)(C::W - 1)) * 0x01010101u) != 0u);  // wave-uniform
}

template <int NP>
__device__ __forceinline__ void qba_count_quad(const uint32_t (&D)[4][CF<NP>::ND], int valid,
                                               uint32_t *hist, const uint32_t *row) {
  const uint32_t one = 0x00010001u;
  if (qba_rows_in_range<NP>(row)) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < valid) qba_count_d<NP>(D[j], one, hist, true);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < valid) qba_count_d<NP>(D[j], one, hist, false);
  }
}

// ---------------------------------------------------------------------------
// Wave-level Q-entry queue: only Q entries are counted, so with
// per-entry counting half the lanes of every count instruction idle.  Each
// wave appends its Q entries (byte-layout words, SoA in LDS) to a ring of
// QBA_QCAP slots and counts them 64 at a time with every lane busy.  All
// queue state is wave-uniform and pushes / drains run with the full wave
// (the callers keep exec full), so no entry is lost or counted twice.
// ---------------------------------------------------------------------------
#define QBA_QCAP 128  // ring slots per wave (two drains' worth)
// L0 != L1 (tfg.py:327) for an active lane: am = 0xff on active lanes, 0 on
// the idle lanes of the last step (one v_bitop3 + compare straight into VCC)
template <int NP>
__device__ __forceinline__ bool qba_isq_d(const uint32_t (&D)[CF<NP>::ND], uint32_t am = 0xffu) {
  return ((D[0] ^ (D[0] >> 8)) & am) != 0u;
}
struct QbaWaveQ {
  uint32_t base;      // LDS byte address of this wave's ring [ND][QBA_QCAP] words (aligned to 4 QBA_QCAP B)
  uint32_t tail, qn;  // wave-uniform: first queued slot (not reduced mod QBA_QCAP), queued entries
  uint32_t hoff;      // LDS byte address of the histogram, kept in a VGPR (see qba_count_d)
};

// LDS byte address of ring slot s (any integer: taken mod QBA_QCAP); the
// ring's alignment makes the slot bits an OR into the base
__device__ __forceinline__ uint32_t qba_q_addr(const QbaWaveQ &q, uint32_t s) {
  return ((s & (QBA_QCAP - 1)) << 2) | q.base;
}
__device__ __forceinline__ qba_lds_u32 *qba_lds(uint32_t addr) {
  return reinterpret_cast<qba_lds_u32 *>(static_cast<uintptr_t>(addr));
}

// The queue area starts after the histogram, aligned to one ring (the host
// sizes the launch's LDS with QBA_QCAP * 4 bytes of slack for it:
// qba_count_lds).
template <int NP>
__device__ __forceinline__ uint32_t qba_queue_base(uint32_t *hist) {
  const uint32_t h = (uint32_t)(uintptr_t)(qba_lds_u32 *)hist + ((QCfg<NP>::NBP + 3) & ~3) * 4;
  return (h + QBA_QCAP * 4 - 1) & ~(uint32_t)(QBA_QCAP * 4 - 1);
}
// LDS bytes of a counting workgroup of bs threads after its staged tables, as
// qba_queue_base and the kernels' wq.base lay them out: the histogram, the
// ring alignment's slack, one ring [ND][QBA_QCAP] per wave.
template <int NP>
__host__ __device__ constexpr size_t qba_count_lds(int bs) {
  static_assert(QCfg<NP>::NBP % 4 == 0, "the histogram is whole 16-B words");
  return (size_t)QCfg<NP>::NBP * 4 + QBA_QCAP * 4 + (size_t)(bs / 64) * CF<NP>::ND * QBA_QCAP * 4;
}

// Count the nv (<= 64) oldest queued entries, one per lane.  TRUSTED: the
// values were produced by this kernel's sampler, masked to nq bits, so
// Cond2's range test cannot fail and is skipped (check-only launches keep it).
template <int NP, bool TRUSTED>
__device__ __forceinline__ void qba_q_drain(QbaWaveQ &q, uint32_t *hist, uint32_t nv) {
  constexpr int ND = CF<NP>::ND;
  const uint32_t lane = __lane_id();
  const uint32_t a = qba_q_addr(q, q.tail + lane);
  uint32_t D[ND];
  // a draining wave issues at raised priority: its queue reads, atomics and
  // address VALU go ahead of the sampling waves', so the LDS queue it feeds
  // drains sooner (745 k -> 727-729 k cycles per launch, window -2.5 %,
  // profiles/r3/r3k/drain_priority_ab.txt)
  __builtin_amdgcn_s_setprio(2);
#pragma unroll
  for (int i = 0; i < ND; ++i) D[i] = *qba_lds(a + i * QBA_QCAP * 4);
  if (nv >= 64 || lane < nv) qba_count_d<NP>(D, 0x00010001u, hist, TRUSTED, true, q.hoff);
  __builtin_amdgcn_s_setprio(0);
  q.tail += nv;
  q.qn -= nv;
}

// Append the lanes' entries with isq set (in lane order) and count a full
// batch of 64 as soon as one is queued.  Slot = tail + qn + the number of
// queued lanes below this one (mbcnt adds the base for free).
template <int NP, bool TRUSTED>
__device__ __forceinline__ void qba_q_push(QbaWaveQ &q, const uint32_t (&D)[CF<NP>::ND], bool isq,
                                           uint32_t *hist) {
  constexpr int ND = CF<NP>::ND;
  const uint64_t m = __ballot(isq);
  // mbcnt from 0 and the wave-uniform base added with the slot-to-byte shift
  // (one v_add_lshl_u32): no v_mov of the base into a VGPR per push
  const uint32_t mb = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (isq) {
    const uint32_t a = (((mb + q.tail + q.qn) << 2) & (uint32_t)(QBA_QCAP * 4 - 1)) | q.base;
#pragma unroll
    for (int i = 0; i < ND; ++i) *qba_lds(a + i * QBA_QCAP * 4) = D[i];
  }
  q.qn += (uint32_t)__popcll(m);
  if (q.qn >= 64) qba_q_drain<NP, TRUSTED>(q, hist, 64u);
}

// ---------------------------------------------------------------------------
// Pair-bin counting (CNT = 1: the fused n = 11 kernel, qba_k_lists MODE 1).
// The classic histogram takes one ds_add_u32 per counted group per Q entry
// (11 at n = 11, ~3.5-way bank conflicts each).  Here one atomic counts TWO
// groups: the bin of a pair (g, h) is (u, L_g, L_h), u = L1, held as an 8-bit
// lane of a dword:
//   array A [x_h][u][x_g] dwords (16 KB): lane 0 = pair (2,3), 1 = (4,5),
//                                         2 = (6,7), 3 = (8,9);
//   array B, same indexing (16 KB):       lane 0 = pair (10,11); lanes 1-3
//     (a 24-bit counter, added as 1 << 8) hold group 0 at x_h = u, and the
//     equal-pair bins C[u][k] at x_g = k & 15, x_h = u ^ (1 + (k >> 4)).
// The byte address of bin (u, x_g, x_h) is 4 x_g + 64 u + 1024 x_h: with
// E = values << 2 (byte g = 4 L_g) a 16-bit half of E IS 4 x_g + 1024 x_h
// for the groups of that half, so each address is ONE v_add_u32 with an SDWA
// word select onto the entry's row base A + 64 u -- as cheap as the classic
// per-group address -- and 6 atomics count the 11 groups.  The queue holds an
// entry as 8 B (c0 = groups 0-3 | groups 4-7 << 4, c1 = groups 8-11): one
// ds_write_b64 per push and one ds_read_b64 per drain instead of 3 + 3.
//
// An 8-bit lane can wrap.  Every Q entry adds exactly one count to every lane
// and to group 0, so per workgroup each lane's total equals group 0's total
// (24 bits, exact: a launch gives a workgroup < 2^24 entries) unless a lane
// wrapped: a wrap loses 256 from its lane and carries at most 1 into the next
// lane up, so some lane's total then differs from group 0's (the lowest
// wrapped lane is short by 255 or 256 net, and a lane can only gain what the
// lane below it lost; B's lane 0 carries into group 0's counter, raising its
// total, never the lane's).  The flush compares the totals and a workgroup
// that finds a mismatch recounts its own entries from the rows it stored,
// with the classic 32-bit bins (qba_lists_body) -- exact in every case.
// The launcher keeps a workgroup at <= QBA_PB_BUDGET entries per launch, so
// for sampled lists a wrap needs a bin ~18 sigma above its mean and never
// happens in practice (tests force it through qba_test_set_knobs' list_grid).
// ---------------------------------------------------------------------------
#define QBA_PB_BUDGET (1u << 18)  // entries per workgroup per launch (wrap-free in practice)
#define QBA_PB_FORCED_LOG2 23     // entries per workgroup (log2) under the tests' list_grid knob
// group 0's total sits in 24-bit lanes: every workgroup must count < 2^24 entries
static_assert(QBA_PB_BUDGET < (1u << 24) && QBA_PB_FORCED_LOG2 < 24, "pair-bin group-0 total is 24 bits");
struct QbaPB {
  static constexpr int WORDS = 8192;       // A [4096] then B [4096]
  static constexpr int BOFF = 4096;        // B, in words
  static constexpr int MISC = 8;           // after B: lane totals [0..4], group 0 total [5]
  static constexpr int AREA = WORDS + MISC;
  static constexpr int QSLOT = 8;          // queue bytes per entry
};
// LDS bytes of a pair-bin workgroup of bs threads after its staged tables, as
// qba_lists_body (CNT) lays them out: up to 1 KiB to align array A, the bins,
// the ring alignment's slack (one ring), one ring [QBA_QCAP] of 8-B slots per wave.
__host__ __device__ constexpr size_t qba_pb_lds(int bs) {
  static_assert(QbaPB::QSLOT == 8, "qba_lists_body places the rings QBA_QCAP * 8 bytes apart");
  return 1024 + (size_t)QbaPB::AREA * 4 + (size_t)(bs / 64 + 1) * QBA_QCAP * QbaPB::QSLOT;
}
// the kernels that count with pair bins: the fused closed-form n = 11 kernel
// and the n = 11 check of nibble rows (every value < 16 = w, so no range test)
template <int NP, int MODE, int SAMP, int PK>
struct QbaUsePB {
  static constexpr bool value =
      NP == 11 && ((MODE == 1 && SAMP == QBA_S_CLOSED) || (MODE == 2 && PK == 1));
};

// base + 16-bit half h of x in one VALU op (v_add_u32 with an SDWA word select)
__device__ __forceinline__ uint32_t qba_add_word(uint32_t base, uint32_t x, int h) {
  uint32_t r;
  if (h == 0)
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(r) : "v"(base), "v"(x));
  else
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(r) : "v"(base), "v"(x));
  return r;
}

__device__ __forceinline__ void qba_lds_add(uint32_t addr, uint32_t v) {
  atomicAdd((uint32_t *)qba_lds(addr), v);
}

// Count one Q-correlated entry (c0, c1) into the pair bins; hA = LDS byte
// address of array A.  Values are the sampler's (< 16), so no range test.
template <int NP>
__device__ __forceinline__ void qba_count_pb(uint32_t c0, uint32_t c1, uint32_t hA) {
  static_assert(NP == 11, "pair bins are laid out for n = 11");
  constexpr uint32_t B = QbaPB::BOFF * 4;
  const uint32_t E0 = (c0 << 2) & 0x3c3c3c3cu;  // groups 0-3, x4
  const uint32_t t = c0 >> 2;
  const uint32_t E1 = t & 0x3c3c3c3cu;          // groups 4-7, x4
  const uint32_t E2 = c1 << 2;                  // groups 8-11, x4
  // A + 64 u: u = group 1 sits at bits 6-9 of c0 >> 2, and A is 1-KiB
  // aligned (qba_lists_body), so the base is one v_and_or
  const uint32_t hb = (t & 0x3c0u) | hA;
  qba_lds_add(qba_add_word(hb, E0, 0) + B, 0x100u);      // group 0 at (x_0, u, u), B lanes 1-3
  qba_lds_add(qba_add_word(hb, E0, 1), 0x1u);            // (2,3)   A lane 0
  qba_lds_add(qba_add_word(hb, E1, 0), 0x100u);          // (4,5)   A lane 1
  qba_lds_add(qba_add_word(hb, E1, 1), 0x10000u);        // (6,7)   A lane 2
  qba_lds_add(qba_add_word(hb, E2, 0), 0x1000000u);      // (8,9)   A lane 3
  qba_lds_add(qba_add_word(hb, E2, 1) + B, 0x1u);        // (10,11) B lane 0
  // Cond3 (tfg.py:96-98) on every counted entry: its 12 values are pairwise
  // distinct iff the union of their 16-bit one-hots has 12 bits.  Each
  // v_pk_lshlrev_b16 makes two one-hots from the low nibbles of the two
  // halves of its amount: c0 -> groups 0, 2; c0 >> 4 -> 4, 6; c0 >> 8 -> 1,
  // 3; c0 >> 12 -> 5, 7; c1 -> 8, 10; c1 >> 8 -> 9, 11.
  const uint32_t one = 0x00010001u;
  const uint32_t s4 = c0 >> 4;
  // the union as two all-VGPR v_bitop3_b32 (a | b | c) and one v_or_b32, the
  // forms gfx950 issues at the full rate, instead of v_or + two v_or3_b32
  // (tools/exp/valu_mix2.hip; the same cycles per launch, the driver's window
  // -3 % in the 300-launch traces of profiles/r6/ab_cond3_bitop3)
  uint32_t U = __builtin_amdgcn_bitop3_b32(qba_pk_onehot(c0, one), qba_pk_onehot(s4, one),
                                           qba_pk_onehot(c0 >> 8, one), 0xFE);
  U = __builtin_amdgcn_bitop3_b32(U, qba_pk_onehot(s4 >> 8, one), qba_pk_onehot(c1, one), 0xFE);
  U |= qba_pk_onehot(c1 >> 8, one);
  if (__popc(qba_fold16(U)) != QCfg<NP>::G) {  // some pair collides: exact slow path
    // C[u][k] for every equal pair k = pidx(g, h): B lanes 1-3 of the word
    // (x_g = k & 15, u, x_h = u ^ (1 + k / 16)), a word no Q entry's group 0
    // uses (x_h != u; qba_pb_flush reads them back)
    const uint32_t w0 = c0 & 0x0f0f0f0fu, w1 = s4 & 0x0f0f0f0fu, w2 = c1;
    const uint32_t u = __builtin_amdgcn_ubfe(c0, 8, 4);
    int k = 0;
#pragma nounroll
    for (int g = 0; g < QCfg<NP>::G; ++g) {
      const uint32_t lg = qba_byte_of(g, w0, w1, w2, 0u);
#pragma nounroll
      for (int h = g + 1; h < QCfg<NP>::G; ++h, ++k)
        if (lg == qba_byte_of(h, w0, w1, w2, 0u))
          qba_lds_add(hA + B + 4 * (uint32_t)((k & 15) + 16 * u + 256 * (u ^ (1 + (k >> 4)))), 0x100u);
    }
  }
}

// the queue's 8-B form of an entry in the byte layout (values < 16)
template <int NP>
__device__ __forceinline__ uint2 qba_pb_pack(const uint32_t (&D)[CF<NP>::ND]) {
  return make_uint2(D[0] | (D[1] << 4), D[2]);
}

// The pair-bin queue is LINEAR: slots [0, qn) of the wave's 128-slot area
// hold the queued entries.  A push writes slot qn + (queued lanes below this
// one): ONE v_add_lshl_u32 (the wave's base / 8 rides in the SGPR sum); a
// drain counts slots [0, nv), one per lane at a loop-invariant address, then
// moves the leftover (< 64 entries) down to slot 0 with one read (offset
// 512) and one write per leftover lane.
template <int NP>
__device__ __forceinline__ void qba_q_drain_pb(QbaWaveQ &q, uint32_t nv) {
  const uint32_t lane = __lane_id();
  typedef uint32_t v2u __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(3))) v2u lds_v2u;
  uint32_t a;  // base + 8 lane in one op
  asm("v_lshl_add_u32 %0, %1, 3, %2" : "=v"(a) : "v"(lane), "s"(q.base));
  const v2u c = *reinterpret_cast<lds_v2u *>(static_cast<uintptr_t>(a));
  __builtin_amdgcn_s_setprio(2);  // as qba_q_drain
  if (nv >= 64 || lane < nv) qba_count_pb<NP>(c.x, c.y, q.hoff);
  __builtin_amdgcn_s_setprio(0);
  q.qn -= nv;
  if (q.qn) {  // wave-uniform: the leftover of a full drain (nv = 64)
    if (lane < q.qn) {
      const v2u m = *reinterpret_cast<lds_v2u *>(static_cast<uintptr_t>(a + 512u));
      *reinterpret_cast<lds_v2u *>(static_cast<uintptr_t>(a)) = m;
    }
  }
}

// The lanes whose entry is Q-correlated (L0 != L1, tfg.py:327: byte 0 vs byte
// 1 of word 0 of the byte layout) among the active lanes `act`: one SDWA
// v_cmp, then an s_and -- the last writer of the mask is the scalar unit.
__device__ __forceinline__ uint64_t qba_isq_mask(uint32_t w0, uint64_t act) {
  uint64_t m;
  asm("v_cmp_ne_u32_sdwa %0, %1, %1 src0_sel:BYTE_0 src1_sel:BYTE_1\n\ts_and_b64 %0, %0, %2"
      : "=&s"(m) : "v"(w0), "s"(act));
  return m;
}

// Push the entries of the lanes in m (a lane mask, qba_isq_mask)
template <int NP>
__device__ __forceinline__ void qba_q_push_pb_m(QbaWaveQ &q, const uint32_t (&D)[CF<NP>::ND], uint64_t m) {
  const uint32_t mb = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (__builtin_amdgcn_inverse_ballot_w64(m)) {
    uint32_t a;  // (mb + qn + base / 8) * 8 in one op
    asm("v_add_lshl_u32 %0, %1, %2, 3" : "=v"(a) : "v"(mb), "s"(q.qn + (q.base >> 3)));
    const uint2 c = qba_pb_pack<NP>(D);
    typedef uint32_t v2u __attribute__((ext_vector_type(2)));
    v2u cv;
    cv.x = c.x;
    cv.y = c.y;
    *reinterpret_cast<__attribute__((address_space(3))) v2u *>(static_cast<uintptr_t>(a)) = cv;
  }
  q.qn += (uint32_t)__popcll(m);
  if (q.qn >= 64) qba_q_drain_pb<NP>(q, 64u);
}

template <int NP>
__device__ __forceinline__ void qba_q_push_pb(QbaWaveQ &q, const uint32_t (&D)[CF<NP>::ND], bool isq) {
  const uint64_t m = __ballot(isq);
  const uint32_t mb = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (isq) {
    uint32_t a;  // (mb + qn + base / 8) * 8 in one op (the compiler splits it into three)
    asm("v_add_lshl_u32 %0, %1, %2, 3" : "=v"(a) : "v"(mb), "s"(q.qn + (q.base >> 3)));
    const uint2 c = qba_pb_pack<NP>(D);
    typedef uint32_t v2u __attribute__((ext_vector_type(2)));
    v2u cv;
    cv.x = c.x;
    cv.y = c.y;
    *reinterpret_cast<__attribute__((address_space(3))) v2u *>(static_cast<uintptr_t>(a)) = cv;
  }
  q.qn += (uint32_t)__popcll(m);
  if (q.qn >= 64) qba_q_drain_pb<NP>(q, 64u);
}

// Push (the wave queue) / count one entry directly (tails) with the counting
// scheme CNT (0: classic 32-bit bins in `hist`, 1: pair bins, hist = array A).
template <int NP, bool TRUSTED, int CNT>
__device__ __forceinline__ void qba_push(QbaWaveQ &q, const uint32_t (&D)[CF<NP>::ND], bool isq, uint32_t *hist) {
  if constexpr (CNT == 1)
    qba_q_push_pb<NP>(q, D, isq);
  else
    qba_q_push<NP, TRUSTED>(q, D, isq, hist);
}
template <int NP, int CNT>
__device__ __forceinline__ void qba_count_one(const uint32_t (&D)[CF<NP>::ND], uint32_t *hist) {
  if constexpr (CNT == 1) {
    if ((D[0] & 0xffu) == ((D[0] >> 8) & 0xffu)) return;  // not Q-correlated (tfg.py:327)
    const uint2 c = qba_pb_pack<NP>(D);
    qba_count_pb<NP>(c.x, c.y, (uint32_t)(uintptr_t)(qba_lds_u32 *)hist);
  } else {
    qba_count_d<NP>(D, 0x00010001u, hist, true);
  }
}

// The pair bins' flush: the classic slab row (H [u][g][x] as counted, the
// pair bins C[u][k], the stats) from the marginals of arrays A / B, after the
// wrap test (see QbaPB).  Returns true -- for every thread -- when a lane
// wrapped; the slab row is then left to the caller's recount.  Slab words of
// group 1 and the row padding are not written (the reductions skip them).
template <int NP, int BS>
__device__ __forceinline__ bool qba_pb_flush(uint32_t *hist, uint32_t *row, int t) {
  using C = QCfg<NP>;
  static_assert(BS >= 512, "four roles of 256 threads");
  const uint32_t *A = hist, *Bw = hist + QbaPB::BOFF;
  uint32_t *misc = hist + QbaPB::WORDS;
  uint32_t v[5] = {0u, 0u, 0u, 0u, 0u}, g0 = 0u;
  const int ug = (t & 255) >> 4, xg = t & 15;    // column-sum threads: (u, x)
  const int ur = t & 15, yr = (t & 255) >> 4;    // row-sum threads: (u, y), u fastest
  if (t < 256) {  // groups 2, 4, 6, 8, 10 (x_g of each pair): sums over x_h
    uint32_t s02 = 0u, s13 = 0u, sb = 0u;
    const uint32_t *a = A + xg + 16 * ug, *b = Bw + xg + 16 * ug;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t d = a[256 * k];
      s02 += d & 0x00ff00ffu;
      s13 += (d >> 8) & 0x00ff00ffu;
      sb += b[256 * k] & 0xffu;
    }
    v[0] = s02 & 0xffffu;  // (2,3)
    v[1] = s13 & 0xffffu;  // (4,5)
    v[2] = s02 >> 16;      // (6,7)
    v[3] = s13 >> 16;      // (8,9)
    v[4] = sb;             // (10,11)
    g0 = Bw[xg + 16 * ug + 256 * ug] >> 8;
    // lane totals: summed across the wave first (64 same-address LDS atomics
    // per instruction serialise: +12 us per launch), then one atomic per wave
    uint32_t s6[6] = {v[0], v[1], v[2], v[3], v[4], g0};
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
      for (int p = 0; p < 6; ++p) s6[p] += __shfl_xor(s6[p], m, 64);
    if ((t & 63) == 0)
#pragma unroll
      for (int p = 0; p < 6; ++p) atomicAdd(&misc[p], s6[p]);
  } else if (t < 512) {  // groups 3, 5, 7, 9, 11 (x_h of each pair): sums over x_g
    uint32_t s02 = 0u, s13 = 0u, sb = 0u;
    const uint4 *a = reinterpret_cast<const uint4 *>(A + 16 * ur + 256 * yr);
    const uint4 *b = reinterpret_cast<const uint4 *>(Bw + 16 * ur + 256 * yr);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4 d = a[(k + ur) & 3], e = b[(k + ur) & 3];  // rotated: fewer bank conflicts
      s02 += (d.x & 0x00ff00ffu) + (d.y & 0x00ff00ffu) + (d.z & 0x00ff00ffu) + (d.w & 0x00ff00ffu);
      s13 += ((d.x >> 8) & 0x00ff00ffu) + ((d.y >> 8) & 0x00ff00ffu) + ((d.z >> 8) & 0x00ff00ffu) +
             ((d.w >> 8) & 0x00ff00ffu);
      sb += (e.x & 0xffu) + (e.y & 0xffu) + (e.z & 0xffu) + (e.w & 0xffu);
    }
    v[0] = s02 & 0xffffu;
    v[1] = s13 & 0xffffu;
    v[2] = s02 >> 16;
    v[3] = s13 >> 16;
    v[4] = sb;
  }
  __syncthreads();
  const bool wrap = misc[0] != misc[5] || misc[1] != misc[5] || misc[2] != misc[5] || misc[3] != misc[5] ||
                    misc[4] != misc[5];
  if (wrap) return true;  // workgroup-uniform
  if (t < 256) {
    row[(ug * C::G + 0) * C::WP + xg] = g0;
#pragma unroll
    for (int p = 0; p < 5; ++p) row[(ug * C::G + 2 + 2 * p) * C::WP + xg] = v[p];
  } else if (t < 512) {
#pragma unroll
    for (int p = 0; p < 5; ++p) row[(ur * C::G + 3 + 2 * p) * C::WP + yr] = v[p];
  }
  for (int i = t; i < C::CBL; i += BS) {  // C[u][k]: B lanes 1-3 at (k & 15, u, u ^ (1 + k / 16))
    const int u = i / C::CP, k = i - u * C::CP;
    row[C::HBL + i] = Bw[(k & 15) + 16 * u + 256 * (u ^ (1 + (k >> 4)))] >> 8;
  }
  if (t < C::STATS) row[C::HBL + C::CBL + t] = 0u;  // sampled values are < w
  return false;
}
