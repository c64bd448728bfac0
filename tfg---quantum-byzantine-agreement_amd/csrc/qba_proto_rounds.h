// qba_proto_rounds.h -- the count-mode protocol rounds of ONE instance on one
// wavefront, as device code shared by the kernels that decide instances:
//   qba_k_protocol (qba_proto.hip)     distils the int64 count tables
//   qba_k_mc_lists (qba_proto.hip)     distils injected byte rows
//   qba_k_mc_sampled (qba_mc_kern.h)   distils the entries it samples itself
//   qba_k_mc_curve_sampled / _lists    the same two at several counts in one pass
// Each brings the distilled state -- pnz (bit u: P_u is not empty) and, in
// ProtoShared, per (u, g) the mask of x with H[u][g][x] != 0, the mask of h
// with C[u][g][h] == 0 and rep(u, g) = min h with C[u][g][h] == |P_u| -- and
// proto_rounds does the rest: the dishonest draw, the commander, epoch 0,
// rounds 1 .. n_dis + 1, the decisions and the row stores (tfg.py:101-125,
// 166-196, 266-306, 337-363).
//
// Lane r is rank r (0 = QSD, 1 = commander, >= 2 = lieutenants).
//   packet    32 bits: v [0:4), P's u [4:8), P cleared [8], the descriptors'
//             u [9:13), EMPTY descriptor present [13], mask of reps [16:32)
//   rounds    within an epoch the lieutenants are independent (a message is
//             delivered at the next barrier); lane `dest` walks its inbox
//             box[epoch - 1][dest][src][slot] in (src, slot) order = LocalWorld's
//             (source, sequence) order, and lane `src` appends its sends to
//             box[epoch][dest][src][..]: no atomics.  A sender re-broadcasts only
//             a v newly added to its V_i, so at most w packets per (dest, src)
//             and round: w slots, bounds-checked.
// Every loop has a static bound; hitting the RNG word cap or a full mailbox
// sets a status bit and the instance's other outputs are written as zero.
// All results are written with ordinary (vector) stores.
#pragma once
#include "qba_internal.h"

#define QBA_PROTO_BLOCK 64
#define QBA_PROTO_MAXG 16       // ranks 0..15

#define QBA_PKT_CLEARED (1u << 8)
#define QBA_PKT_EMPTY (1u << 13)

namespace {

// The protocol stream of one rank (layout in qba_internal.h).
struct ProtoRng {
  uint32_t k0, k1, rank, t, blk, status;
  QbaU4 b;

  __device__ __forceinline__ uint32_t next() {
    const uint32_t want = t >> 2;
    if (want != blk) {
      b = qba_philox(want, rank, 0u, QBA_PROTO_CTR_TAG, k0, k1);
      blk = want;
    }
    const uint32_t j = t & 3u;
    ++t;
    return j == 0 ? b.x : j == 1 ? b.y : j == 2 ? b.z : b.w;
  }

  // Lemire: m = x * k, accept m >> 32 when (uint32)m >= 2^32 mod k
  __device__ __forceinline__ uint32_t randint(uint32_t k) {
    const uint32_t thr = (0u - k) % k;
    uint32_t r = 0;
    for (int i = 0; i < QBA_PROTO_RNG_CAP; ++i) {
      const uint64_t m = (uint64_t)next() * k;
      r = (uint32_t)(m >> 32);
      if ((uint32_t)m >= thr) return r;
    }
    status |= QBA_PROTO_ST_RNG;
    return r;
  }
};

struct ProtoShared {
  int64_t p64[16];                                   // P[u] (qba_k_protocol's prologue)
  uint32_t tab[16 * QBA_PROTO_MAXG];                 // [u][g]: H mask | C-zero mask << 16
  uint8_t rep[16 * QBA_PROTO_MAXG];                  // [u][g]: rep(u, g)
  uint8_t cnt[2 * QBA_PROTO_MAXG * QBA_PROTO_MAXG];  // [buf][dest][src] packets in box
  int32_t dec[QBA_PROTO_MAXG];                       // decisions
  uint32_t cv[QBA_PROTO_MAXG];                       // commander's v per destination
  uint32_t dis_mask;
};

// Mailbox words of one instance: [2][G][box_ld], box_ld = G * w + 1 (+ 1: the
// lanes' inbox rows start on different banks); <= 8224 words at n = 15
__host__ __device__ constexpr int proto_box_words(int G, int w) { return 2 * G * (G * w + 1); }

// ProtoShared in front of the mailbox when both sit in dynamic LDS (16-B words)
constexpr int PROTO_S_WORDS = (int)((sizeof(ProtoShared) + 15) / 16 * 4);

// The barrier between the phases of an instance.  WG: the workgroup's (the
// one-wavefront workgroups of qba_k_protocol, where it costs no s_barrier).
// Otherwise the wavefront's own: its LDS operations execute in program order,
// so ordering the compiler (the fences) is all a phase boundary needs, and the
// waves of a workgroup stay independent of each other -- each may own another
// number of instances.
template <bool WG>
__device__ __forceinline__ void proto_sync() {
  if constexpr (WG) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// L.add(own descriptor), consistent(v, L), len(L)  (countmode.CountTables)
__device__ __forceinline__ bool proto_check(const ProtoShared &S, uint32_t &pkt, int g, int G, uint32_t pnz,
                                            int &len) {
  const uint32_t v = pkt & 15u, pu = (pkt >> 4) & 15u;
  if ((pkt & QBA_PKT_CLEARED) || !((pnz >> pu) & 1u)) {
    pkt |= QBA_PKT_EMPTY;
  } else {
    pkt = (pkt & ~(15u << 9)) | (pu << 9) | (1u << (16 + S.rep[pu * QBA_PROTO_MAXG + g]));
  }
  const uint32_t mask = pkt >> 16, du = (pkt >> 9) & 15u;
  const bool empty = (pkt & QBA_PKT_EMPTY) != 0;
  len = __popc(mask) + (empty ? 1 : 0);
  if (empty && mask) return false;  // Cond1: lengths 0 and |P_u| > 0
  bool ok = true;
  for (int a = 0; a < G; ++a) {
    if (!((mask >> a) & 1u)) continue;
    const uint32_t t = S.tab[du * QBA_PROTO_MAXG + a];
    if ((t >> v) & 1u) ok = false;                           // Cond2: v occurs in the tuple
    if ((mask & ~(1u << a)) & ~(t >> 16) & 0xFFFFu) ok = false;  // Cond3: a shared position
  }
  return ok;
}

// lieu_broadcast (tfg.py:266-286): the dishonest mutations stay for later dest
__device__ __forceinline__ void proto_broadcast(ProtoShared &S, uint32_t *box, int box_ld, int w, int n, int me,
                                                bool dishonest, uint32_t pkt, int buf, ProtoRng &rng,
                                                int &sent) {
  for (int dest = 2; dest <= n; ++dest) {
    if (dest == me) continue;
    uint32_t go = 1;
    if (dishonest) {
      const uint32_t action = rng.randint(4);
      if (action == 0) go = rng.randint(2);
      else if (action == 1) pkt = (pkt & ~15u) | rng.randint((uint32_t)n + 1u);
      else if (action == 2) pkt |= QBA_PKT_CLEARED;
      else pkt &= ~(QBA_PKT_EMPTY | 0xFFFF0000u);
    }
    if (!go) continue;
    ++sent;
    const int ci = (buf * QBA_PROTO_MAXG + dest) * QBA_PROTO_MAXG + me;
    const int k = S.cnt[ci];
    if (k < w) {
      box[(buf * (n + 1) + dest) * box_ld + me * w + k] = pkt;
      S.cnt[ci] = (uint8_t)(k + 1);
    } else {
      rng.status |= QBA_PROTO_ST_MAILBOX;
    }
  }
}

// Everything after the distillation, for the instance keyed `key`; `o` is its
// result row (4 + 5 * (n + 1) words, layout in qba.h).  S.tab, S.rep and pnz
// hold the distilled state (made visible by the caller's proto_sync); box is
// the instance's mailbox, proto_box_words(n + 1, w) words.  st0: status bits
// the caller found while distilling (QBA_PROTO_ST_RANGE), wave-uniform.
template <bool WG>
__device__ __forceinline__ void proto_rounds(ProtoShared &S, uint32_t *box, int n, int n_dis, uint64_t key,
                                             uint32_t pnz, uint32_t st0, int lane, int32_t *__restrict__ o) {
  const int G = n + 1, nq = 32 - __clz(n), w = 1 << nq;  // nq = ceil(log2(n + 1)), tfg.py:317
  const int box_ld = G * w + 1;
  ProtoRng rng;
  rng.k0 = (uint32_t)key;
  rng.k1 = (uint32_t)(key >> 32);
  rng.rank = (uint32_t)lane;
  rng.t = 0;
  rng.blk = 0xFFFFFFFFu;
  rng.status = 0;
  rng.b = QbaU4{0, 0, 0, 0};

  // ---- tfg.py:101-125: rank 0 draws the dishonest ranks ------------------------
  if (lane == 0) {
    // choice(arange(1, n + 1), n_dis, replace=False): partial Fisher-Yates on
    // the nibbles of `a`
    uint64_t a = 0xFEDCBA987654321ull;
    uint32_t dm = 0;
    for (int j = 0; j < n_dis; ++j) {
      const int s = j + (int)rng.randint((uint32_t)(n - j));
      const uint64_t aj = (a >> (4 * j)) & 15u, as = (a >> (4 * s)) & 15u;
      a ^= ((aj ^ as) << (4 * j)) | ((aj ^ as) << (4 * s));
      dm |= 1u << as;
    }
    S.dis_mask = dm;
  }
  proto_sync<WG>();
  const uint32_t dis_mask = S.dis_mask;
  const bool dishonest = (dis_mask >> lane) & 1u;
  const bool lieutenant = lane >= 2 && lane <= n;

  int accept = 0, reject = 0, sent = 0, decision = 0;
  uint32_t Vi = 0;

  // ---- tfg.py:166-185, 329: the commander's order(s) ---------------------------
  if (lane == 1) {
    const uint32_t v = rng.randint((uint32_t)w);
    uint32_t v1 = v, v2 = v;
    if (dishonest) {
      v1 = rng.randint((uint32_t)w);
      v2 = rng.randint((uint32_t)w);
      int tries = 0;
      while (v2 == v1 && tries < QBA_PROTO_RNG_CAP) {
        v2 = rng.randint((uint32_t)w);
        ++tries;
      }
      if (v2 == v1) rng.status |= QBA_PROTO_ST_RNG;
    }
    for (int dest = 2; dest <= n; ++dest) {
      S.cv[dest] = dest <= (n + 1) / 2 ? v1 : v2;
      ++sent;
    }
    decision = (int)v;
  }
  proto_sync<WG>();

  // ---- tfg.py:186-196: epoch 0, the lieutenants take the commander's packet ----
  if (lieutenant) {
    for (int d = 0; d < G; ++d) S.cnt[d * QBA_PROTO_MAXG + lane] = 0;
    uint32_t pkt = S.cv[lane] | (S.cv[lane] << 4);
    int len;
    if (proto_check(S, pkt, lane, G, pnz, len)) {
      ++accept;
      Vi |= 1u << (pkt & 15u);
      proto_broadcast(S, box, box_ld, w, n, lane, dishonest, pkt, 0, rng, sent);
    } else {
      ++reject;
    }
  }
  proto_sync<WG>();

  // ---- tfg.py:337-350: rounds 1 .. n_dis + 1 -----------------------------------
  for (int rnd = 1; rnd <= n_dis + 1; ++rnd) {
    const int wb = rnd & 1, rb = wb ^ 1;
    if (lieutenant) {
      for (int d = 0; d < G; ++d) S.cnt[(wb * QBA_PROTO_MAXG + d) * QBA_PROTO_MAXG + lane] = 0;
      for (int src = 2; src <= n; ++src) {
        int c = S.cnt[(rb * QBA_PROTO_MAXG + lane) * QBA_PROTO_MAXG + src];
        c = c < w ? c : w;
        for (int k = 0; k < c; ++k) {
          uint32_t pkt = box[(rb * G + lane) * box_ld + src * w + k];
          const uint32_t v = pkt & 15u;
          int len;
          const bool ok = proto_check(S, pkt, lane, G, pnz, len);
          if (ok) ++accept; else ++reject;
          if (ok && !((Vi >> v) & 1u) && len == rnd + 1) {
            Vi |= 1u << v;
            if (rnd <= n_dis) proto_broadcast(S, box, box_ld, w, n, lane, dishonest, pkt, wb, rng, sent);
          }
        }
      }
    }
    proto_sync<WG>();
  }

  // ---- tfg.py:303-306, 352-363: decisions and success --------------------------
  if (lieutenant) decision = Vi ? __ffs((int)Vi) - 1 : -1;
  if (lane <= n) S.dec[lane] = decision;
  const uint32_t empty_mask = (uint32_t)__ballot(lieutenant && Vi == 0);
  const uint32_t status = st0 | (__ballot(rng.status & QBA_PROTO_ST_MAILBOX) ? QBA_PROTO_ST_MAILBOX : 0u) |
                          (__ballot(rng.status & QBA_PROTO_ST_RNG) ? QBA_PROTO_ST_RNG : 0u);
  proto_sync<WG>();
  if (lane == 0) {
    int first = 0, seen = 0, same = 1;
    for (int r = 1; r <= n; ++r) {
      if ((dis_mask >> r) & 1u) continue;
      if (!seen) first = S.dec[r];
      else if (S.dec[r] != first) same = 0;
      seen = 1;
    }
    o[0] = status ? 0 : (seen && same);
    o[1] = status ? 0 : (int32_t)dis_mask;
    o[2] = status ? 0 : (int32_t)empty_mask;
    o[3] = (int32_t)status;
  }
  if (lane <= n) {
    int32_t *r = o + 4 + 5 * lane;
    const bool z = status != 0 || lane == 0;
    r[0] = z ? 0 : decision;
    r[1] = z ? 0 : (int32_t)Vi;
    r[2] = z ? 0 : accept;
    r[3] = z ? 0 : reject;
    r[4] = z ? 0 : sent;
  }
}

// ---------------------------------------------------------------------------
// Distilling list entries straight into the masks (the fused Monte-Carlo
// kernels).  Everything the rounds consult is a bitwise reduction over the
// Q-correlated entries (L0 != L1) of P_u, u = L1; with E(g) = the entry's
// equal-pair mask {h : L_h == L_g}:
//   P[u] != 0                          an entry with this u exists
//   {x : H[u][g][x] != 0}              OR of 1 << L_g
//   {h : C[u][g][h] == 0}              complement of OR of E(g)
//   rep(u, g) = min h, C[u][g][h]==P[u]  lowest bit of AND of E(g)  (all ones
//                                      for an empty P_u: rep = 0, as the tables give)
// While an instance is distilled, S.tab[u][g] accumulates the two ORs (the
// E(g) half NOT yet complemented) by LDS atomics, and the wave's mailbox --
// idle until the rounds -- holds the AND words:
//   mcw[u * G + g]  AND of E(g) over the entries with a collision
//   mcw[w * G]      bit u: P_u has an entry of pairwise distinct values
//   mcw[w * G + 1]  != 0: a value >= w at a Q-correlated position
// An entry of pairwise distinct values has E(g) = {g}: one popcount of the
// union of its one-hots decides that, its AND is folded in once per u by
// mc_finish, and only a colliding entry walks its pairs (sampled Q entries
// never collide; injected lists may on every entry).
// ---------------------------------------------------------------------------
// value of group g (runtime g) of an entry's byte-layout words: selects, so
// that D stays in registers
__device__ __forceinline__ uint32_t qba_byte_at(const uint32_t (&D)[4], int g) {
  const int i = g >> 2;
  const uint32_t x = i == 0 ? D[0] : i == 1 ? D[1] : i == 2 ? D[2] : D[3];
  return (x >> (8 * (g & 3))) & 0xffu;
}

__device__ __forceinline__ void mc_begin(ProtoShared &S, uint32_t *mcw, int G, int w, int lane) {
  for (int i = lane; i < w * QBA_PROTO_MAXG; i += 64) S.tab[i] = 0u;
  for (int i = lane; i < w * G + 2; i += 64) mcw[i] = i < w * G ? 0xFFFFFFFFu : 0u;
}

// One entry, group g = byte g % 4 of D[g / 4] (the layout of qba_entry_d).
// RANGE: the values are untrusted; an entry with one >= w is flagged and left
// out (its u could index past the masks).  seen: this lane's distinct-entry bits.
// mc_entry_at (the curve kernels): the OR words are tab[u * tld + g], an
// accumulator area with rows G apart.  mc_entry below is the same body on
// S.tab; it is kept as its own text, because routing it through mc_entry_at
// changed the code the compiler emits for qba_k_mc_sampled at n >= 7, and the
// existing kernels stay byte for byte what they were.
template <bool RANGE>
__device__ __forceinline__ void mc_entry_at(uint32_t *tab, int tld, uint32_t *mcw, const uint32_t (&D)[4], int G,
                                            int w, uint32_t &seen, uint32_t &bad) {
  const uint32_t l0 = D[0] & 0xffu, u = (D[0] >> 8) & 0xffu;
  if (l0 == u) return;  // not Q-correlated (tfg.py:327)
  uint32_t U = 0, hi = 0;
  for (int g = 0; g < G; ++g) {
    const uint32_t v = qba_byte_at(D, g);
    hi |= v;
    U |= 1u << (v & 15u);
  }
  if (RANGE && hi >= (uint32_t)w) {
    bad = 1u;
    return;
  }
  uint32_t *t = &tab[u * tld];
  if (__popc(U) == G) {  // pairwise distinct: E(g) = {g}
    for (int g = 0; g < G; ++g) atomicOr(&t[g], (1u << qba_byte_at(D, g)) | (0x10000u << g));
    seen |= 1u << u;
    return;
  }
  for (int g = 0; g < G; ++g) {
    const uint32_t v = qba_byte_at(D, g);
    uint32_t eq = 0;
    for (int h = 0; h < G; ++h) eq |= (uint32_t)(qba_byte_at(D, h) == v) << h;
    atomicOr(&t[g], (1u << v) | (eq << 16));
    atomicAnd(&mcw[u * G + g], eq);
  }
}

template <bool RANGE>
__device__ __forceinline__ void mc_entry(ProtoShared &S, uint32_t *mcw, const uint32_t (&D)[4], int G, int w,
                                         uint32_t &seen, uint32_t &bad) {
  const uint32_t l0 = D[0] & 0xffu, u = (D[0] >> 8) & 0xffu;
  if (l0 == u) return;  // not Q-correlated (tfg.py:327)
  uint32_t U = 0, hi = 0;
  for (int g = 0; g < G; ++g) {
    const uint32_t v = qba_byte_at(D, g);
    hi |= v;
    U |= 1u << (v & 15u);
  }
  if (RANGE && hi >= (uint32_t)w) {
    bad = 1u;
    return;
  }
  uint32_t *t = &S.tab[u * QBA_PROTO_MAXG];
  if (__popc(U) == G) {  // pairwise distinct: E(g) = {g}
    for (int g = 0; g < G; ++g) atomicOr(&t[g], (1u << qba_byte_at(D, g)) | (0x10000u << g));
    seen |= 1u << u;
    return;
  }
  for (int g = 0; g < G; ++g) {
    const uint32_t v = qba_byte_at(D, g);
    uint32_t eq = 0;
    for (int h = 0; h < G; ++h) eq |= (uint32_t)(qba_byte_at(D, h) == v) << h;
    atomicOr(&t[g], (1u << v) | (eq << 16));
    atomicAnd(&mcw[u * G + g], eq);
  }
}

// The lanes' flags into the wave's words (one LDS atomic per lane that has any).
__device__ __forceinline__ void mc_flags(uint32_t *mcw, int G, int w, uint32_t seen, uint32_t bad) {
  if (seen) atomicOr(&mcw[w * G], seen);
  if (bad) atomicOr(&mcw[w * G + 1], bad);
}

// After a proto_sync: the masks into the tab / rep form of the tables'
// prologue.  Returns pnz; st gets QBA_PROTO_ST_RANGE when an entry was flagged.
// The caller syncs once more before the rounds (which then reuse mcw's words
// as the mailbox: every lane has read what it needs of them by then).
template <bool WG>
__device__ __forceinline__ uint32_t mc_finish(ProtoShared &S, uint32_t *mcw, int G, int w, int lane,
                                              uint32_t &st) {
  const uint32_t seen = mcw[w * G];
  st = mcw[w * G + 1] ? QBA_PROTO_ST_RANGE : 0u;
  for (int e = lane; e < w * G; e += 64) {
    const int u = e / G, g = e - u * G, at = u * QBA_PROTO_MAXG + g;
    uint32_t a = mcw[e];
    if ((seen >> u) & 1u) a &= 1u << g;
    const uint32_t t = S.tab[at];
    S.tab[at] = (t & 0xFFFFu) | ((~(t >> 16) & ((1u << G) - 1u)) << 16);
    S.rep[at] = (uint8_t)(__ffs((int)a) - 1);  // a keeps bit g at least: g is in every E(g)
  }
  proto_sync<WG>();
  uint32_t pnz = 0;
  for (int u = 0; u < w; ++u) pnz |= (uint32_t)((S.tab[u * QBA_PROTO_MAXG] & 0xFFFFu) != 0u) << u;
  return pnz;
}

// ---------------------------------------------------------------------------
// The curve kernels decide one instance at several counts c_0 < c_1 < ...: the
// masks at count c are the reductions over the entries [0, c), so they keep
// RUNNING masks over the segments [c_(j-1), c_j) and run the rounds at every
// c_j.  mc_finish complements S.tab in place and the rounds write the mailbox,
// so the running masks live in an accumulator area of the wave's own, outside
// ProtoShared and the mailbox, that only the segments write:
//   acc[u * G + g]          the two ORs, as S.tab[u][g] holds them while an
//                           instance is distilled (mc_entry_at, rows G apart)
//   acc[w * G + ...]        the AND words and the two flag words, laid out as
//                           mc_entry / mc_flags lay them out in the mailbox
// mc_acc_finish is mc_finish reading the area and writing S.tab / S.rep: the
// area stays as it was, and the next segment goes on from it.
// ---------------------------------------------------------------------------
__host__ __device__ constexpr int mc_acc_words(int G, int w) { return 2 * w * G + 2; }

__device__ __forceinline__ void mc_acc_begin(uint32_t *acc, int G, int w, int lane) {
  for (int i = lane; i < 2 * w * G + 2; i += 64) acc[i] = i >= w * G && i < 2 * w * G ? 0xFFFFFFFFu : 0u;
}

template <bool WG>
__device__ __forceinline__ uint32_t mc_acc_finish(ProtoShared &S, const uint32_t *acc, int G, int w, int lane,
                                                  uint32_t &st) {
  const uint32_t *mcw = acc + w * G;
  const uint32_t seen = mcw[w * G];
  st = mcw[w * G + 1] ? QBA_PROTO_ST_RANGE : 0u;
  for (int e = lane; e < w * G; e += 64) {
    const int u = e / G, g = e - u * G, at = u * QBA_PROTO_MAXG + g;
    uint32_t a = mcw[e];
    if ((seen >> u) & 1u) a &= 1u << g;
    const uint32_t t = acc[e];
    S.tab[at] = (t & 0xFFFFu) | ((~(t >> 16) & ((1u << G) - 1u)) << 16);
    S.rep[at] = (uint8_t)(__ffs((int)a) - 1);
  }
  proto_sync<WG>();
  uint32_t pnz = 0;
  for (int u = 0; u < w; ++u) pnz |= (uint32_t)((S.tab[u * QBA_PROTO_MAXG] & 0xFFFFu) != 0u) << u;
  return pnz;
}

}  // namespace
