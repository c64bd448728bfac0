// qba_proto_adv.h -- the protocol rounds of qba_proto_rounds.h under an
// adversary policy: what a dishonest lieutenant does
// to a packet per destination, and how a dishonest commander splits the
// lieutenants, are read from a 32-bit policy word instead of being the
// reference's one rule (tfg.py:166-185, 266-286).
//
//   bits [0:5)  acts   the actions a dishonest lieutenant draws from: 0 maybe do
//                      not send, 1 replace the order, 2 clear P, 3 clear L
//                      (the reference's four), 4 relay unchanged
//   bits [8:10) order  what action 1 writes: 0 randint(n + 1) (the reference),
//                      1 the smallest order in [0, w) other than the packet's
//                      current v (no draw), 2 randint(w)
//   bit  12     fresh  0: a mutation stays for the later destinations of the
//                      broadcast (the reference); 1: every destination starts
//                      from the packet as it was handed to the broadcast
//   bit  16     comm   the dishonest commander's split: 0 dest <= (n + 1) / 2
//                      gets v1 (the reference), 1 even dest gets v1
// Every other bit is 0, acts is not 0 and order <= 2 (qba_adv_bad).  0xF is the
// reference policy, and with it proto_rounds_adv draws the words proto_rounds
// draws and writes its rows.
//
// The draw per destination: a = randint(popcount(acts)), always (Lemire with
// k = 1 accepts its first word); the action is the a-th set bit of acts in
// ascending order; action 0 then draws randint(2), action 1 as `order` says,
// the others nothing.  montecarlo.AdversaryParty is the host restatement.
//
// proto_broadcast_adv and proto_rounds_adv are texts of their own: the kernels
// that existed before them keep proto_broadcast / proto_rounds and their code.
// The policy is wave-uniform (a kernel argument) and takes no LDS; the
// mailbox bound is untouched (at most one send per destination and broadcast).
#pragma once
#include "qba_proto_rounds.h"

#define QBA_ADV_VALID 0x0001131Fu  // the bits a policy word may set

// What is wrong with a policy word (NULL: nothing), for qba_mc_check's envelope
inline const char *qba_adv_bad(uint32_t adv) {
  if (adv & ~QBA_ADV_VALID) return "adv sets a reserved bit";
  if (!(adv & 0x1Fu)) return "adv allows no action (acts == 0)";
  if (((adv >> 8) & 3u) > 2u) return "adv's order field must be <= 2";
  return nullptr;
}

// The launches of qba_proto_adv.hip's kernels (one wavefront per instance,
// instances [first, first + grid.x)), for the entry points in qba_proto.hip
void qba_launch_protocol_adv(dim3 grid, size_t lds, hipStream_t stream, int n, int n_dis, uint64_t seed_base,
                             int64_t first, const int64_t *H, const int64_t *C, const int64_t *P, int32_t *out,
                             uint32_t adv);
void qba_launch_mc_lists_adv(dim3 grid, size_t lds, hipStream_t stream, int n, int n_dis, uint64_t seed_base,
                             int64_t first, uint32_t count, const uint8_t *lists, uint64_t ld, uint64_t inst_stride,
                             int32_t *out, uint32_t adv);
void qba_launch_mc_curve_lists_adv(dim3 grid, size_t lds, hipStream_t stream, int n, int n_dis, uint64_t seed_base,
                                   int64_t first, int64_t n_inst, const uint8_t *lists, uint64_t ld,
                                   uint64_t inst_stride, int32_t *out, const QbaMcCounts &cv, uint32_t adv);
// ... and of qba_proto_sweep.hip's (the curve under every scenario of `sv`)
void qba_launch_mc_sweep_lists(dim3 grid, size_t lds, hipStream_t stream, int n, uint64_t seed_base, int64_t first,
                               int64_t n_inst, const uint8_t *lists, uint64_t ld, uint64_t inst_stride, int32_t *out,
                               const QbaMcCounts &cv, const QbaMcScen &sv);

namespace {

// The fields of a policy word, decoded once before the rounds (scalars).
struct ProtoAdv {
  uint32_t acts, nacts, order, fresh, comm;
};

__device__ __forceinline__ ProtoAdv proto_adv_of(uint32_t adv) {
  return ProtoAdv{adv & 0x1Fu, (uint32_t)__popc(adv & 0x1Fu), (adv >> 8) & 3u, (adv >> 12) & 1u, (adv >> 16) & 1u};
}

// lieu_broadcast under the policy A (montecarlo.AdversaryParty.lieu_broadcast)
__device__ __forceinline__ void proto_broadcast_adv(ProtoShared &S, uint32_t *box, int box_ld, int w, int n, int me,
                                                    bool dishonest, const uint32_t pkt0, int buf, ProtoRng &rng,
                                                    int &sent, const ProtoAdv &A) {
  uint32_t pkt = pkt0;
  for (int dest = 2; dest <= n; ++dest) {
    if (dest == me) continue;
    uint32_t go = 1;
    if (dishonest) {
      if (A.fresh) pkt = pkt0;
      const uint32_t a = rng.randint(A.nacts);
      uint32_t action = 0, seen = 0;  // the a-th set bit of acts
      for (uint32_t b = 0; b < 5u; ++b) {
        if (!((A.acts >> b) & 1u)) continue;
        if (seen == a) action = b;
        ++seen;
      }
      if (action == 0) {
        go = rng.randint(2);
      } else if (action == 1) {
        uint32_t v;
        if (A.order == 1u) v = (pkt & 15u) == 0u ? 1u : 0u;
        else v = rng.randint(A.order == 0u ? (uint32_t)n + 1u : (uint32_t)w);
        pkt = (pkt & ~15u) | v;
      } else if (action == 2) {
        pkt |= QBA_PKT_CLEARED;
      } else if (action == 3) {
        pkt &= ~(QBA_PKT_EMPTY | 0xFFFF0000u);
      }
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

// proto_rounds under the policy word `adv` (wave-uniform): the same arguments,
// state and result row.
template <bool WG>
__device__ __forceinline__ void proto_rounds_adv(ProtoShared &S, uint32_t *box, int n, int n_dis, uint64_t key,
                                                 uint32_t pnz, uint32_t st0, int lane, int32_t *__restrict__ o,
                                                 uint32_t adv) {
  const int G = n + 1, nq = 32 - __clz(n), w = 1 << nq;  // nq = ceil(log2(n + 1)), tfg.py:317
  const int box_ld = G * w + 1;
  const ProtoAdv A = proto_adv_of(adv);
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

  // ---- the commander's order(s); v1 and v2 are drawn as the reference draws them
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
      const bool first = A.comm ? !(dest & 1) : dest <= (n + 1) / 2;
      S.cv[dest] = first ? v1 : v2;
      ++sent;
    }
    decision = (int)v;
  }
  proto_sync<WG>();

  // ---- epoch 0, the lieutenants take the commander's packet --------------------
  if (lieutenant) {
    for (int d = 0; d < G; ++d) S.cnt[d * QBA_PROTO_MAXG + lane] = 0;
    uint32_t pkt = S.cv[lane] | (S.cv[lane] << 4);
    int len;
    if (proto_check(S, pkt, lane, G, pnz, len)) {
      ++accept;
      Vi |= 1u << (pkt & 15u);
      proto_broadcast_adv(S, box, box_ld, w, n, lane, dishonest, pkt, 0, rng, sent, A);
    } else {
      ++reject;
    }
  }
  proto_sync<WG>();

  // ---- rounds 1 .. n_dis + 1 ----------------------------------------------------
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
            if (rnd <= n_dis) proto_broadcast_adv(S, box, box_ld, w, n, lane, dishonest, pkt, wb, rng, sent, A);
          }
        }
      }
    }
    proto_sync<WG>();
  }

  // ---- decisions and success ----------------------------------------------------
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

}  // namespace
