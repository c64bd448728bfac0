// qba_proto_trace.h -- the protocol rounds of qba_proto_adv.h writing a
// transcript: proto_rounds_trace is proto_rounds_adv
// plus one event store per packet a rank processes, per destination a
// broadcast visits and per decision.  It draws the words proto_rounds_adv
// draws, in its order, and writes its row.
//
// An event is two uint32 {head, pkt}; head = kind [0:3) | round [3:8) |
// peer [8:12) | slot [12:17) | code [17:21) | len [21:26), every other bit 0:
//   RECV (1)    a packet a lieutenant processes: peer the source, slot the
//               mailbox slot read (the commander's packet: peer 1, slot 0, round
//               0), len proto_check's len, code the verdict -- 0 added to V_i;
//               1, 2, 3 the first of Cond1, Cond2, Cond3 that fails in
//               consistent's order; 4 consistent but v already in V_i; 5
//               consistent and new but len != round + 1
//   SEND (2)    a destination a broadcast visits: peer the destination, code the
//               drawn action 0..4 or 7 (an honest sender, the commander's round-0
//               sends included), len the lists of the packet sent, slot the
//               mailbox slot written, 31 for a send action 0 suppressed, 30 for
//               one dropped on a full mailbox
//   DECIDE (3)  the last event of every rank 1..n: pkt the decision, len |V_i|
// pkt is the packet word of qba_proto_rounds.h (RECV: as read, before the own
// descriptor joins; SEND: after the traitor's mutation) with the two fields
// that carry no information zeroed: P's u [4:8) under the cleared bit, and the
// descriptors' u [9:13) when the mask of reps is empty (proto_trace_canon).
// The words in the mailbox keep whatever those bits held.
//
// Lane r stores rank r's events to its own region ev[0 .. cap) with plain
// vector stores, the first `cap` of them; all are counted.  A text of its own:
// proto_rounds_adv, proto_check and the kernels built on them keep their code.
#pragma once
#include "qba_noise.h"
#include "qba_proto_adv.h"

// QBA_EV_*, QBA_TRACE_CAP_MAX: qba.h

// The launches of qba_proto_trace.hip's and qba_mc_trace_inst.hip's kernels
// (one wavefront per slot of idx), for the entry points in qba_proto_trace.hip
struct QbaTrace {
  const char *who;
  const QbaProgramSet *ps;  // the sampled form alone
  uint64_t seed_base;
  const int64_t *idx;
  int64_t n_idx;
  const int64_t *n_match;
  uint32_t count;
  int n_dis;
  uint32_t adv;
  QbaNoise noise;  // steps == 0: no noise
  uint32_t cap;
  int32_t *rows, *counts;
  uint32_t *events;
  hipStream_t stream;
};
template <int NP>
int qba_launch_mc_trace(qba_ctx *ctx, const QbaTrace &T);

namespace {

// One rank's event region and how many events it produced so far.
struct ProtoTrace {
  uint2 *ev;
  uint32_t cap, n;

  __device__ __forceinline__ void put(uint32_t kind, int round, int peer, uint32_t slot, uint32_t code, int len,
                                      uint32_t pkt) {
    if (n < cap)
      ev[n] = make_uint2(kind | (uint32_t)round << 3 | (uint32_t)peer << 8 | slot << 12 | code << 17 |
                             (uint32_t)len << 21,
                         pkt);
    ++n;
  }
};

__device__ __forceinline__ uint32_t proto_trace_canon(uint32_t pkt) {
  if (pkt & QBA_PKT_CLEARED) pkt &= ~(15u << 4);
  if (!(pkt >> 16)) pkt &= ~(15u << 9);
  return pkt;
}

__device__ __forceinline__ int proto_trace_len(uint32_t pkt) {
  return __popc(pkt >> 16) + ((pkt & QBA_PKT_EMPTY) ? 1 : 0);
}

// proto_check reporting which condition fails first: 0 consistent, else 1, 2, 3
// (consistent tests Cond2 on every tuple before Cond3 on any pair)
__device__ __forceinline__ uint32_t proto_check_trace(const ProtoShared &S, uint32_t &pkt, int g, int G, uint32_t pnz,
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
  if (empty && mask) return 1u;  // Cond1: lengths 0 and |P_u| > 0
  bool c2 = false, c3 = false;
  for (int a = 0; a < G; ++a) {
    if (!((mask >> a) & 1u)) continue;
    const uint32_t t = S.tab[du * QBA_PROTO_MAXG + a];
    if ((t >> v) & 1u) c2 = true;                                  // Cond2: v occurs in the tuple
    if ((mask & ~(1u << a)) & ~(t >> 16) & 0xFFFFu) c3 = true;     // Cond3: a shared position
  }
  return c2 ? 2u : c3 ? 3u : 0u;
}

// proto_broadcast_adv with a SEND event per destination
__device__ __forceinline__ void proto_broadcast_trace(ProtoShared &S, uint32_t *box, int box_ld, int w, int n, int me,
                                                      bool dishonest, const uint32_t pkt0, int buf, ProtoRng &rng,
                                                      int &sent, const ProtoAdv &A, ProtoTrace &T, int rnd) {
  uint32_t pkt = pkt0;
  for (int dest = 2; dest <= n; ++dest) {
    if (dest == me) continue;
    uint32_t go = 1, action = QBA_EV_HONEST;
    if (dishonest) {
      if (A.fresh) pkt = pkt0;
      const uint32_t a = rng.randint(A.nacts);
      uint32_t seen = 0;  // the a-th set bit of acts
      action = 0;
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
    uint32_t slot = QBA_EV_SLOT_MUTED;
    if (go) {
      ++sent;
      const int ci = (buf * QBA_PROTO_MAXG + dest) * QBA_PROTO_MAXG + me;
      const int k = S.cnt[ci];
      if (k < w) {
        box[(buf * (n + 1) + dest) * box_ld + me * w + k] = pkt;
        S.cnt[ci] = (uint8_t)(k + 1);
        slot = (uint32_t)k;
      } else {
        rng.status |= QBA_PROTO_ST_MAILBOX;
        slot = QBA_EV_SLOT_FULL;
      }
    }
    T.put(QBA_EV_SEND, rnd, dest, slot, action, proto_trace_len(pkt), proto_trace_canon(pkt));
  }
}

// proto_rounds_adv with the transcript: lane r's events go to ev (cap of them,
// nothing when st0 != 0: an instance refused while distilling has no
// transcript), and cnt[r], r = 0..n, gets how many rank r produced -- 0 in a
// row with a nonzero status, as every other field of such a row.
template <bool WG>
__device__ __forceinline__ void proto_rounds_trace(ProtoShared &S, uint32_t *box, int n, int n_dis, uint64_t key,
                                                   uint32_t pnz, uint32_t st0, int lane, int32_t *__restrict__ o,
                                                   uint32_t adv, uint2 *ev, uint32_t cap, int32_t *__restrict__ cnt) {
  const int G = n + 1, nq = 32 - __clz(n), w = 1 << nq;  // nq = ceil(log2(n + 1)), tfg.py:317
  const int box_ld = G * w + 1;
  const ProtoAdv A = proto_adv_of(adv);
  ProtoTrace T{ev, st0 ? 0u : cap, 0u};
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
      const uint32_t cv = first ? v1 : v2;
      S.cv[dest] = cv;
      ++sent;
      T.put(QBA_EV_SEND, 0, dest, 0u, QBA_EV_HONEST, 0, cv | (cv << 4));
    }
    decision = (int)v;
  }
  proto_sync<WG>();

  // ---- epoch 0, the lieutenants take the commander's packet --------------------
  if (lieutenant) {
    for (int d = 0; d < G; ++d) S.cnt[d * QBA_PROTO_MAXG + lane] = 0;
    uint32_t pkt = S.cv[lane] | (S.cv[lane] << 4);
    const uint32_t read = pkt;
    int len;
    const uint32_t code = proto_check_trace(S, pkt, lane, G, pnz, len);
    T.put(QBA_EV_RECV, 0, 1, 0u, code, len, read);
    if (!code) {
      ++accept;
      Vi |= 1u << (pkt & 15u);
      proto_broadcast_trace(S, box, box_ld, w, n, lane, dishonest, pkt, 0, rng, sent, A, T, 0);
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
          const uint32_t v = pkt & 15u, read = proto_trace_canon(pkt);
          int len;
          uint32_t code = proto_check_trace(S, pkt, lane, G, pnz, len);
          if (!code) ++accept; else ++reject;
          if (!code) code = (Vi >> v) & 1u ? 4u : len != rnd + 1 ? 5u : 0u;
          T.put(QBA_EV_RECV, rnd, src, (uint32_t)k, code, len, read);
          if (!code) {
            Vi |= 1u << v;
            if (rnd <= n_dis) proto_broadcast_trace(S, box, box_ld, w, n, lane, dishonest, pkt, wb, rng, sent, A, T, rnd);
          }
        }
      }
    }
    proto_sync<WG>();
  }

  // ---- decisions and success ----------------------------------------------------
  if (lieutenant) decision = Vi ? __ffs((int)Vi) - 1 : -1;
  if (lane >= 1 && lane <= n) T.put(QBA_EV_DECIDE, 0, 0, 0u, 0u, __popc(Vi), (uint32_t)decision);
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
    cnt[lane] = z ? 0 : (int32_t)T.n;
  }
}

}  // namespace
