// qba_proto_nettrace.h -- the protocol rounds of qba_proto_net.h writing the
// transcript of qba_proto_trace.h:
// proto_rounds_nettrace is proto_rounds_net plus the event stores of
// proto_rounds_trace.  It draws the words proto_rounds_net draws, in its order
// (the loss bits of a broadcast before its loop, nothing when drop_q16 == 0),
// and writes its row; with net == 0 its events are proto_rounds_trace's word
// for word.
//
// Two events beyond section 13.9's:
//   SEND slot QBA_EV_SLOT_LOST (29)  the packet was handed to a lossy link and
//               lost in flight: it counts in `sent` and advances the link's
//               seq, takes no mailbox slot (the next send to that destination
//               in that round gets the slot this one would have had); code the
//               drawn action or QBA_EV_HONEST, len and pkt those of the packet
//               as handed over, after a traitor's mutation.  Under cmd the
//               commander's round-0 SEND carries it too.
//   RECV code QBA_EV_NO_PACKET (6)   the one event of a lieutenant whose
//               commander packet was lost: round 0, peer 1, slot 0, len 0,
//               pkt 0; neither an accept nor a reject.
// A send that action 0 suppresses stays QBA_EV_SLOT_MUTED: it is not handed to
// the link and seq does not move.  A lost lieutenant-to-lieutenant packet leaves
// no event at the receiver.
//
// proto_check_trace supplies the verdict and ProtoTrace::put does the stores
// (qba_proto_trace.h).  proto_broadcast_nettrace and proto_rounds_nettrace are
// texts of their own: qba_proto_net.h, qba_proto_trace.h and the kernels built
// on them keep their code.
#pragma once
#include "qba_proto_net.h"
#include "qba_proto_trace.h"

// QBA_EV_SLOT_LOST, QBA_EV_NO_PACKET: qba.h

// The launches of qba_proto_nettrace.hip's and qba_mc_nettrace_inst.hip's
// kernels (one wavefront per slot of idx), for the entry points in
// qba_proto_nettrace.hip
struct QbaNetTrace {
  QbaTrace t;
  uint32_t net;
};
template <int NP>
int qba_launch_mc_nettrace(qba_ctx *ctx, const QbaNetTrace &T);

namespace {

// proto_broadcast_net with a SEND event per destination
__device__ __forceinline__ void proto_broadcast_nettrace(ProtoShared &S, uint32_t *box, int box_ld, int w, int n, int me,
                                                         bool dishonest, const uint32_t pkt0, int buf, ProtoRng &rng,
                                                         int &sent, const ProtoAdv &A, const ProtoNet &N, uint32_t e,
                                                         uint64_t &seqs, ProtoTrace &T) {
  uint32_t pkt = pkt0;
  // the loss bits of the whole broadcast, as proto_broadcast_net draws them
  uint32_t lost = 0;
  if (N.drop) {  // wave-uniform
#pragma nounroll
    for (int dest = 2; dest <= n; ++dest) {
      const uint32_t seq = (uint32_t)(seqs >> (4 * (dest - 2))) & 15u;
      lost |= (uint32_t)proto_net_lost(rng.k0, rng.k1, e, (uint32_t)me, (uint32_t)dest, seq, N.drop) << dest;
    }
  }
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
      bool gone = false;
      if (N.drop) {
        const int sh = 4 * (dest - 2);
        const uint32_t seq = (uint32_t)(seqs >> sh) & 15u;
        seqs = (seqs & ~(15ull << sh)) | ((uint64_t)((seq + 1u) & 15u) << sh);
        gone = (lost >> dest) & 1u;
      }
      if (gone) {
        slot = QBA_EV_SLOT_LOST;
      } else {
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
    }
    T.put(QBA_EV_SEND, (int)e, dest, slot, action, proto_trace_len(pkt), proto_trace_canon(pkt));
  }
}

// proto_rounds_net with the transcript: the arguments, the event regions and
// the counts of proto_rounds_trace, the network word of proto_rounds_net.
template <bool WG>
__device__ __forceinline__ void proto_rounds_nettrace(ProtoShared &S, uint32_t *box, int n, int n_dis, uint64_t key,
                                                      uint32_t pnz, uint32_t st0, int lane, int32_t *__restrict__ o,
                                                      uint32_t adv, uint32_t net, uint2 *ev, uint32_t cap,
                                                      int32_t *__restrict__ cnt) {
  const int G = n + 1, nq = 32 - __clz(n), w = 1 << nq;  // nq = ceil(log2(n + 1)), tfg.py:317
  const int box_ld = G * w + 1;
  const ProtoAdv A = proto_adv_of(adv);
  const ProtoNet N = proto_net_of(net);
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

  // ---- the commander's order(s); under cmd each of its sends (seq 0 of its link
  // ---- in epoch 0) may be lost
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
      const bool gone = N.cmd && proto_net_lost(rng.k0, rng.k1, 0u, 1u, (uint32_t)dest, 0u, N.drop);
      S.cv[dest] = gone ? QBA_NET_CV_LOST : cv;
      ++sent;
      T.put(QBA_EV_SEND, 0, dest, gone ? QBA_EV_SLOT_LOST : 0u, QBA_EV_HONEST, 0, cv | (cv << 4));
    }
    decision = (int)v;
  }
  proto_sync<WG>();

  // ---- epoch 0, the lieutenants take the commander's packet (if it arrived) ----
  uint64_t seqs = 0;
  if (lieutenant) {
    for (int d = 0; d < G; ++d) S.cnt[d * QBA_PROTO_MAXG + lane] = 0;
    const uint32_t cv = S.cv[lane];
    if (cv != QBA_NET_CV_LOST) {
      uint32_t pkt = cv | (cv << 4);
      const uint32_t read = pkt;
      int len;
      const uint32_t code = proto_check_trace(S, pkt, lane, G, pnz, len);
      T.put(QBA_EV_RECV, 0, 1, 0u, code, len, read);
      if (!code) {
        ++accept;
        Vi |= 1u << (pkt & 15u);
        proto_broadcast_nettrace(S, box, box_ld, w, n, lane, dishonest, pkt, 0, rng, sent, A, N, 0u, seqs, T);
      } else {
        ++reject;
      }
    } else {
      T.put(QBA_EV_RECV, 0, 1, 0u, QBA_EV_NO_PACKET, 0, 0u);
    }
  }
  proto_sync<WG>();

  // ---- rounds 1 .. n_dis + 1 ----------------------------------------------------
  for (int rnd = 1; rnd <= n_dis + 1; ++rnd) {
    const int wb = rnd & 1, rb = wb ^ 1;
    seqs = 0;
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
            if (rnd <= n_dis)
              proto_broadcast_nettrace(S, box, box_ld, w, n, lane, dishonest, pkt, wb, rng, sent, A, N, (uint32_t)rnd,
                                       seqs, T);
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
