// qba_proto_net.h -- the protocol rounds of qba_proto_adv.h on a network that
// loses packets: a second 32-bit word, `net`, beside
// the policy word `adv`.
//
//   bits [0:16)  drop_q16  a packet on a lossy link is lost with probability
//                          drop_q16 / 65536
//   bit  16      cmd       1: the commander's n - 1 sends of epoch 0 cross a
//                          lossy link too; 0: only lieutenant-to-lieutenant
//                          packets do
// Every other bit is 0 and cmd is not set with drop_q16 == 0 (qba_net_bad).
// net == 0 is the perfect network, and proto_rounds_net then draws the words
// proto_rounds_adv draws and writes its rows.
//
// Loss is a pure function of the packet, not a position in a stream: with
// key = seed_base + i, the epoch e in which the packet is sent (0 for the
// commander's epoch and the relays after step 3a, r for round r), src, dest and
// seq = the number of packets src has already handed to the link towards dest
// in epoch e (sends suppressed by action 0 are not handed over), the packet is
// lost iff
//   (word(seq & 3) of philox(ctr = {e, src | dest << 8, seq >> 2, QBA_NET_CTR_TAG},
//                            key = {key_lo, key_hi}) & 0xFFFF) < drop_q16
// The test sees what the sender hands over, after a traitor's mutation, from
// honest and dishonest senders alike.  montecarlo.NetParty is the host
// restatement, montecarlo.net_lost the function.
//
// A lost packet counts in the sender's `sent`, advances seq, takes no mailbox
// slot and is never seen by the receiver.  Under cmd a lieutenant whose
// commander packet is lost skips step 3a (no accept, no reject, no relay) and
// enters the rounds with an empty V_i.
//
// seq: a sender adds a v to its V_i at most 16 times in an epoch, so it hands
// at most 16 packets to one link and the seq of a send is < 16.  The 14 counters
// of a lane (dest = 2 .. 15) are the nibbles of one 64-bit register, reset at
// every epoch; the broadcast's loop over dest shifts by a wave-uniform amount.
// No array, no LDS, no scratch.  The Philox block of (e, src, dest, seq >> 2) is
// recomputed at every broadcast: the sends of a lane to one link are
// interleaved with its sends to the other links (one per broadcast), so a
// cached block would have to be kept per destination -- 4 words x 14 in
// registers, or LDS the launch shape does not have.  A broadcast draws the loss
// bits of all its destinations before it serves them (a bit drawn for a send
// that action 0 then suppresses is not used: seq did not advance); with
// drop_q16 == 0 (wave-uniform) nothing is drawn.
//
// proto_broadcast_net and proto_rounds_net are texts of their own: the kernels
// that existed before them keep their rounds and their code.
#pragma once
#include "qba_proto_adv.h"

#define QBA_NET_VALID 0x0001FFFFu    // the bits a network word may set
#define QBA_NET_CTR_TAG 0x4E455457u  // word 3 of every loss counter ("NETW")

// What is wrong with a network word (NULL: nothing), for qba_mc_check's envelope
inline const char *qba_net_bad(uint32_t net) {
  if (net & ~QBA_NET_VALID) return "net sets a reserved bit";
  if (((net >> 16) & 1u) && !(net & 0xFFFFu)) return "net sets the cmd field with drop_q16 == 0";
  return nullptr;
}

// The launch of qba_proto_net.hip's kernel, for the entry point in qba_proto.hip
void qba_launch_mc_net_lists(dim3 grid, size_t lds, hipStream_t stream, int n, int n_dis, uint64_t seed_base,
                             int64_t first, int64_t n_inst, const uint8_t *lists, uint64_t ld, uint64_t inst_stride,
                             int32_t *out, const QbaMcCounts &cv, uint32_t adv, uint32_t net);
// ... and of qba_proto_grid.hip's (the curve under every scenario of `gv`)
void qba_launch_grid_lists(dim3 grid, size_t lds, hipStream_t stream, int n, uint64_t seed_base, int64_t first,
                           int64_t n_inst, const uint8_t *lists, uint64_t ld, uint64_t inst_stride, int32_t *out,
                           const QbaMcCounts &cv, const QbaMcGrid &gv);

namespace {

#define QBA_NET_CV_LOST 0xFFFFFFFFu  // S.cv[dest]: the commander's packet to dest was lost

// The fields of a network word, decoded once before the rounds (scalars).
struct ProtoNet {
  uint32_t drop, cmd;
};

__device__ __forceinline__ ProtoNet proto_net_of(uint32_t net) { return ProtoNet{net & 0xFFFFu, (net >> 16) & 1u}; }

// montecarlo.net_lost for drop > 0
__device__ __forceinline__ bool proto_net_lost(uint32_t k0, uint32_t k1, uint32_t e, uint32_t src, uint32_t dest,
                                               uint32_t seq, uint32_t drop) {
  const QbaU4 b = qba_philox(e, src | (dest << 8), seq >> 2, QBA_NET_CTR_TAG, k0, k1);
  const uint32_t j = seq & 3u;
  const uint32_t x = j == 0 ? b.x : j == 1 ? b.y : j == 2 ? b.z : b.w;
  return (x & 0xFFFFu) < drop;
}

// proto_broadcast_adv over lossy links (montecarlo.NetParty.send): `seqs` holds
// the lane's seq per destination in epoch e, nibble dest - 2.
__device__ __forceinline__ void proto_broadcast_net(ProtoShared &S, uint32_t *box, int box_ld, int w, int n, int me,
                                                    bool dishonest, const uint32_t pkt0, int buf, ProtoRng &rng,
                                                    int &sent, const ProtoAdv &A, const ProtoNet &N, uint32_t e,
                                                    uint64_t &seqs) {
  uint32_t pkt = pkt0;
  // A broadcast hands at most one packet to each link, so the seq of every
  // destination is known before the loop: the loss bits of the whole broadcast
  // are drawn here, where little else is live, and the loop tests a bit.
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
    if (N.drop) {
      const int sh = 4 * (dest - 2);
      const uint32_t seq = (uint32_t)(seqs >> sh) & 15u;
      seqs = (seqs & ~(15ull << sh)) | ((uint64_t)((seq + 1u) & 15u) << sh);
      if ((lost >> dest) & 1u) continue;
    }
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

// proto_rounds_adv under the network word `net` (wave-uniform): the same
// arguments, state and result row.
template <bool WG>
__device__ __forceinline__ void proto_rounds_net(ProtoShared &S, uint32_t *box, int n, int n_dis, uint64_t key,
                                                 uint32_t pnz, uint32_t st0, int lane, int32_t *__restrict__ o,
                                                 uint32_t adv, uint32_t net) {
  const int G = n + 1, nq = 32 - __clz(n), w = 1 << nq;  // nq = ceil(log2(n + 1)), tfg.py:317
  const int box_ld = G * w + 1;
  const ProtoAdv A = proto_adv_of(adv);
  const ProtoNet N = proto_net_of(net);
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
      uint32_t cv = first ? v1 : v2;
      if (N.cmd && proto_net_lost(rng.k0, rng.k1, 0u, 1u, (uint32_t)dest, 0u, N.drop)) cv = QBA_NET_CV_LOST;
      S.cv[dest] = cv;
      ++sent;
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
      int len;
      if (proto_check(S, pkt, lane, G, pnz, len)) {
        ++accept;
        Vi |= 1u << (pkt & 15u);
        proto_broadcast_net(S, box, box_ld, w, n, lane, dishonest, pkt, 0, rng, sent, A, N, 0u, seqs);
      } else {
        ++reject;
      }
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
          const uint32_t v = pkt & 15u;
          int len;
          const bool ok = proto_check(S, pkt, lane, G, pnz, len);
          if (ok) ++accept; else ++reject;
          if (ok && !((Vi >> v) & 1u) && len == rnd + 1) {
            Vi |= 1u << v;
            if (rnd <= n_dis)
              proto_broadcast_net(S, box, box_ld, w, n, lane, dishonest, pkt, wb, rng, sent, A, N, (uint32_t)rnd, seqs);
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
