// qba_proto_coal.h -- the protocol rounds of qba_proto_adv.h with traitors that
// know each other: a second 32-bit word, `coal`,
// beside the policy word `adv`.
//
//   bit  0       on       1: the traitors collude; coal == 0 is "no coalition",
//                         and proto_rounds_coal then draws the words
//                         proto_rounds_adv draws and writes its rows
//   bits [4:6)   when     the delivery round R: 0 n_dis + 1 (the last round: an
//                         acceptance there is never relayed), 1 max(1, n_dis)
//                         (the last round whose acceptances are relayed)
//   bits [8:10)  targets  the honest lieutenants that receive held packets:
//                         0 all, 1 those of even rank, 2 the lowest-ranked one
//   bit  12      starve   the dishonest commander sends v1 to every honest and
//                         v2 to every dishonest lieutenant
// Every other bit is 0, when <= 1, targets <= 2 and no field is set without
// `on` (qba_coal_bad).
//
// A dishonest lieutenant under `on`, per destination of a broadcast in round r
// (epoch 0 is r = 0): a dishonest destination gets the packet as it was handed
// to the broadcast and no word is drawn; a target, while r < R - 1, gets
// nothing and draws nothing -- the handed packet goes once to the lane's hold
// list; every other destination is served as proto_broadcast_adv serves it.
// In round R - 1, after its inbox walk, the lane sends its hold list in
// acceptance order to every target in ascending rank, each packet that has
// neither the EMPTY nor the CLEARED flag padded with pool rows until its mask
// holds R reps: rep(pu, g) of the dishonest lieutenants g ascending, then
// under a dishonest commander rep(pu, 0), its list, and (v != pu) rep(pu, 1),
// its extra list Lc, which equals pu on all of P_pu and so passes Cond2 under
// another v only; a row whose rep is in the mask already is skipped.
// montecarlo.CoalitionParty is the host restatement.
//
// The hold list is LDS, [G][w] words per instance in flight (lane r owns words
// [r * w, r * w + w)); its fill is a register of the lane, set to 0 by every
// call of the rounds, so nothing of a run is read by the next.  A lane holds a
// packet only on adding its v to V_i, so at most w packets: bounds-checked.
// The deliveries read S.rep and the dishonest mask alone.
//
// The mailbox bound of w slots per (dest, src, round) holds: in round R - 1 a
// lane's ordinary sends to a target each carry a v new to its V_i and its held
// packets each carry a distinct v already in it, together at most w.
//
// proto_broadcast_coal and proto_rounds_coal are texts of their own: the
// kernels that existed before them keep their rounds and their code.
#pragma once
#include "qba_proto_adv.h"

#define QBA_COAL_VALID 0x00001331u  // the bits a coalition word may set

// What is wrong with a coalition word (NULL: nothing), for qba_mc_check's envelope
inline const char *qba_coal_bad(uint32_t coal) {
  if (coal & ~QBA_COAL_VALID) return "coal sets a reserved bit";
  if (((coal >> 4) & 3u) > 1u) return "coal's when field must be <= 1";
  if (((coal >> 8) & 3u) > 2u) return "coal's targets field must be <= 2";
  if (!(coal & 1u)) {
    if ((coal >> 4) & 3u) return "coal sets the when field without on";
    if ((coal >> 8) & 3u) return "coal sets the targets field without on";
    if ((coal >> 12) & 1u) return "coal sets the starve field without on";
  }
  return nullptr;
}

// Hold-list words of one instance: [G][w]
__host__ __device__ constexpr int proto_hold_words(int G, int w) { return (G * w + 3) & ~3; }

// The launch of qba_proto_coal.hip's kernel, for the entry point in qba_proto.hip
void qba_launch_mc_coal_lists(dim3 grid, size_t lds, hipStream_t stream, int n, int n_dis, uint64_t seed_base,
                              int64_t first, int64_t n_inst, const uint8_t *lists, uint64_t ld, uint64_t inst_stride,
                              int32_t *out, const QbaMcCounts &cv, uint32_t adv, uint32_t coal);

namespace {

// A coalition word decoded for one run (scalars): R from n_dis, the traitors
// and the targets from the dishonest mask.
struct ProtoCoal {
  uint32_t on, starve, dis, tmask;
  int R;
};

__device__ __forceinline__ ProtoCoal proto_coal_of(uint32_t coal, int n, int n_dis, uint32_t dis_mask) {
  ProtoCoal K;
  K.on = coal & 1u;
  K.starve = (coal >> 12) & 1u;
  K.R = ((coal >> 4) & 3u) == 0u ? n_dis + 1 : (n_dis > 1 ? n_dis : 1);
  K.dis = dis_mask;
  const uint32_t honest = ((2u << n) - 4u) & ~dis_mask, sel = (coal >> 8) & 3u;  // lieutenants 2 .. n
  K.tmask = sel == 0u ? honest : sel == 1u ? honest & 0x5555u : honest & (0u - honest);
  return K;
}

// One send of `me` to `dest` into the round buffer `buf` (the tail of proto_broadcast_adv)
__device__ __forceinline__ void proto_put(ProtoShared &S, uint32_t *box, int box_ld, int w, int n, int me, int dest,
                                          uint32_t pkt, int buf, ProtoRng &rng, int &sent) {
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

// lieu_broadcast of a packet accepted in round rnd, under the policy A and the
// coalition K (montecarlo.CoalitionParty.lieu_broadcast)
__device__ __forceinline__ void proto_broadcast_coal(ProtoShared &S, uint32_t *box, int box_ld, int w, int n, int me,
                                                     bool dishonest, const uint32_t pkt0, int buf, ProtoRng &rng,
                                                     int &sent, const ProtoAdv &A, const ProtoCoal &K, int rnd,
                                                     uint32_t *hold, int &nheld) {
  const bool collude = dishonest && K.on;
  const bool early = rnd < K.R - 1;
  bool held = false;
  uint32_t pkt = pkt0;
  for (int dest = 2; dest <= n; ++dest) {
    if (dest == me) continue;
    if (collude && ((K.dis >> dest) & 1u)) {  // a fellow traitor: the handed packet, no draw
      proto_put(S, box, box_ld, w, n, me, dest, pkt0, buf, rng, sent);
      continue;
    }
    if (collude && early && ((K.tmask >> dest) & 1u)) {  // withheld: once per accepted packet
      if (!held) {
        if (nheld < w) hold[nheld++] = pkt0;
        else rng.status |= QBA_PROTO_ST_MAILBOX;
        held = true;
      }
      continue;
    }
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
    if (go) proto_put(S, box, box_ld, w, n, me, dest, pkt, buf, rng, sent);
  }
}

// The hold list of `me`, padded from the pool, to every target (round R - 1,
// after the lane's ordinary sends)
__device__ __forceinline__ void proto_deliver_coal(ProtoShared &S, uint32_t *box, int box_ld, int w, int n, int me,
                                                   int buf, ProtoRng &rng, int &sent, const ProtoCoal &K,
                                                   const uint32_t *hold, int nheld) {
  for (int k = 0; k < nheld; ++k) {
    uint32_t pkt = hold[k];
    if (!(pkt & (QBA_PKT_EMPTY | QBA_PKT_CLEARED))) {
      const uint32_t pu = (pkt >> 4) & 15u;
      const uint8_t *rep = &S.rep[pu * QBA_PROTO_MAXG];
      // a pool row: skipped when its rep is in the mask, dropped when the mask is full
      auto pad = [&](int g) {
        const uint32_t bit = 0x10000u << rep[g];
        if (__popc(pkt >> 16) < K.R && !(pkt & bit)) pkt |= bit;
      };
      for (int g = 2; g <= n; ++g)
        if ((K.dis >> g) & 1u) pad(g);
      if ((K.dis >> 1) & 1u) {  // row 0: the commander's list; row 1: Lc, which is pu on all of P_pu
        pad(0);
        if ((pkt & 15u) != pu) pad(1);
      }
    }
    for (int dest = 2; dest <= n; ++dest)
      if ((K.tmask >> dest) & 1u) proto_put(S, box, box_ld, w, n, me, dest, pkt, buf, rng, sent);
  }
}

// proto_rounds_adv under the coalition word `coal` (wave-uniform): the same
// arguments, state and result row; hold_all is the instance's hold area,
// proto_hold_words(n + 1, w) words.
template <bool WG>
__device__ __forceinline__ void proto_rounds_coal(ProtoShared &S, uint32_t *box, uint32_t *hold_all, int n, int n_dis,
                                                  uint64_t key, uint32_t pnz, uint32_t st0, int lane,
                                                  int32_t *__restrict__ o, uint32_t adv, uint32_t coal) {
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
  const ProtoCoal K = proto_coal_of(coal, n, n_dis, dis_mask);
  uint32_t *hold = hold_all + (lieutenant ? lane : 0) * w;  // read and written by lieutenants alone
  int nheld = 0;

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
      const bool first = (K.on && K.starve) ? !((dis_mask >> dest) & 1u)
                                            : A.comm ? !(dest & 1) : dest <= (n + 1) / 2;
      S.cv[dest] = first ? v1 : v2;
      ++sent;
    }
    decision = (int)v;
  }
  proto_sync<WG>();

  // ---- epoch 0, the lieutenants take the commander's packet --------------------
  // (R - 1 == 0 holds nothing -- no round is earlier -- so epoch 0 delivers nothing)
  if (lieutenant) {
    for (int d = 0; d < G; ++d) S.cnt[d * QBA_PROTO_MAXG + lane] = 0;
    uint32_t pkt = S.cv[lane] | (S.cv[lane] << 4);
    int len;
    if (proto_check(S, pkt, lane, G, pnz, len)) {
      ++accept;
      Vi |= 1u << (pkt & 15u);
      proto_broadcast_coal(S, box, box_ld, w, n, lane, dishonest, pkt, 0, rng, sent, A, K, 0, hold, nheld);
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
            if (rnd <= n_dis)
              proto_broadcast_coal(S, box, box_ld, w, n, lane, dishonest, pkt, wb, rng, sent, A, K, rnd, hold, nheld);
          }
        }
      }
      if (rnd == K.R - 1) proto_deliver_coal(S, box, box_ld, w, n, lane, wb, rng, sent, K, hold, nheld);
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
