// qba_proto.hip -- the count-mode protocol rounds of many independent
// instances on the device (qba_protocol_batched): tfg.py:101-125 (dishonest
// draw), 166-196 (commander broadcast), 266-306 (lieutenant rounds, decision)
// and 337-363 (round loop, success), evaluated from the per-instance count
// tables of qba_sample_check_batched exactly as countmode.CountParty does under
// protocol.run_local (barrier-epoch delivery, comm.py).  DESIGN.md section 13.
//
// One wavefront (a 64-thread workgroup) per instance; lane r is rank r
// (0 = QSD, 1 = commander, >= 2 = lieutenants).
//   prologue  the int64 tables are read once, coalesced, and distilled into
//             LDS: P[u] != 0; per (u, g) the mask of x with H[u][g][x] != 0,
//             the mask of h with C[u][g][h] == 0 and rep(u, g) = min h with
//             C[u][g][h] == P[u]  (what CountTables.desc / consistent consult)
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
#include "qba_internal.h"

#define QBA_PROTO_BLOCK 64
#define QBA_PROTO_MAXG 16       // ranks 0..15
#define QBA_PROTO_LAUNCH (1 << 20)  // instances per launch

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
  int64_t p64[16];                                   // P[u] (prologue)
  uint32_t tab[16 * QBA_PROTO_MAXG];                 // [u][g]: H mask | C-zero mask << 16
  uint8_t rep[16 * QBA_PROTO_MAXG];                  // [u][g]: rep(u, g)
  uint8_t cnt[2 * QBA_PROTO_MAXG * QBA_PROTO_MAXG];  // [buf][dest][src] packets in box
  int32_t dec[QBA_PROTO_MAXG];                       // decisions
  uint32_t cv[QBA_PROTO_MAXG];                       // commander's v per destination
  uint32_t dis_mask;
};

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

__global__ __launch_bounds__(QBA_PROTO_BLOCK) void qba_k_protocol(int n, int n_dis, uint64_t seed_base,
                                                                  int64_t inst0, const int64_t *__restrict__ Hd,
                                                                  const int64_t *__restrict__ Cd,
                                                                  const int64_t *__restrict__ Pd,
                                                                  int32_t *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t box[];  // [2][G][box_ld]; C flags in the prologue
  __shared__ ProtoShared S;
  const int lane = threadIdx.x;
  const int G = n + 1, nq = 32 - __clz(n), w = 1 << nq;  // nq = ceil(log2(n + 1)), tfg.py:317
  const int box_ld = G * w + 1;  // + 1: the lanes' inbox rows start on different banks
  const int64_t inst = inst0 + blockIdx.x;
  const int64_t *H = Hd + inst * (int64_t)(w * G * w);
  const int64_t *C = Cd + inst * (int64_t)(w * G * G);
  const int64_t *P = Pd + inst * (int64_t)w;

  // ---- prologue: distil the tables ------------------------------------------
  if (lane < w) S.p64[lane] = P[lane];
  __syncthreads();
  uint32_t pnz = 0;
  for (int u = 0; u < w; ++u) pnz |= (uint32_t)(S.p64[u] != 0) << u;
  {
    const int nH = w * G * w, per = 64 >> nq;
    for (int base = 0; base < nH; base += 64) {
      const int i = base + lane;
      const bool nz = i < nH && H[i] != 0;
      const unsigned long long bal = __ballot(nz);
      const int e = (base >> nq) + lane;
      if (lane < per && e < w * G)
        S.tab[(e / G) * QBA_PROTO_MAXG + e % G] = (uint32_t)(bal >> (lane * w)) & ((1u << w) - 1u);
    }
    uint8_t *cflag = reinterpret_cast<uint8_t *>(box);  // w*G*G bytes <= the mailbox's
    const int nC = w * G * G;
    for (int i = lane; i < nC; i += 64) {
      const int64_t c = C[i];
      cflag[i] = (uint8_t)((c == 0 ? 1 : 0) | (c == S.p64[i / (G * G)] ? 2 : 0));
    }
    __syncthreads();
    for (int e = lane; e < w * G; e += 64) {
      uint32_t cz = 0;
      int rep = -1;
      for (int h = 0; h < G; ++h) {
        const uint32_t f = cflag[e * G + h];
        cz |= (f & 1u) << h;
        if ((f & 2u) && rep < 0) rep = h;
      }
      const int at = (e / G) * QBA_PROTO_MAXG + e % G;
      S.tab[at] |= cz << 16;
      S.rep[at] = (uint8_t)(rep < 0 ? e % G : rep);  // the diagonal is |P_u|: rep <= g always exists
    }
    __syncthreads();
  }

  const uint64_t key = seed_base + (uint64_t)inst;
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
  __syncthreads();
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
  __syncthreads();

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
  __syncthreads();

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
    __syncthreads();
  }

  // ---- tfg.py:303-306, 352-363: decisions and success --------------------------
  if (lieutenant) decision = Vi ? __ffs((int)Vi) - 1 : -1;
  if (lane <= n) S.dec[lane] = decision;
  const uint32_t empty_mask = (uint32_t)__ballot(lieutenant && Vi == 0);
  const uint32_t status = (__ballot(rng.status & QBA_PROTO_ST_MAILBOX) ? QBA_PROTO_ST_MAILBOX : 0u) |
                          (__ballot(rng.status & QBA_PROTO_ST_RNG) ? QBA_PROTO_ST_RNG : 0u);
  __syncthreads();
  int32_t *o = out + inst * (int64_t)(4 + 5 * G);
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

extern "C" int qba_protocol_batched(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                    const int64_t *H, const int64_t *C, const int64_t *P, int32_t *out,
                                    qba_stream stream) {
  if (n < 1 || n > QBA_MAX_PARTIES)
    return qba_fail(QBA_EINVAL, "qba_protocol_batched: n_parties must be in [1, 15]");
  if (n_dis < 0 || n_dis > n)
    return qba_fail(QBA_EINVAL, "qba_protocol_batched: n_dishonest must be in [0, n_parties]");
  if (!ctx) return qba_fail(QBA_EINVAL, "qba_protocol_batched: ctx is NULL");
  if (n_inst < 0) return qba_fail(QBA_EINVAL, "qba_protocol_batched: n_instances < 0");
  if (n_inst == 0) return QBA_OK;
  if (!H || !C || !P || !out) return qba_fail(QBA_EINVAL, "qba_protocol_batched: a table or out pointer is NULL");
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  const int G = n + 1, w = 1 << qba_nq(n);
  const size_t lds = (size_t)2 * G * (G * w + 1) * sizeof(uint32_t);  // <= 32896 B at n = 15
  for (int64_t first = 0; first < n_inst; first += QBA_PROTO_LAUNCH) {
    const int64_t blocks = n_inst - first < QBA_PROTO_LAUNCH ? n_inst - first : QBA_PROTO_LAUNCH;
    hipLaunchKernelGGL(qba_k_protocol, dim3((unsigned)blocks), dim3(QBA_PROTO_BLOCK), lds, (hipStream_t)stream,
                       n, n_dis, seed_base, first, H, C, P, out);
    QBA_HIP(hipGetLastError());
  }
  return QBA_OK;
}
