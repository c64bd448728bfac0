// qba_proto_adv.hip -- qba_k_protocol, qba_k_mc_lists and qba_k_mc_curve_lists
// (qba_proto.hip) with the rounds under an adversary policy
// (proto_rounds_adv, qba_proto_adv.h).  What feeds the
// rounds -- the tables prologue, the distillation of byte rows, the running
// masks of a curve -- is what those kernels do; the kernels are texts of their
// own in a code object of their own, so that qba_proto.hip's stays what it was.
// Their names (qba_k_proto_adv, qba_k_mc_lists_adv, qba_k_mc_lists_curve_adv)
// do not contain "qba_k_protocol" or "qba_k_mc_curve_lists": the descriptor
// tests find exactly one kernel by each of those.
// The C entry points and their checks are in qba_proto.hip; this file holds
// the kernels and one launch function each.
#include "qba_proto_adv.h"

namespace {

__global__ __launch_bounds__(QBA_PROTO_BLOCK) void qba_k_proto_adv(int n, int n_dis, uint64_t seed_base,
                                                                      int64_t inst0, const int64_t *__restrict__ Hd,
                                                                      const int64_t *__restrict__ Cd,
                                                                      const int64_t *__restrict__ Pd,
                                                                      int32_t *__restrict__ out, uint32_t adv) {
  // ProtoShared | box [2][G][box_ld] (C flags in the prologue): all dynamic, as in the list kernels
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(lds);
  uint32_t *box = lds + PROTO_S_WORDS;
  const int lane = threadIdx.x;
  const int G = n + 1, nq = 32 - __clz(n), w = 1 << nq;  // nq = ceil(log2(n + 1)), tfg.py:317
  const int64_t inst = inst0 + blockIdx.x;
  const int64_t *H = Hd + inst * (int64_t)(w * G * w);
  const int64_t *C = Cd + inst * (int64_t)(w * G * G);
  const int64_t *P = Pd + inst * (int64_t)w;

  // ---- prologue: distil the tables (qba_k_protocol's) -------------------------
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

  proto_rounds_adv<true>(S, box, n, n_dis, seed_base + (uint64_t)inst, pnz, 0u, lane,
                         out + inst * (int64_t)(4 + 5 * G), adv);
}

__global__ __launch_bounds__(QBA_PROTO_BLOCK) void qba_k_mc_lists_adv(int n, int n_dis, uint64_t seed_base,
                                                                      int64_t inst0, uint32_t count,
                                                                      const uint8_t *__restrict__ lists, uint64_t ld,
                                                                      uint64_t inst_stride,
                                                                      int32_t *__restrict__ out, uint32_t adv) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // ProtoShared | box [2][G][box_ld]
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(lds);
  uint32_t *box = lds + PROTO_S_WORDS;
  const int lane = threadIdx.x;
  const int G = n + 1, nq = 32 - __clz(n), w = 1 << nq;
  const int64_t inst = inst0 + blockIdx.x;
  const uint8_t *L = lists + (uint64_t)inst * inst_stride;
  mc_begin(S, box, G, w, lane);
  proto_sync<true>();
  uint32_t seen = 0, bad = 0;
  for (uint32_t k = (uint32_t)lane; k < count; k += 64u) {
    uint32_t D[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int g = 0; g < QBA_PROTO_MAXG; ++g)
      if (g < G) D[g / 4] |= (uint32_t)L[(uint64_t)g * ld + k] << (8 * (g % 4));
    mc_entry<true>(S, box, D, G, w, seen, bad);
  }
  mc_flags(box, G, w, seen, bad);
  proto_sync<true>();
  uint32_t st;
  const uint32_t pnz = mc_finish<true>(S, box, G, w, lane, st);
  proto_sync<true>();
  proto_rounds_adv<true>(S, box, n, n_dis, seed_base + (uint64_t)inst, pnz, st, lane,
                         out + inst * (int64_t)(4 + 5 * G), adv);
}

__global__ __launch_bounds__(QBA_PROTO_BLOCK) void qba_k_mc_lists_curve_adv(int n, int n_dis, uint64_t seed_base,
                                                                            int64_t inst0, int64_t n_inst,
                                                                            const uint8_t *__restrict__ lists,
                                                                            uint64_t ld, uint64_t inst_stride,
                                                                            int32_t *__restrict__ out,
                                                                            const QbaMcCounts cv, uint32_t adv) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // ProtoShared | box [2][G][box_ld] | acc
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(lds);
  uint32_t *box = lds + PROTO_S_WORDS;
  const int lane = threadIdx.x;
  const int G = n + 1, nq = 32 - __clz(n), w = 1 << nq;
  uint32_t *acc = box + ((proto_box_words(G, w) + 3) & ~3);
  uint32_t *mcw = acc + w * G;
  const int64_t inst = inst0 + blockIdx.x;
  const uint8_t *L = lists + (uint64_t)inst * inst_stride;
  mc_acc_begin(acc, G, w, lane);
  uint32_t seen = 0, bad = 0, lo = 0;
  for (int j = 0; j < cv.n; ++j) {
    const uint32_t hi = cv.c[j];
    proto_sync<true>();
    for (uint32_t k = lo + (uint32_t)lane; k < hi; k += 64u) {
      uint32_t D[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int g = 0; g < QBA_PROTO_MAXG; ++g)
        if (g < G) D[g / 4] |= (uint32_t)L[(uint64_t)g * ld + k] << (8 * (g % 4));
      mc_entry_at<true>(acc, G, mcw, D, G, w, seen, bad);
    }
    mc_flags(mcw, G, w, seen, bad);
    proto_sync<true>();
    uint32_t st;
    const uint32_t pnz = mc_acc_finish<true>(S, acc, G, w, lane, st);
    proto_sync<true>();
    proto_rounds_adv<true>(S, box, n, n_dis, seed_base + (uint64_t)inst, pnz, st, lane,
                           out + ((int64_t)j * n_inst + inst) * (int64_t)(4 + 5 * G), adv);
    lo = hi;
  }
}

}  // namespace

void qba_launch_protocol_adv(dim3 grid, size_t lds, hipStream_t stream, int n, int n_dis, uint64_t seed_base,
                             int64_t first, const int64_t *H, const int64_t *C, const int64_t *P, int32_t *out,
                             uint32_t adv) {
  hipLaunchKernelGGL(qba_k_proto_adv, grid, dim3(QBA_PROTO_BLOCK), lds, stream, n, n_dis, seed_base, first, H, C, P,
                     out, adv);
}

void qba_launch_mc_lists_adv(dim3 grid, size_t lds, hipStream_t stream, int n, int n_dis, uint64_t seed_base,
                             int64_t first, uint32_t count, const uint8_t *lists, uint64_t ld, uint64_t inst_stride,
                             int32_t *out, uint32_t adv) {
  hipLaunchKernelGGL(qba_k_mc_lists_adv, grid, dim3(QBA_PROTO_BLOCK), lds, stream, n, n_dis, seed_base, first, count,
                     lists, ld, inst_stride, out, adv);
}

void qba_launch_mc_curve_lists_adv(dim3 grid, size_t lds, hipStream_t stream, int n, int n_dis, uint64_t seed_base,
                                   int64_t first, int64_t n_inst, const uint8_t *lists, uint64_t ld,
                                   uint64_t inst_stride, int32_t *out, const QbaMcCounts &cv, uint32_t adv) {
  hipLaunchKernelGGL(qba_k_mc_lists_curve_adv, grid, dim3(QBA_PROTO_BLOCK), lds, stream, n, n_dis, seed_base, first,
                     n_inst, lists, ld, inst_stride, out, cv, adv);
}
