// qba_proto_net.hip -- qba_k_mc_lists_curve_adv (qba_proto_adv.hip) with the
// rounds on a network that loses packets (proto_rounds_net, qba_proto_net.h;
// DESIGN.md section 13.11).  What feeds the rounds -- the distillation of byte
// rows into the running masks of a curve -- is what that kernel does; the
// kernel is a text of its own in a code object of its own, with that kernel's
// LDS layout.  Its name (qba_k_mc_net_lists) contains none of
// "qba_k_protocol", "qba_k_mc_curve_", "qba_k_mc_lists", "qba_k_mc_sweep",
// "_adv", "coal" and "trace": the sibling descriptor tests find their kernels
// by those.
// The C entry point and its checks are in qba_proto.hip; this file holds the
// kernel and its launch function.
#include "qba_proto_net.h"

namespace {

__global__ __launch_bounds__(QBA_PROTO_BLOCK) void qba_k_mc_net_lists(int n, int n_dis, uint64_t seed_base,
                                                                      int64_t inst0, int64_t n_inst,
                                                                      const uint8_t *__restrict__ lists, uint64_t ld,
                                                                      uint64_t inst_stride, int32_t *__restrict__ out,
                                                                      const QbaMcCounts cv, uint32_t adv,
                                                                      uint32_t net) {
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
    proto_rounds_net<true>(S, box, n, n_dis, seed_base + (uint64_t)inst, pnz, st, lane,
                           out + ((int64_t)j * n_inst + inst) * (int64_t)(4 + 5 * G), adv, net);
    lo = hi;
  }
}

}  // namespace

void qba_launch_mc_net_lists(dim3 grid, size_t lds, hipStream_t stream, int n, int n_dis, uint64_t seed_base,
                             int64_t first, int64_t n_inst, const uint8_t *lists, uint64_t ld, uint64_t inst_stride,
                             int32_t *out, const QbaMcCounts &cv, uint32_t adv, uint32_t net) {
  hipLaunchKernelGGL(qba_k_mc_net_lists, grid, dim3(QBA_PROTO_BLOCK), lds, stream, n, n_dis, seed_base, first, n_inst,
                     lists, ld, inst_stride, out, cv, adv, net);
}
