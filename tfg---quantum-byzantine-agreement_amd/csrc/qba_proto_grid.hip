// qba_proto_grid.hip -- qba_k_grid_lists: qba_k_mc_net_lists (qba_proto_net.hip)
// deciding each checkpoint under every scenario (n_dishonest, adv, net) of a
// list.  The running masks are turned into S.tab /
// S.rep once per checkpoint and every scenario's rounds run on them:
// proto_rounds_net reads tab and rep through proto_check's `const ProtoShared &`
// and writes only S.dis_mask, S.cv (the lost-commander sentinel included),
// S.cnt, S.dec and the mailbox, each set again from the key before it is read;
// its seq counters are a register it resets itself; pnz and st are values.
// Every scenario runs proto_rounds_net, a perfect one too: at net == 0 it
// draws what proto_rounds_adv draws, and no loss block.  A text of its own in a
// code object of its own; its name contains none of the patterns the sibling
// descriptor tests find their kernels by.  The C entry point and its checks
// are in qba_proto.hip.
#include "qba_proto_net.h"

namespace {

__global__ __launch_bounds__(QBA_PROTO_BLOCK) void qba_k_grid_lists(int n, uint64_t seed_base, int64_t inst0,
                                                                    int64_t n_inst,
                                                                    const uint8_t *__restrict__ lists, uint64_t ld,
                                                                    uint64_t inst_stride, int32_t *__restrict__ out,
                                                                    const QbaMcCounts cv, const QbaMcGrid gv) {
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
#pragma nounroll
    for (int s = 0; s < gv.n; ++s) {
      proto_sync<true>();  // tab and rep are set; the previous scenario's row stores have read S
      proto_rounds_net<true>(S, box, n, gv.s[s].n_dishonest, seed_base + (uint64_t)inst, pnz, st, lane,
                             out + (((int64_t)j * gv.n + s) * n_inst + inst) * (int64_t)(4 + 5 * G), gv.s[s].adv,
                             gv.s[s].net);
    }
    lo = hi;
  }
}

}  // namespace

void qba_launch_grid_lists(dim3 grid, size_t lds, hipStream_t stream, int n, uint64_t seed_base, int64_t first,
                           int64_t n_inst, const uint8_t *lists, uint64_t ld, uint64_t inst_stride, int32_t *out,
                           const QbaMcCounts &cv, const QbaMcGrid &gv) {
  hipLaunchKernelGGL(qba_k_grid_lists, grid, dim3(QBA_PROTO_BLOCK), lds, stream, n, seed_base, first, n_inst, lists,
                     ld, inst_stride, out, cv, gv);
}
