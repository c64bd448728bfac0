// qba_proto_nprof.hip -- qba_k_mc_lists_curve_adv (qba_proto_adv.hip) with the
// masks of a noise profile (qba_noise_profile.h)
// XORed into the rows it reads, and qba_k_nprof_apply, which XORs them into
// byte rows in place (qba_k_noise_apply's sibling).  What feeds the rounds --
// the distillation of byte rows into the running masks of a curve -- and the
// rounds themselves (proto_rounds_adv, unedited) are that kernel's; the
// kernels are texts of their own in a code object of their own, with that
// kernel's LDS layout.  Their names (qba_k_nprof_lists, qba_k_nprof_apply)
// contain none of "qba_k_mc_", "qba_k_trace_", "qba_k_protocol",
// "qba_k_grid_", "_adv", "_noisy" and "qba_k_nettrace_": the sibling
// descriptor tests find their kernels by those.
// The C entry points and their checks are in qba_proto.hip and qba_lists.hip;
// this file holds the kernels and one launch function each.
#include "qba_noise_profile.h"
#include "qba_proto_adv.h"

namespace {

__global__ __launch_bounds__(QBA_PROTO_BLOCK) void qba_k_nprof_lists(int n, int n_dis, uint64_t seed_base,
                                                                     int64_t inst0, int64_t n_inst,
                                                                     const uint8_t *__restrict__ lists, uint64_t ld,
                                                                     uint64_t inst_stride, int32_t *__restrict__ out,
                                                                     const QbaMcCounts cv, uint32_t adv,
                                                                     const QbaNoiseProfile np) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // ProtoShared | box [2][G][box_ld] | acc
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(lds);
  uint32_t *box = lds + PROTO_S_WORDS;
  const int lane = threadIdx.x;
  const int G = n + 1, nq = 32 - __clz(n), w = 1 << nq;
  uint32_t *acc = box + ((proto_box_words(G, w) + 3) & ~3);
  uint32_t *mcw = acc + w * G;
  const int64_t inst = inst0 + blockIdx.x;
  const uint8_t *L = lists + (uint64_t)inst * inst_stride;
  const uint64_t key = seed_base + (uint64_t)inst;
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
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
      if (np.steps | np.depol) qba_nprof_d(qba_nprof_r(k, 0u, k0, k1, np), D, G, w);
      mc_entry_at<true>(acc, G, mcw, D, G, w, seen, bad);
    }
    mc_flags(mcw, G, w, seen, bad);
    proto_sync<true>();
    uint32_t st;
    const uint32_t pnz = mc_acc_finish<true>(S, acc, G, w, lane, st);
    proto_sync<true>();
    proto_rounds_adv<true>(S, box, n, n_dis, key, pnz, st, lane,
                           out + ((int64_t)j * n_inst + inst) * (int64_t)(4 + 5 * G), adv);
    lo = hi;
  }
}

// One thread per (instance, entry): it draws the entry's r once and walks the
// n + 1 rows, so a wavefront's bytes are consecutive along each row.  Columns
// >= count and the bytes between instances are never addressed.
// vmask = w - 1.
__global__ void qba_k_nprof_apply(int n, uint32_t vmask, uint64_t seed_base, int64_t n_inst, uint64_t count,
                                  uint8_t *__restrict__ lists, uint64_t ld, uint64_t inst_stride,
                                  const QbaNoiseProfile np) {
  const uint64_t total = (uint64_t)n_inst * count;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = t / count, e = t - i * count;
    const uint64_t key = seed_base + i;
    const uint64_t r = qba_nprof_r((uint32_t)e, (uint32_t)(e >> 32), (uint32_t)key, (uint32_t)(key >> 32), np);
    uint8_t *at = lists + i * inst_stride + e;
    for (int g = 0; g <= n; ++g) at[(uint64_t)g * ld] ^= (uint8_t)((uint32_t)(r >> (4 * g)) & vmask);
  }
}

}  // namespace

void qba_launch_nprof_lists(dim3 grid, size_t lds, hipStream_t stream, int n, int n_dis, uint64_t seed_base,
                            int64_t first, int64_t n_inst, const uint8_t *lists, uint64_t ld, uint64_t inst_stride,
                            int32_t *out, const QbaMcCounts &cv, uint32_t adv, const QbaNoiseProfile &np) {
  hipLaunchKernelGGL(qba_k_nprof_lists, grid, dim3(QBA_PROTO_BLOCK), lds, stream, n, n_dis, seed_base, first, n_inst,
                     lists, ld, inst_stride, out, cv, adv, np);
}

int qba_launch_nprof_apply(int n, uint64_t seed_base, int64_t n_inst, uint64_t count, const QbaNoiseProfile &np,
                           uint8_t *lists, uint64_t ld, uint64_t inst_stride, hipStream_t stream) {
  const uint64_t blocks = ((uint64_t)n_inst * count + QBA_BLOCK - 1) / QBA_BLOCK;
  const uint32_t vmask = (1u << qba_nq(n)) - 1u;
  hipLaunchKernelGGL(qba_k_nprof_apply, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(QBA_BLOCK), 0, stream,
                     n, vmask, seed_base, n_inst, count, lists, ld, inst_stride, np);
  QBA_HIP(hipGetLastError());
  return QBA_OK;
}
