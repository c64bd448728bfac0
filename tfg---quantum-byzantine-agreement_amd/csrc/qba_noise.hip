// qba_noise.hip -- qba_k_noise_apply: the flips of the noise model (qba_noise.h,
// DESIGN.md section 13.5) XORed in place into byte-layout lists, the masks the
// noisy fused Monte-Carlo kernels apply in registers.  A utility for callers
// who want the noisy lists themselves; not on the hot path.
#include "qba_noise.h"

// One thread per (instance, entry): it draws the entry's r once and walks the
// n + 1 rows, so a wavefront's bytes are consecutive along each row.  Columns
// >= count and the bytes between instances are never addressed.
// vmask = w - 1.
__global__ void qba_k_noise_apply(int n, uint32_t vmask, uint64_t seed_base, int64_t n_inst, uint64_t count,
                                  const QbaNoise nz, uint8_t *__restrict__ lists, uint64_t ld, uint64_t inst_stride) {
  const uint64_t total = (uint64_t)n_inst * count;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = t / count, e = t - i * count;
    const uint64_t key = seed_base + i;
    const uint64_t r = qba_noise_r((uint32_t)e, (uint32_t)(e >> 32), (uint32_t)key, (uint32_t)(key >> 32), nz);
    uint8_t *at = lists + i * inst_stride + e;
    for (int g = 0; g <= n; ++g) at[(uint64_t)g * ld] ^= (uint8_t)((uint32_t)(r >> (4 * g)) & vmask);
  }
}

int qba_launch_noise_apply(int n, uint64_t seed_base, int64_t n_inst, uint64_t count, uint32_t flip_q16,
                           uint8_t *lists, uint64_t ld, uint64_t inst_stride, hipStream_t stream) {
  const uint64_t blocks = ((uint64_t)n_inst * count + QBA_BLOCK - 1) / QBA_BLOCK;
  const uint32_t vmask = (1u << qba_nq(n)) - 1u;
  hipLaunchKernelGGL(qba_k_noise_apply, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(QBA_BLOCK), 0, stream,
                     n, vmask, seed_base, n_inst, count, qba_noise_of(flip_q16), lists, ld, inst_stride);
  QBA_HIP(hipGetLastError());
  return QBA_OK;
}
