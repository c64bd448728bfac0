// qba_tally.hip -- qba_montecarlo_tally: the Monte-Carlo result rows of a
// batch reduced on the device to QBA_MC_TALLY_WORDS int64 per sizeL slice,
// with the global indices of selected (failed, empty-V_i, status) rows
// captured on the way.  A separate pass over the rows the decision kernels
// wrote (qba_proto.hip, qba_mc_kern.h): those stay as they are.  DESIGN.md
// section 13.3.
//   qba_k_mc_tally: one wavefront per workgroup, grid-stride over tiles of 64
//             rows, slices on blockIdx.y.  A tile is a contiguous word range:
//             it is loaded flat (lane l takes words l, l + 64, ...) into LDS
//             at an odd row stride, then lane l walks row l.  Partial tallies
//             stay in the lane's registers across tiles; one butterfly per
//             wavefront at the end, then lane j adds word j: at most one
//             global atomic per nonzero word and workgroup.  Capture slots
//             cost one more atomic per tile that holds a match.
#include <hip/hip_runtime.h>

#include "qba_internal.h"

#define QBA_TALLY_ROWS 64            // rows of a tile = lanes of the wavefront
#define QBA_TALLY_GRID 2048          // workgroups of a launch, over all slices
#define QBA_TALLY_LAUNCH (1 << 24)   // rows of a slice per launch: every wavefront sum but the three
                                     // field sums stays below 15 * 2^24 < 2^32

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
  return v;
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v |= (uint32_t)__shfl_xor((int)v, m, 64);
  return v;
}

__device__ __forceinline__ int64_t wave_sum64(int64_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (int64_t)__shfl_xor((long long)v, m, 64);
  return v;
}

__global__ __launch_bounds__(QBA_TALLY_ROWS) void qba_k_mc_tally(int n, const int32_t *__restrict__ rows,
                                                                 int64_t row0, int64_t n_rows, int64_t n_inst,
                                                                 uint64_t inst_base, int64_t *__restrict__ tally,
                                                                 int select, int64_t *__restrict__ capture,
                                                                 int64_t cap) {
  extern __shared__ __attribute__((aligned(16))) int32_t tile[];  // [QBA_TALLY_ROWS][S]
  const int lane = threadIdx.x;
  const int W = 4 + 5 * (n + 1);
  const int S = W | 1;  // odd: lanes l and l + k, k < 32, walk different banks
  const int pad = S - W;
  const int step_r = QBA_TALLY_ROWS / W, step_c = QBA_TALLY_ROWS % W;  // what 64 words advance (row, column) by
  const int64_t slice = blockIdx.y;
  const int32_t *src = rows + (slice * n_inst + row0) * (int64_t)W;
  unsigned long long *T = reinterpret_cast<unsigned long long *>(tally + slice * QBA_MC_TALLY_WORDS);
  const int64_t n_tiles = (n_rows + QBA_TALLY_ROWS - 1) / QBA_TALLY_ROWS;

  uint32_t c_runs = 0, c_ok = 0, c_empty = 0, c_status = 0, c_or = 0, c_cmd = 0, c_cmd_ok = 0, c_neg = 0;
  uint32_t bin[16] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  int64_t s_accept = 0, s_reject = 0, s_sent = 0;

  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t first = t * QBA_TALLY_ROWS;
    const int nr = (int)(n_rows - first < QBA_TALLY_ROWS ? n_rows - first : QBA_TALLY_ROWS);
    const int nw = nr * W;
    const int32_t *g = src + first * W;
    __syncthreads();  // the previous tile has been walked
    {
      int r = lane / W, c = lane % W;  // of word `at`
      for (int at = lane; at < nw; at += 4 * QBA_TALLY_ROWS) {
        int32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = at + k * QBA_TALLY_ROWS < nw ? g[at + k * QBA_TALLY_ROWS] : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int a = at + k * QBA_TALLY_ROWS;
          if (a < nw) tile[a + pad * r] = v[k];
          r += step_r;
          c += step_c;
          if (c >= W) {
            c -= W;
            ++r;
          }
        }
      }
    }
    __syncthreads();

    const bool have = lane < nr;
    const int32_t *p = tile + lane * S;
    const int32_t st = have ? p[3] : 0;
    const bool live = have && st == 0;  // a status row counts in words 0, 3 and 4 only
    const bool ok = live && p[0] != 0;
    const uint32_t dis = live ? (uint32_t)p[1] : 0u;
    const bool empty = live && p[2] != 0;
    c_runs += have;
    c_status += have && st != 0;
    c_or |= (uint32_t)st;
    c_ok += ok;
    c_empty += empty;
    c_cmd += (dis >> 1) & 1u;
    c_cmd_ok += ((dis >> 1) & 1u) & (uint32_t)ok;
    if (live) {
      uint64_t nib = 0;  // 16 four-bit counters: a row adds at most n <= 15 to one of them
#pragma unroll
      for (int r = 1; r <= QBA_MAX_PARTIES; ++r) {
        if (r <= n) {
          const int32_t *q = p + 4 + 5 * r;
          s_accept += q[2];
          s_reject += q[3];
          s_sent += q[4];
          const int32_t d = q[0];
          if (!((dis >> r) & 1u)) {
            c_neg += d == -1;
            if ((uint32_t)d < 16u) nib += 1ull << (4 * d);
          }
        }
      }
#pragma unroll
      for (int v = 0; v < 16; ++v) bin[v] += (uint32_t)(nib >> (4 * v)) & 15u;
    }

    if (select) {
      const bool match = have && (st != 0 ? (select & QBA_MC_SEL_STATUS) != 0
                                          : ((select & QBA_MC_SEL_FAILED) && !ok) ||
                                                ((select & QBA_MC_SEL_EMPTY_VI) && empty));
      const unsigned long long who = __ballot(match);
      if (who) {  // one atomic for the tile; the lanes share out the slots it reserves
        unsigned long long base = 0;
        if (lane == __ffsll(who) - 1) base = atomicAdd(&T[10], (unsigned long long)__popcll(who));
        base = (unsigned long long)__shfl((long long)base, __ffsll(who) - 1, 64);
        const unsigned long long slot = base + (unsigned long long)__popcll(who & ((1ull << lane) - 1ull));
        if (match && slot < (unsigned long long)cap)
          capture[slice * cap + (int64_t)slot] = (int64_t)(inst_base + (uint64_t)(row0 + first + lane));
      }
    }
  }

  // every lane ends with the wavefront's totals; lane j keeps word j
  unsigned long long mine = 0;
#define QBA_TALLY_WORD(j, val)                       \
  {                                                  \
    const unsigned long long x_ = (val);             \
    if (lane == (j)) mine = x_;                      \
  }
  QBA_TALLY_WORD(0, wave_sum(c_runs))
  QBA_TALLY_WORD(1, wave_sum(c_ok))
  QBA_TALLY_WORD(2, wave_sum(c_empty))
  QBA_TALLY_WORD(3, wave_sum(c_status))
  QBA_TALLY_WORD(4, wave_or(c_or))
  QBA_TALLY_WORD(5, wave_sum(c_cmd))
  QBA_TALLY_WORD(6, wave_sum(c_cmd_ok))
  QBA_TALLY_WORD(7, (unsigned long long)wave_sum64(s_accept))
  QBA_TALLY_WORD(8, (unsigned long long)wave_sum64(s_reject))
  QBA_TALLY_WORD(9, (unsigned long long)wave_sum64(s_sent))
  QBA_TALLY_WORD(15, wave_sum(c_neg))
#pragma unroll
  for (int v = 0; v < 16; ++v) QBA_TALLY_WORD(16 + v, wave_sum(bin[v]))
#undef QBA_TALLY_WORD
  if (lane < QBA_MC_TALLY_WORDS && mine) {
    if (lane == 4)
      atomicOr(&T[4], mine);
    else
      atomicAdd(&T[lane], mine);  // lanes 10..14 hold 0: word 10 moves with the slots, 11..14 never
  }
}

}  // namespace

extern "C" int qba_montecarlo_tally(qba_ctx *ctx, int n, const int32_t *rows, int64_t n_inst, int n_slices,
                                    uint64_t inst_base, int64_t *tally, int select, int64_t *capture,
                                    int64_t capture_cap, qba_stream stream) {
  const std::string f("qba_montecarlo_tally");
  if (n < 1 || n > QBA_MAX_PARTIES) return qba_fail(QBA_EINVAL, f + ": n_parties must be in [1, 15]");
  if (n_slices < 1 || n_slices > QBA_MC_CURVE_MAX) return qba_fail(QBA_EINVAL, f + ": n_slices must be in [1, 32]");
  if (n_inst < 0) return qba_fail(QBA_EINVAL, f + ": n_instances < 0");
  if (select < 0 || select > 7) return qba_fail(QBA_EINVAL, f + ": select must be in [0, 7]");
  if (capture_cap < 0) return qba_fail(QBA_EINVAL, f + ": capture_cap < 0");
  if (!tally) return qba_fail(QBA_EINVAL, f + ": tally_dev is NULL");
  if (n_inst > 0 && !rows) return qba_fail(QBA_EINVAL, f + ": rows_dev is NULL");
  if (select != 0 && capture_cap > 0 && !capture) return qba_fail(QBA_EINVAL, f + ": capture_dev is NULL");
  if (!ctx) return qba_fail(QBA_EINVAL, f + ": ctx is NULL");
  if (n_inst == 0) return QBA_OK;
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  const int W = 4 + 5 * (n + 1);
  const size_t lds = (size_t)QBA_TALLY_ROWS * (W | 1) * sizeof(int32_t);  // <= 21760 B at n = 15
  const int64_t per_slice = QBA_TALLY_GRID / n_slices;                    // >= 64
  for (int64_t first = 0; first < n_inst; first += QBA_TALLY_LAUNCH) {
    const int64_t n_rows = n_inst - first < QBA_TALLY_LAUNCH ? n_inst - first : QBA_TALLY_LAUNCH;
    const int64_t tiles = qba_ceil_div(n_rows, QBA_TALLY_ROWS);
    const int64_t gx = tiles < per_slice ? tiles : per_slice;
    hipLaunchKernelGGL(qba_k_mc_tally, dim3((unsigned)gx, (unsigned)n_slices), dim3(QBA_TALLY_ROWS), lds,
                       (hipStream_t)stream, n, rows, first, n_rows, n_inst, inst_base, tally, select, capture,
                       capture_cap);
    QBA_HIP(hipGetLastError());
  }
  return QBA_OK;
}
