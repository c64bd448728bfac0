// qba_exact.hip -- exact-order checks for bit-exact protocol parity, and the
// wire-compatible bit codec.
//
// The reference builds every party's tuple in its own set-iteration order
// (tfg.py:189, 291) and compares tuples position by position (tfg.py:97-98),
// so parity with it needs the host's index orders, not a canonical one.  The
// host keeps the Python sets; these kernels do the per-element work: the isQ
// and P-filter predicates of the compaction (qba_compact.h), gather,
// consistent, the packet check in its two launch shapes, check_gather and the
// codec.  The host-pointer forms (*_host) share one round trip, QbaTrip.
#include <string.h>

#include "qba_compact.h"

// workgroups of 256 threads over n items, at most cap
static unsigned qba_grid(uint64_t n, unsigned cap) { return (unsigned)std::min<uint64_t>((n + 255) / 256, cap); }

// --- isQCorrList = {k : Li[k] != Lc[k]}  (tfg.py:327) -------------------------------
struct QbaIsqPred {
  const uint8_t *l0, *l1;
  int64_t *out;
  __device__ bool test(int64_t i) const { return l0[i] != l1[i]; }
  __device__ void emit(int64_t i, int64_t pos) const { out[pos] = i; }
};

extern "C" int qba_isq_indices(qba_ctx *ctx, const uint8_t *li, const uint8_t *lc, uint64_t count,
                               int64_t *idx, int64_t cap, int64_t *count_host, qba_stream stream) {
  if (!ctx || !count_host || (count && (!li || !lc)) || (cap > 0 && !idx) || cap < 0)
    return qba_fail(QBA_EINVAL, "qba_isq_indices: bad arguments");
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  return qba_compact(ctx, QbaIsqPred{li, lc, idx}, (int64_t)count, cap, count_host,
                     (hipStream_t)stream);
}

// --- P = {x in isQCorr : Lc[x] == v}, isQCorr's iteration order kept (tfg.py:182) ------
// An index outside [0, lc_len) is never dereferenced: it flags the call,
// which then fails with QBA_EINVAL (the order comes through the public ABI).
// The flag is a plain store of 1 (every writer stores the same value), so
// `bad` may be the ctx's device flag or a word of the zero-copy staging.
struct QbaSelPred {
  const int64_t *order;
  const uint8_t *lc;
  uint64_t lc_len;
  int64_t v;
  int64_t *out;
  int64_t *bad;
  __device__ bool test(int64_t i) const {
    const int64_t x = order[i];
    if ((uint64_t)x >= lc_len) {
      *bad = 1;
      return false;
    }
    return (int64_t)lc[x] == v;
  }
  __device__ void emit(int64_t i, int64_t pos) const { out[pos] = order[i]; }
};

extern "C" int qba_select_eq(qba_ctx *ctx, const int64_t *order, int64_t m, const uint8_t *lc,
                             uint64_t lc_len, int64_t v, int64_t *out, int64_t *count_host,
                             qba_stream stream) {
  if (!ctx || !count_host || m < 0 || (m && (!order || !lc || !out)))
    return qba_fail(QBA_EINVAL, "qba_select_eq: bad arguments");
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  int64_t *flag = reinterpret_cast<int64_t *>(ctx->flag);  // 64 bytes allocated
  QBA_HIP(hipMemsetAsync(flag, 0, sizeof(int64_t), s));
  rc = qba_compact(ctx, QbaSelPred{order, lc, lc_len, v, out, flag}, m, m, count_host, s);
  if (rc) return rc;
  int64_t bad = 0;  // qba_compact has synchronised the stream
  QBA_HIP(hipMemcpy(&bad, flag, sizeof(int64_t), hipMemcpyDeviceToHost));
  if (bad) return qba_fail(QBA_EINVAL, "qba_select_eq: index outside Lc");
  return QBA_OK;
}

// --- the round trip of a host-pointer call (the protocol host's calls) ------------------
// nin int64 words go to the device and nout come back.  Small calls use the
// zero-copy staging, laid out [in | out]: the kernels read and write host
// memory themselves, with plain loads and stores, and nothing but the
// launches and one sync stands between the host and the answer.  Larger ones
// go through the pinned staging: pinned copy, one H2D, the launches, one D2H,
// a sync, a copy out.
struct QbaTrip {
  hipStream_t s;
  bool zc;
  size_t nin;
  int64_t *in_h, *out_h;  // host side; out_h holds the result after sync() only with zc
  int64_t *in_d, *out_d;  // what the kernels are given

  int open(qba_ctx *ctx, hipStream_t stream, size_t words_in, size_t words_out, bool may_zc) {
    s = stream, zc = may_zc, nin = words_in;
    const int rc = zc ? qba_ensure_zc(ctx, 8 * (nin + words_out))
                      : qba_ensure_staging(ctx, 8 * std::max(nin, words_out), 8 * (nin + words_out));
    if (rc) return rc;
    in_h = static_cast<int64_t *>(zc ? ctx->zc : ctx->pin_h);
    in_d = static_cast<int64_t *>(zc ? ctx->zc_d : ctx->pin_d);
    out_h = zc ? in_h + nin : in_h;
    out_d = in_d + nin;
    return QBA_OK;
  }
  int upload(const void *src) {
    if (!nin) return QBA_OK;
    memcpy(in_h, src, 8 * nin);
    if (!zc) QBA_HIP(hipMemcpyAsync(in_d, in_h, 8 * nin, hipMemcpyHostToDevice, s));
    return QBA_OK;
  }
  int sync() {
    QBA_HIP(hipStreamSynchronize(s));
    return QBA_OK;
  }
  // words [off, off + n) of the output to the caller's buffer; waits for the stream
  int download(void *dst, size_t n, size_t off = 0) {
    if (!zc) QBA_HIP(hipMemcpyAsync(out_h, out_d + off, 8 * n, hipMemcpyDeviceToHost, s));
    QBA_HIP(hipStreamSynchronize(s));
    memcpy(dst, zc ? out_h + off : out_h, 8 * n);
    return QBA_OK;
  }
};

// Up to QBA_CS_MAX items the two calls below are ONE qba_k_compact_small
// launch whose total, bad flag and output are words of the zero-copy staging
// (zeroed by the host); larger inputs go through the device compaction.
extern "C" int qba_isq_indices_host(qba_ctx *ctx, const uint8_t *li, const uint8_t *lc, uint64_t count,
                                    int64_t *idx_host, int64_t cap, int64_t *count_host, qba_stream stream) {
  if (!ctx || !count_host || (count && (!li || !lc)) || (cap > 0 && !idx_host) || cap < 0)
    return qba_fail(QBA_EINVAL, "qba_isq_indices_host: bad arguments");
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t keep = std::min<int64_t>(cap, (int64_t)count);
  QbaTrip t;  // out: [total | idx (keep)]
  if ((rc = t.open(ctx, s, 0, (size_t)keep + 1, count <= QBA_CS_MAX))) return rc;
  if (!t.zc) {
    if ((rc = qba_compact(ctx, QbaIsqPred{li, lc, t.out_d + 1}, (int64_t)count, keep, count_host, s))) return rc;
    return t.download(idx_host, (size_t)std::min<int64_t>(*count_host, keep), 1);
  }
  t.out_h[0] = 0;
  if (count) {
    hipLaunchKernelGGL(qba_k_compact_small<QbaIsqPred>, dim3(1), dim3(QBA_CS_THREADS), 0, s,
                       QbaIsqPred{li, lc, t.out_d + 1}, (int64_t)count, keep, t.out_d);
    QBA_HIP(hipGetLastError());
    if ((rc = t.sync())) return rc;
  }
  *count_host = t.out_h[0];
  memcpy(idx_host, t.out_h + 1, 8 * (size_t)std::min<int64_t>(t.out_h[0], keep));
  return QBA_OK;
}

extern "C" int qba_select_eq_host(qba_ctx *ctx, const int64_t *order_host, int64_t m, const uint8_t *lc,
                                  uint64_t lc_len, int64_t v, int64_t *out_host, int64_t *count_host,
                                  qba_stream stream) {
  if (!ctx || !count_host || m < 0 || (m && (!order_host || !lc || !out_host)))
    return qba_fail(QBA_EINVAL, "qba_select_eq_host: bad arguments");
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (m == 0) {
    *count_host = 0;
    return QBA_OK;
  }
  QbaTrip t;  // in: order (m); out: [total | bad | out (m)]
  if ((rc = t.open(ctx, s, (size_t)m, (size_t)m + 2, m <= QBA_CS_MAX)) || (rc = t.upload(order_host))) return rc;
  if (!t.zc) {
    if ((rc = qba_select_eq(ctx, t.in_d, m, lc, lc_len, v, t.out_d + 2, count_host, stream))) return rc;
    return t.download(out_host, (size_t)*count_host, 2);
  }
  t.out_h[0] = t.out_h[1] = 0;
  hipLaunchKernelGGL(qba_k_compact_small<QbaSelPred>, dim3(1), dim3(QBA_CS_THREADS), 0, s,
                     QbaSelPred{t.in_d, lc, lc_len, v, t.out_d + 2, t.out_d + 1}, m, m, t.out_d);
  QBA_HIP(hipGetLastError());
  if ((rc = t.sync())) return rc;
  if (t.out_h[1]) return qba_fail(QBA_EINVAL, "qba_select_eq_host: index outside Lc");
  *count_host = t.out_h[0];
  memcpy(out_host, t.out_h + 2, 8 * (size_t)t.out_h[0]);
  return QBA_OK;
}

// --- tuple(Li[j] for j in P)  (tfg.py:189, 291) --------------------------------------
__global__ void qba_k_gather(const uint8_t *__restrict__ li, const int64_t *__restrict__ idx,
                             int64_t m, int64_t *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = li[idx[i]];
}

// Indices must lie in [0, list_len): verified on the device first so a bad
// packet cannot make the gather read out of bounds.
__global__ void qba_k_bounds(const int64_t *__restrict__ idx, int64_t m, int64_t len,
                             int32_t *__restrict__ bad) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x)
    if (idx[i] < 0 || idx[i] >= len) atomicOr(bad, 1);
}

extern "C" int qba_gather(qba_ctx *ctx, const uint8_t *li, uint64_t list_len, const int64_t *idx,
                          int64_t m, int64_t *out, qba_stream stream) {
  if (!ctx || m < 0 || (m && (!li || !idx || !out)))
    return qba_fail(QBA_EINVAL, "qba_gather: bad arguments");
  if (m == 0) return QBA_OK;
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = qba_grid(m, 4096);
  QBA_HIP(hipMemsetAsync(ctx->flag, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(qba_k_bounds, dim3(grid), dim3(256), 0, s, idx, m, (int64_t)list_len, ctx->flag);
  int32_t bad = 0;
  QBA_HIP(hipMemcpyAsync(&bad, ctx->flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  QBA_HIP(hipStreamSynchronize(s));
  if (bad) return qba_fail(QBA_EINVAL, "qba_gather: index outside the list");
  hipLaunchKernelGGL(qba_k_gather, dim3(grid), dim3(256), 0, s, li, idx, m, out);
  QBA_HIP(hipGetLastError());
  return QBA_OK;
}

// --- consistent(v, L, w): Cond2 and Cond3 (tfg.py:93-98) ---------------------------
// The m values t[a * len + k] at position k are good when every one satisfies
// 0 <= x <= w and x != v (inclusive w, as the reference) and they are
// pairwise distinct.  each(a, x) sees every value visited.  STOP ends the
// walk at the first bad value, for a caller that wants the verdict alone; a
// caller that counts in `each` must see them all.
template <bool STOP, class Each>
__device__ __forceinline__ bool qba_received_good(const int64_t *__restrict__ t, int64_t m, int64_t len, int64_t k,
                                                  int64_t v, int64_t w, Each each) {
  bool good = true;
  for (int64_t a = 0; a < m && (good || !STOP); ++a) {
    const int64_t x = t[a * len + k];
    if (x < 0 || x > w || x == v) good = false;
    for (int64_t b = a + 1; b < m && good; ++b)
      if (t[b * len + k] == x) good = false;
    each(a, x);
  }
  return good;
}

// One thread per position k; any violation clears the flag.
__global__ void qba_k_consistent(const int64_t *__restrict__ t, int64_t m, int64_t len, int64_t v,
                                 int64_t w, int32_t *__restrict__ ok) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < len;
       k += (int64_t)gridDim.x * blockDim.x)
    if (!qba_received_good<true>(t, m, len, k, v, w, [](int64_t, int64_t) {})) atomicAnd(ok, 0);
}

extern "C" int qba_consistent(qba_ctx *ctx, const int64_t *tuples, int64_t m, int64_t len,
                              int64_t v, int64_t w, int32_t *ok_host, qba_stream stream) {
  if (!ctx || !ok_host || m < 1 || len < 0 || (len && !tuples))
    return qba_fail(QBA_EINVAL, "qba_consistent: bad arguments (m >= 1 required)");
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int32_t one = 1;
  QBA_HIP(hipMemcpyAsync(ctx->flag, &one, sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (len > 0) {
    hipLaunchKernelGGL(qba_k_consistent, dim3(qba_grid(len, 4096)), dim3(256), 0, s, tuples, m, len, v, w,
                       ctx->flag);
    QBA_HIP(hipGetLastError());
  }
  QBA_HIP(hipMemcpyAsync(ok_host, ctx->flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  QBA_HIP(hipStreamSynchronize(s));
  return QBA_OK;
}

// --- one packet of the exact-order protocol in ONE launch (tfg.py:189-192, 291-294) ---
// The receiving lieutenant gathers its own tuple Li[P] in its set-iteration
// order and evaluates consistent(v, L | {own}) (tfg.py:87-98) over the packet's
// m received tuples.  Cond1 (equal lengths) is the host's; here all tuples
// have length len.  L is a set, so own is dropped from the pairwise test when
// it equals a received tuple: per received tuple a, eq[a] counts positions k
// with t_a[k] == own[k], and a pair (a, own) violates Cond3 iff
// 0 < eq[a] < len.  stage: [order (len) | m received tuples (len each)].
// Output (int64): own[0..len), then 3 + m words, [len] bad index,
// [len+1] Cond2/3 violation among the received tuples, [len+2] Cond2
// violation of own, [len+3+a] eq[a].
//
// The work at position k: own[k] is stored, the rest goes to acc, which
// says where the 3 + m words accumulate: acc.flag(i) sets word i,
// acc.eq(a) adds one to word 3 + a.
template <class Acc>
__device__ __forceinline__ void qba_packet_at(const uint8_t *__restrict__ li, uint64_t list_len,
                                              const int64_t *__restrict__ stage, int64_t m, int64_t len, int64_t v,
                                              int64_t w, int64_t k, int64_t *__restrict__ out, Acc acc) {
  const int64_t j = stage[k];
  int64_t own = -1;
  if ((uint64_t)j >= list_len)
    acc.flag(0);
  else
    own = li[j];
  out[k] = own;
  if (own < 0 || own > w || own == v) acc.flag(2);
  if (!qba_received_good<false>(stage + len, m, len, k, v, w, [&](int64_t a, int64_t x) {
        if (x == own) acc.eq(a);
      }))
    acc.flag(1);
}

// Where a packet kernel accumulates is chosen by its launch shape, and the
// choice keeps one invariant: NO ATOMIC EVER TARGETS THE ZERO-COPY STAGING.
// It is host memory, and only plain stores go there.  The many-workgroup
// kernel's out is device memory (qba_check_packet's contract), so its words
// take 64-bit global atomics; the one-workgroup kernel, whose out is the
// staging, counts in LDS and stores the words once.
struct QbaAccGlobal {
  unsigned long long *words;  // out + len, device memory, zeroed by the host
  __device__ void flag(int i) const { atomicOr(&words[i], 1ull); }
  __device__ void eq(int64_t a) const { atomicAdd(&words[3 + a], 1ull); }
};
struct QbaAccLds {
  unsigned int *words;
  __device__ void flag(int i) const { atomicOr(&words[i], 1u); }
  __device__ void eq(int64_t a) const { atomicAdd(&words[3 + a], 1u); }
};

__global__ void qba_k_check_packet(const uint8_t *__restrict__ li, uint64_t list_len,
                                   const int64_t *__restrict__ stage, int64_t m, int64_t len, int64_t v,
                                   int64_t w, int64_t *__restrict__ out) {
  const QbaAccGlobal acc{reinterpret_cast<unsigned long long *>(out + len)};
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < len;
       k += (int64_t)gridDim.x * blockDim.x)
    qba_packet_at(li, list_len, stage, m, len, v, w, k, out, acc);
}

extern "C" int qba_check_packet(qba_ctx *ctx, const uint8_t *li, uint64_t list_len, const int64_t *stage,
                                int64_t m, int64_t len, int64_t v, int64_t w, int64_t *out,
                                qba_stream stream) {
  if (!ctx || !out || m < 0 || len < 0 || (len && (!li || !stage)))
    return qba_fail(QBA_EINVAL, "qba_check_packet: bad arguments");
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  QBA_HIP(hipMemsetAsync(out + len, 0, (size_t)(3 + m) * sizeof(int64_t), s));
  if (len > 0) {
    hipLaunchKernelGGL(qba_k_check_packet, dim3(qba_grid(len, 1024)), dim3(256), 0, s, li, list_len, stage, m, len,
                       v, w, out);
    QBA_HIP(hipGetLastError());
  }
  return QBA_OK;
}

// --- consistent(v, L, w) over tuples gathered from the device lists (SURVEY.md
// §8(b) qba_check_gather) ---------------------------------------------------------
// T_a[k] = lists[party[a]][idx[a][k]] for m index orders of length len (each
// tuple in its own order, as each lieutenant ships its own set-iteration
// order, tfg.py:189, 291).  L is a set (tfg.py:209, 240, 260), so identical
// tuples collapse: the pair (a, b) violates Cond3 iff 0 < eq(a, b) < len,
// eq = the number of positions where T_a and T_b agree.  cnt (scratch):
// [0] bad index/party, [1] Cond2 violation, [2 + pair] eq per pair a < b,
// each workgroup adding its LDS partial once.
#define QBA_GATHER_MAXM 64
__global__ void __launch_bounds__(256)
    qba_k_check_gather(const uint8_t *__restrict__ lists, uint64_t ld, int rows, uint64_t list_len,
                       const int64_t *__restrict__ idx, const int32_t *__restrict__ party, int64_t m,
                       int64_t len, int64_t v, int64_t w, unsigned long long *__restrict__ cnt) {
  __shared__ unsigned int eq[QBA_GATHER_MAXM * (QBA_GATHER_MAXM - 1) / 2];
  __shared__ unsigned int flags[2];
  const int np = (int)(m * (m - 1) / 2);
  for (int i = threadIdx.x; i < np; i += blockDim.x) eq[i] = 0u;
  if (threadIdx.x < 2) flags[threadIdx.x] = 0u;
  __syncthreads();
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < len;
       k += (int64_t)gridDim.x * blockDim.x) {
    // values re-read per pair (m is small; a runtime-indexed private array
    // would live in scratch)
    auto val = [&](int64_t a) -> int64_t {
      const int64_t j = idx[a * len + k];
      const int32_t r = party[a];
      if (r < 0 || r >= rows || (uint64_t)j >= list_len) return -1;
      return lists[(uint64_t)r * ld + (uint64_t)j];
    };
    int p = 0;
    for (int64_t a = 0; a < m; ++a) {
      const int64_t xa = val(a);
      if (xa < 0) atomicOr(&flags[0], 1u);
      if (xa < 0 || xa > w || xa == v) atomicOr(&flags[1], 1u);
      for (int64_t b = a + 1; b < m; ++b, ++p)
        if (xa == val(b)) atomicAdd(&eq[p], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < np; i += blockDim.x)
    if (eq[i]) atomicAdd(&cnt[2 + i], (unsigned long long)eq[i]);
  if (threadIdx.x < 2 && flags[threadIdx.x]) atomicOr(&cnt[threadIdx.x], 1ull);
}

__global__ void qba_k_check_gather_fin(const unsigned long long *__restrict__ cnt, int64_t m, int64_t len,
                                       int32_t *__restrict__ ok) {
  if (threadIdx.x != 0) return;
  int32_t r = 1;
  if (cnt[0]) {
    r = -1;
  } else if (cnt[1]) {
    r = 0;
  } else {
    const int64_t np = m * (m - 1) / 2;
    for (int64_t p = 0; p < np; ++p)
      if (cnt[2 + p] != 0ull && cnt[2 + p] != (unsigned long long)len) r = 0;
  }
  *ok = r;
}

extern "C" int qba_check_gather(qba_ctx *ctx, const uint8_t *lists, uint64_t ld, int rows, uint64_t list_len,
                                const int64_t *idx, const int32_t *party, int64_t m, int64_t len, int64_t v,
                                int64_t w, int32_t *ok, qba_stream stream) {
  if (!ctx || !ok || m < 1 || m > QBA_GATHER_MAXM || len < 0 || rows < 1 || ld < list_len ||
      (len && (!lists || !idx || !party)))
    return qba_fail(QBA_EINVAL, "qba_check_gather: bad arguments (1 <= m <= 64 tuples required; "
                                "an empty L is the reference's StopIteration, tfg.py:90)");
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  const size_t ncnt = 2 + (size_t)(m * (m - 1) / 2);
  if ((rc = qba_ensure_scan(ctx, ncnt * sizeof(unsigned long long)))) return rc;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long *cnt = static_cast<unsigned long long *>(ctx->scan);
  QBA_HIP(hipMemsetAsync(cnt, 0, ncnt * sizeof(unsigned long long), s));
  if (len > 0) {
    hipLaunchKernelGGL(qba_k_check_gather, dim3(qba_grid(len, 1024)), dim3(256), 0, s, lists, ld, rows, list_len, idx,
                       party, m, len, v, w, cnt);
    QBA_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(qba_k_check_gather_fin, dim3(1), dim3(64), 0, s, cnt, m, len, ok);
  QBA_HIP(hipGetLastError());
  return QBA_OK;
}

// The one-workgroup form; m <= QBA_GATHER_MAXM.
__global__ void __launch_bounds__(1024)
    qba_k_check_packet_zc(const uint8_t *__restrict__ li, uint64_t list_len, const int64_t *__restrict__ stage,
                          int64_t m, int64_t len, int64_t v, int64_t w, int64_t *__restrict__ out) {
  __shared__ unsigned int words[3 + QBA_GATHER_MAXM];
  if (threadIdx.x < 3 + QBA_GATHER_MAXM) words[threadIdx.x] = 0u;
  __syncthreads();
  for (int64_t k = threadIdx.x; k < len; k += blockDim.x)
    qba_packet_at(li, list_len, stage, m, len, v, w, k, out, QbaAccLds{words});
  __syncthreads();
  if (threadIdx.x < 3 + m) out[len + threadIdx.x] = words[threadIdx.x];
}

// int64 words of one packet's stage and of its output
static size_t packet_in(int64_t m, int64_t len) { return (size_t)len * (size_t)(m + 1); }
static size_t packet_out(int64_t m, int64_t len) { return (size_t)(len + 3 + m); }

// k packets, desc[i] = {m_i, len_i, v_i}, their stages concatenated in
// stage_host and their outputs in out_host, in one round trip.  When every
// packet has m <= QBA_GATHER_MAXM tuples and all of it fits QBA_ZC_MAX bytes,
// each packet is one workgroup working straight from and into the zero-copy
// staging; otherwise ONE H2D, one qba_check_packet per packet and ONE D2H.
static int check_packets(qba_ctx *ctx, const uint8_t *li, uint64_t list_len, const int64_t *stage_host,
                         const int64_t *desc, int64_t k, int64_t w, int64_t *out_host, qba_stream stream) {
  size_t nin = 0, nout = 0;
  bool small = true;
  for (int64_t i = 0; i < k; ++i) {
    nin += packet_in(desc[3 * i], desc[3 * i + 1]);
    nout += packet_out(desc[3 * i], desc[3 * i + 1]);
    small = small && desc[3 * i] <= QBA_GATHER_MAXM;
  }
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  QbaTrip t;
  if ((rc = t.open(ctx, s, nin, nout, small && 8 * (nin + nout) <= QBA_ZC_MAX)) || (rc = t.upload(stage_host)))
    return rc;
  size_t oi = 0, oo = 0;
  for (int64_t i = 0; i < k; ++i) {
    const int64_t m = desc[3 * i], len = desc[3 * i + 1], v = desc[3 * i + 2];
    if (!t.zc) {
      if ((rc = qba_check_packet(ctx, li, list_len, t.in_d + oi, m, len, v, w, t.out_d + oo, stream))) return rc;
    } else if (len > 0) {
      hipLaunchKernelGGL(qba_k_check_packet_zc, dim3(1), dim3(1024), 0, s, li, list_len, t.in_d + oi, m, len, v, w,
                         t.out_d + oo);
      QBA_HIP(hipGetLastError());
    } else {
      memset(t.out_h + oo, 0, 8 * packet_out(m, len));
    }
    oi += packet_in(m, len);
    oo += packet_out(m, len);
  }
  return t.download(out_host, nout);
}

// Synchronous host-pointer form (the protocol host's per-packet call).
extern "C" int qba_check_packet_host(qba_ctx *ctx, const uint8_t *li, uint64_t list_len,
                                     const int64_t *stage_host, int64_t m, int64_t len, int64_t v,
                                     int64_t w, int64_t *out_host, qba_stream stream) {
  if (!ctx || !out_host || m < 0 || len < 0 || (len && (!li || !stage_host)))
    return qba_fail(QBA_EINVAL, "qba_check_packet_host: bad arguments");
  const int64_t desc[3] = {m, len, v};
  return check_packets(ctx, li, list_len, stage_host, desc, 1, w, out_host, stream);
}

// A round's packets (tfg.py:337-348 -> 289-294): packet i's stage is
// [order | rows] of len_i * (m_i + 1) int64, its output len_i + 3 + m_i
// int64, as qba_check_packet.
extern "C" int qba_check_packets_host(qba_ctx *ctx, const uint8_t *li, uint64_t list_len,
                                      const int64_t *stage_host, const int64_t *desc, int64_t k, int64_t w,
                                      int64_t *out_host, qba_stream stream) {
  if (!ctx || !desc || !out_host || k < 1 || !stage_host)
    return qba_fail(QBA_EINVAL, "qba_check_packets_host: bad arguments");
  for (int64_t i = 0; i < k; ++i)
    if (desc[3 * i] < 0 || desc[3 * i + 1] < 0 || (desc[3 * i + 1] && !li))
      return qba_fail(QBA_EINVAL, "qba_check_packets_host: bad packet descriptor");
  return check_packets(ctx, li, list_len, stage_host, desc, k, w, out_host, stream);
}

// --- wire codec: rawS bits (one int64 per measured bit, MSB first) <-> values ---------
__global__ void qba_k_bits_to_values(const int64_t *__restrict__ raw, uint64_t count, int nq,
                                     uint8_t *__restrict__ vals) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count;
       k += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t v = 0;
    for (int j = 0; j < nq; ++j) v = (v << 1) | (uint32_t)(raw[k * nq + j] & 1);
    vals[k] = (uint8_t)v;
  }
}

__global__ void qba_k_values_to_bits(const uint8_t *__restrict__ vals, uint64_t count, int nq,
                                     int64_t *__restrict__ raw) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count * nq;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t k = i / nq;
    const int j = (int)(i - k * nq);
    raw[i] = (vals[k] >> (nq - 1 - j)) & 1;
  }
}

extern "C" int qba_bits_to_values(qba_ctx *ctx, const int64_t *raw, uint64_t count, int nq,
                                  uint8_t *vals, qba_stream stream) {
  if (!ctx || nq < 1 || nq > 8 || (count && (!raw || !vals)))
    return qba_fail(QBA_EINVAL, "qba_bits_to_values: bad arguments (1 <= nq <= 8)");
  if (count == 0) return QBA_OK;
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  hipLaunchKernelGGL(qba_k_bits_to_values, dim3(qba_grid(count, 8192)), dim3(256), 0, (hipStream_t)stream, raw,
                     count, nq, vals);
  QBA_HIP(hipGetLastError());
  return QBA_OK;
}

// rawS of a whole run (tfg.py:81-84): rows [0, rows) of a lists matrix (row
// stride ld) encoded and copied to raw_host[rows][count * nq]; synchronous.
extern "C" int qba_lists_to_bits_host(qba_ctx *ctx, const uint8_t *lists, uint64_t ld, int rows,
                                      uint64_t count, int nq, int64_t *raw_host, qba_stream stream) {
  if (!ctx || rows < 0 || nq < 1 || nq > 8 || (rows && count && (!lists || !raw_host)))
    return qba_fail(QBA_EINVAL, "qba_lists_to_bits_host: bad arguments");
  const size_t n = (size_t)rows * count * nq;
  if (n == 0) return QBA_OK;
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  QbaTrip t;
  if ((rc = t.open(ctx, s, 0, n, 8 * n <= QBA_ZC_MAX))) return rc;
  for (int g = 0; g < rows; ++g)
    hipLaunchKernelGGL(qba_k_values_to_bits, dim3(qba_grid(count * nq, 8192)), dim3(256), 0, s,
                       lists + (uint64_t)g * ld, count, nq, t.out_d + (size_t)g * count * nq);
  QBA_HIP(hipGetLastError());
  return t.download(raw_host, n);
}

// measure_to_ints of a received rawS row (tfg.py:158, 161) from host memory.
// Through the pinned staging the call is synchronous; through the zero-copy
// staging it returns after the launch, and the next user of that staging
// waits for the event recorded here (qba_ensure_zc).
extern "C" int qba_bits_to_values_host(qba_ctx *ctx, const int64_t *raw_host, uint64_t count, int nq,
                                       uint8_t *vals, qba_stream stream) {
  if (!ctx || nq < 1 || nq > 8 || (count && (!raw_host || !vals)))
    return qba_fail(QBA_EINVAL, "qba_bits_to_values_host: bad arguments (1 <= nq <= 8)");
  if (count == 0) return QBA_OK;
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  const size_t n = count * (size_t)nq;
  hipStream_t s = (hipStream_t)stream;
  QbaTrip t;
  if ((rc = t.open(ctx, s, n, 0, 8 * n <= QBA_ZC_MAX)) || (rc = t.upload(raw_host))) return rc;
  hipLaunchKernelGGL(qba_k_bits_to_values, dim3(qba_grid(count, 8192)), dim3(256), 0, s, t.in_d, count, nq, vals);
  QBA_HIP(hipGetLastError());
  if (!t.zc) return t.sync();
  if (!ctx->zc_ev) QBA_HIP(hipEventCreateWithFlags(&ctx->zc_ev, hipEventDisableTiming));
  QBA_HIP(hipEventRecord(ctx->zc_ev, s));
  ctx->zc_pending = true;
  return QBA_OK;
}

extern "C" int qba_values_to_bits(qba_ctx *ctx, const uint8_t *vals, uint64_t count, int nq,
                                  int64_t *raw, qba_stream stream) {
  if (!ctx || nq < 1 || nq > 8 || (count && (!raw || !vals)))
    return qba_fail(QBA_EINVAL, "qba_values_to_bits: bad arguments (1 <= nq <= 8)");
  if (count == 0) return QBA_OK;
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  hipLaunchKernelGGL(qba_k_values_to_bits, dim3(qba_grid(count * nq, 8192)), dim3(256), 0, (hipStream_t)stream, vals,
                     count, nq, raw);
  QBA_HIP(hipGetLastError());
  return QBA_OK;
}
