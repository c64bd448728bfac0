// qba_proto_nettrace.hip -- a transcript of chosen Monte-Carlo runs on a
// network that loses packets: the C entry points
// qba_montecarlo_trace_sampled_net / _lists_net with their checks, and
// qba_k_nettrace_lists, which is qba_k_trace_lists (qba_proto_trace.hip)
// running proto_rounds_nettrace (qba_proto_nettrace.h).  The sampled form's
// kernel is qba_k_nettrace_sampled (qba_mc_nettrace_inst.hip).  Both are texts
// and code objects of their own; their names hold none of the substrings the
// descriptor tests collect the earlier kernels by.
#include <type_traits>

#include "qba_proto_nettrace.h"

namespace {

__global__ __launch_bounds__(QBA_PROTO_BLOCK) void qba_k_nettrace_lists(
    int n, int n_dis, uint64_t seed_base, int64_t j0, const int64_t *__restrict__ idx, int64_t n_idx,
    const int64_t *__restrict__ n_match, uint32_t count, const uint8_t *__restrict__ lists, uint64_t ld,
    uint64_t inst_stride, int32_t *__restrict__ rows, int32_t *__restrict__ counts, uint32_t *__restrict__ events,
    const QbaNoise nz, uint32_t adv, uint32_t cap, uint32_t net) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // ProtoShared | box [2][G][box_ld]
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(lds);
  uint32_t *box = lds + PROTO_S_WORDS;
  const int lane = threadIdx.x;
  const int G = n + 1, nq = 32 - __clz(n), w = 1 << nq;
  const int64_t j = j0 + blockIdx.x;
  int64_t lim = n_idx;
  if (n_match) {
    const int64_t m = *n_match;
    lim = m < lim ? (m < 0 ? 0 : m) : lim;
  }
  if (j >= lim) return;  // the whole (one-wavefront) workgroup
  const uint64_t key = seed_base + (uint64_t)idx[j];
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  const uint8_t *L = lists + (uint64_t)j * inst_stride;
  mc_begin(S, box, G, w, lane);
  proto_sync<true>();
  uint32_t seen = 0, bad = 0;
  for (uint32_t k = (uint32_t)lane; k < count; k += 64u) {
    uint32_t D[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int g = 0; g < QBA_PROTO_MAXG; ++g)
      if (g < G) D[g / 4] |= (uint32_t)L[(uint64_t)g * ld + k] << (8 * (g % 4));
    if (nz.steps) {  // qba_noise_d with G and w at run time
      const uint64_t r = qba_noise_r(k, 0u, k0, k1, nz);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        D[i] ^= qba_noise_spread((uint32_t)(r >> (16 * i)) & 0xFFFFu) & qba_noise_keep(G, w, i);
    }
    mc_entry<true>(S, box, D, G, w, seen, bad);
  }
  mc_flags(box, G, w, seen, bad);
  proto_sync<true>();
  uint32_t st;
  const uint32_t pnz = mc_finish<true>(S, box, G, w, lane, st);
  proto_sync<true>();
  // lane r <= n owns events[j][r][0 .. cap); the other lanes store nothing
  uint2 *ev = lane < G ? reinterpret_cast<uint2 *>(events) + (j * G + lane) * (int64_t)cap : nullptr;
  proto_rounds_nettrace<true>(S, box, n, n_dis, key, pnz, st, lane, rows + j * (int64_t)(4 + 5 * G), adv, net, ev, cap,
                              counts + j * G);
}

// f(std::integral_constant<int, n>()) for the n of a call
template <int K = 1, class F>
int with_n(int n, const F &f) {
  if constexpr (K > QBA_MAX_PARTIES) {
    return qba_fail(QBA_EUNSUPPORTED, "n_parties must be in [1, 15]");
  } else {
    if (n != K) return with_n<K + 1>(n, f);
    return f(std::integral_constant<int, K>());
  }
}

// The trace calls' checks in their order (qba_proto_trace.hip), with the
// network word right after adv.
int nettrace_check(const char *who, qba_ctx *ctx, int n, uint64_t count, uint32_t flip_q16, int n_dis, uint32_t adv,
                   uint32_t net, const int64_t *idx, int64_t n_idx, int64_t cap, const void *rows, const void *counts,
                   const void *events) {
  const char *bad = nullptr;
  if (n >= 1 && n <= QBA_MAX_PARTIES) {  // n_parties itself is qba_mc_check's first refusal
    if (count >> 31) bad = "count must be < 2^31";
    else if (flip_q16 > 65535u) bad = "flip_q16 must be <= 65535";
    else if (n_dis < 0 || n_dis > n) bad = "n_dishonest must be in [0, n_parties]";
    else if ((bad = qba_adv_bad(adv))) {}
    else if ((bad = qba_net_bad(net))) {}
    else if (n_idx < 0) bad = "n_idx < 0";
    else if (n_idx > 0 && !idx) bad = "idx is NULL";
    else if (cap < 1 || cap > QBA_TRACE_CAP_MAX) bad = "cap must be in [1, 4096]";
    else if (n_idx > 0 && (!rows || !counts || !events)) bad = "rows, counts or events is NULL";
  }
  return qba_mc_check(who, ctx, n, 0, bad, 0, nullptr);
}

}  // namespace

extern "C" int qba_montecarlo_trace_sampled_net(qba_ctx *ctx, int n, uint64_t seed_base, const int64_t *idx,
                                                int64_t n_idx, const int64_t *n_match, uint64_t count, int n_dis,
                                                uint32_t adv, uint32_t flip_q16, int64_t cap, int32_t *rows,
                                                int32_t *counts, uint32_t *events, qba_stream stream, uint32_t net) {
  const char *who = "qba_montecarlo_trace_sampled_net";
  if (int rc = nettrace_check(who, ctx, n, count, flip_q16, n_dis, adv, net, idx, n_idx, cap, rows, counts, events))
    return rc;
  if (!ctx->compiled[n][0] || !ctx->compiled[n][1])
    return qba_fail(QBA_ESTATE, std::string(who) + ": no resource program compiled for n=" + std::to_string(n) +
                                    " (call qba_resource_compile for both kinds)");
  if (n_idx == 0) return QBA_OK;
  if (int rc = qba_set_device(ctx)) return rc;
  QbaNetTrace T{{who,   (const QbaProgramSet *)ctx->prog_dev[n], seed_base, idx, n_idx, n_match, (uint32_t)count,
                 n_dis, adv, flip_q16 ? qba_noise_of(flip_q16) : QbaNoise{}, (uint32_t)cap, rows, counts, events,
                 (hipStream_t)stream},
                net};
  return with_n(n, [&](auto k) { return qba_launch_mc_nettrace<decltype(k)::value>(ctx, T); });
}

extern "C" int qba_montecarlo_trace_lists_net(qba_ctx *ctx, int n, uint64_t seed_base, const int64_t *idx,
                                              int64_t n_idx, const int64_t *n_match, uint64_t count, int n_dis,
                                              uint32_t adv, uint32_t flip_q16, int64_t cap, const uint8_t *lists,
                                              uint64_t ld, uint64_t inst_stride, int32_t *rows, int32_t *counts,
                                              uint32_t *events, qba_stream stream, uint32_t net) {
  const char *who = "qba_montecarlo_trace_lists_net";
  if (int rc = nettrace_check(who, ctx, n, count, flip_q16, n_dis, adv, net, idx, n_idx, cap, rows, counts, events))
    return rc;
  if (count && n_idx && (!lists || ld < count || (n_idx > 1 && inst_stride < (uint64_t)(n + 1) * ld)))
    return qba_fail(QBA_EINVAL, std::string(who) + ": need lists, ld >= the count and inst_stride >= (n+1)*ld");
  if (n_idx == 0) return QBA_OK;
  if (int rc = qba_set_device(ctx)) return rc;
  const int G = n + 1, w = 1 << qba_nq(n);
  const size_t lds = (size_t)(PROTO_S_WORDS + proto_box_words(G, w)) * sizeof(uint32_t);  // <= 34960 B
  const QbaNoise nz = flip_q16 ? qba_noise_of(flip_q16) : QbaNoise{};
  constexpr int64_t LAUNCH = 1 << 20;  // slots per launch
  for (int64_t first = 0; first < n_idx; first += LAUNCH) {
    const int64_t blocks = n_idx - first < LAUNCH ? n_idx - first : LAUNCH;
    hipLaunchKernelGGL(qba_k_nettrace_lists, dim3((unsigned)blocks), dim3(QBA_PROTO_BLOCK), lds, (hipStream_t)stream,
                       n, n_dis, seed_base, first, idx, n_idx, n_match, (uint32_t)count, lists, ld, inst_stride, rows,
                       counts, events, nz, adv, (uint32_t)cap, net);
    QBA_HIP(hipGetLastError());
  }
  return QBA_OK;
}
