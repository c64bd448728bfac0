// qba_proto.hip -- the count-mode protocol rounds of many independent
// instances on the device, one wavefront (a 64-thread workgroup) per instance:
//   qba_protocol_batched   from the per-instance count tables of
//                          qba_sample_check_batched, exactly as
//                          countmode.CountParty does under protocol.run_local
//                          (barrier-epoch delivery, comm.py);
//   qba_montecarlo_lists   from injected byte rows, with no tables in between;
//   qba_montecarlo_curve_lists  the same at several counts in one pass.
// The rounds themselves are qba_proto_rounds.h (shared with the sampling
// kernel qba_k_mc_sampled); this file holds what feeds them.  DESIGN.md
// section 13.
//   qba_k_protocol's prologue: the int64 tables are read once, coalesced, and
//             distilled into LDS: P[u] != 0; per (u, g) the mask of x with
//             H[u][g][x] != 0, the mask of h with C[u][g][h] == 0 and
//             rep(u, g) = min h with C[u][g][h] == P[u]  (what
//             CountTables.desc / consistent consult)
//   qba_k_mc_lists: lane l distils entries l, l + 64, ... of the instance's
//             rows into the same masks (mc_entry, qba_proto_rounds.h)
#include "qba_proto_adv.h"  // the entry points' policy check and launches; the kernels here keep qba_proto_rounds.h
#include "qba_proto_coal.h"  // ... and the coalition word's check and launch
#include "qba_proto_net.h"   // ... and the network word's
#include "qba_noise_profile.h"  // ... and the noise profile's

namespace {

__global__ __launch_bounds__(QBA_PROTO_BLOCK) void qba_k_protocol(int n, int n_dis, uint64_t seed_base,
                                                                  int64_t inst0, const int64_t *__restrict__ Hd,
                                                                  const int64_t *__restrict__ Cd,
                                                                  const int64_t *__restrict__ Pd,
                                                                  int32_t *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t box[];  // [2][G][box_ld]; C flags in the prologue
  __shared__ ProtoShared S;
  const int lane = threadIdx.x;
  const int G = n + 1, nq = 32 - __clz(n), w = 1 << nq;  // nq = ceil(log2(n + 1)), tfg.py:317
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

  proto_rounds<true>(S, box, n, n_dis, seed_base + (uint64_t)inst, pnz, 0u, lane,
                     out + inst * (int64_t)(4 + 5 * G));
}

__global__ __launch_bounds__(QBA_PROTO_BLOCK) void qba_k_mc_lists(int n, int n_dis, uint64_t seed_base,
                                                                  int64_t inst0, uint32_t count,
                                                                  const uint8_t *__restrict__ lists, uint64_t ld,
                                                                  uint64_t inst_stride,
                                                                  int32_t *__restrict__ out) {
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
  proto_rounds<true>(S, box, n, n_dis, seed_base + (uint64_t)inst, pnz, st, lane,
                     out + inst * (int64_t)(4 + 5 * G));
}

// qba_k_mc_lists at the checkpoints cv.c[0] < cv.c[1] < ...: the running masks
// of the entries so far live in an accumulator area behind the mailbox
// (mc_acc_begin, qba_proto_rounds.h), which the rounds leave alone; row j is
// the row of qba_k_mc_lists at count cv.c[j].  A value >= w at a Q-correlated
// position sets the flag from its segment's checkpoint on.
__global__ __launch_bounds__(QBA_PROTO_BLOCK) void qba_k_mc_curve_lists(int n, int n_dis, uint64_t seed_base,
                                                                        int64_t inst0, int64_t n_inst,
                                                                        const uint8_t *__restrict__ lists,
                                                                        uint64_t ld, uint64_t inst_stride,
                                                                        int32_t *__restrict__ out,
                                                                        const QbaMcCounts cv) {
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
    proto_rounds<true>(S, box, n, n_dis, seed_base + (uint64_t)inst, pnz, st, lane,
                       out + ((int64_t)j * n_inst + inst) * (int64_t)(4 + 5 * G));
    lo = hi;
  }
}

}  // namespace


// The launches of a one-wave-per-instance kernel: launch(first, grid) starts
// instances [first, first + grid.x), at most 2^20 a time.
template <class F>
static int launch_chunks(qba_ctx *ctx, int64_t n_inst, const F &launch) {
  constexpr int64_t QBA_PROTO_LAUNCH = 1 << 20;  // instances per launch
  if (int rc = qba_set_device(ctx)) return rc;
  for (int64_t first = 0; first < n_inst; first += QBA_PROTO_LAUNCH) {
    const int64_t blocks = n_inst - first < QBA_PROTO_LAUNCH ? n_inst - first : QBA_PROTO_LAUNCH;
    launch(first, dim3((unsigned)blocks));
    QBA_HIP(hipGetLastError());
  }
  return QBA_OK;
}

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
  const int G = n + 1, w = 1 << qba_nq(n);
  const size_t lds = (size_t)proto_box_words(G, w) * sizeof(uint32_t);  // <= 32896 B at n = 15
  return launch_chunks(ctx, n_inst, [&](int64_t first, dim3 grid) {
    hipLaunchKernelGGL(qba_k_protocol, grid, dim3(QBA_PROTO_BLOCK), lds, (hipStream_t)stream, n, n_dis, seed_base,
                       first, H, C, P, out);
  });
}

// The argument envelope of the four Monte-Carlo calls (that of
// qba_protocol_batched with the count in the middle), in the order of
// rejection: n_parties, n_dishonest, `bad_count` (what is wrong with the count
// or the checkpoints; NULL: nothing), then ctx, n_instances and out.
int qba_mc_check(const char *who, qba_ctx *ctx, int n, int n_dis, const char *bad_count, int64_t n_inst,
                 const void *out) {
  const std::string f(who);
  if (n < 1 || n > QBA_MAX_PARTIES) return qba_fail(QBA_EINVAL, f + ": n_parties must be in [1, 15]");
  if (n_dis < 0 || n_dis > n) return qba_fail(QBA_EINVAL, f + ": n_dishonest must be in [0, n_parties]");
  if (bad_count) return qba_fail(QBA_EINVAL, f + ": " + bad_count);
  if (!ctx) return qba_fail(QBA_EINVAL, f + ": ctx is NULL");
  if (n_inst < 0) return qba_fail(QBA_EINVAL, f + ": n_instances < 0");
  if (n_inst > 0 && !out) return qba_fail(QBA_EINVAL, f + ": out is NULL");
  return QBA_OK;
}

static const char *bad_counts(const uint32_t *counts, int n_counts) {
  if (!counts) return "counts is NULL";
  if (n_counts < 1 || n_counts > QBA_MC_CURVE_MAX) return "n_counts must be in [1, 32]";
  for (int j = 1; j < n_counts; ++j)
    if (counts[j] <= counts[j - 1]) return "counts must be strictly increasing";
  return counts[n_counts - 1] >= (1u << 31) ? "counts must be < 2^31" : nullptr;
}

int qba_mc_curve_check(const char *who, qba_ctx *ctx, int n, int n_dis, int64_t n_inst, const uint32_t *counts,
                       int n_counts, const void *out, QbaMcCounts *cv, const char *bad_other) {
  const char *bad = bad_counts(counts, n_counts);
  if (int rc = qba_mc_check(who, ctx, n, n_dis, bad ? bad : bad_other, n_inst, out)) return rc;
  *cv = QbaMcCounts{};
  for (int j = 0; j < n_counts; ++j) cv->c[j] = counts[j];
  cv->n = n_counts;
  return QBA_OK;
}

int qba_mc_sweep_check(const char *who, qba_ctx *ctx, int n, int64_t n_inst, const uint32_t *counts, int n_counts,
                       const qba_mc_scenario *scen, int n_scen, const char *bad_flip, const void *out,
                       QbaMcCounts *cv, QbaMcScen *sv) {
  std::string at;  // "scenario i: what": the envelope reports the first bad scenario by its index
  const char *bad = bad_counts(counts, n_counts);
  if (!bad) bad = bad_flip;
  if (!bad) {
    if (!scen) bad = "scen is NULL";
    else if (n_scen < 1 || n_scen > QBA_MC_SWEEP_MAX) bad = "n_scen must be in [1, 16]";
    else if (n_counts * n_scen > QBA_MC_CURVE_MAX) bad = "n_counts * n_scen must be <= 32";
  }
  for (int s = 0; !bad && s < n_scen; ++s) {
    const char *b = scen[s].n_dishonest < 0 || scen[s].n_dishonest > n ? "n_dishonest must be in [0, n_parties]"
                                                                       : qba_adv_bad(scen[s].adv);
    if (!b) continue;
    at = "scenario " + std::to_string(s) + ": " + b;
    bad = at.c_str();
  }
  if (int rc = qba_mc_check(who, ctx, n, 0, bad, n_inst, out)) return rc;
  *cv = QbaMcCounts{};
  for (int j = 0; j < n_counts; ++j) cv->c[j] = counts[j];
  cv->n = n_counts;
  *sv = QbaMcScen{};
  for (int s = 0; s < n_scen; ++s) sv->s[s] = scen[s];
  sv->n = n_scen;
  return QBA_OK;
}

int qba_mc_grid_check(const char *who, qba_ctx *ctx, int n, int64_t n_inst, const uint32_t *counts, int n_counts,
                      const qba_mc_grid_scenario *scen, int n_scen, const char *bad_flip, const void *out,
                      QbaMcCounts *cv, QbaMcGrid *gv) {
  std::string at;  // "scenario i: what": the envelope reports the first bad scenario by its index
  const char *bad = bad_counts(counts, n_counts);
  if (!bad) bad = bad_flip;
  if (!bad) {
    if (!scen) bad = "scen is NULL";
    else if (n_scen < 1 || n_scen > QBA_MC_GRID_MAX) bad = "n_scen must be in [1, 16]";
    else if (n_counts * n_scen > QBA_MC_CURVE_MAX) bad = "n_counts * n_scen must be <= 32";
  }
  for (int s = 0; !bad && s < n_scen; ++s) {
    const char *b = scen[s].n_dishonest < 0 || scen[s].n_dishonest > n ? "n_dishonest must be in [0, n_parties]"
                                                                       : qba_adv_bad(scen[s].adv);
    if (!b) b = qba_net_bad(scen[s].net);
    if (!b) continue;
    at = "scenario " + std::to_string(s) + ": " + b;
    bad = at.c_str();
  }
  if (int rc = qba_mc_check(who, ctx, n, 0, bad, n_inst, out)) return rc;
  *cv = QbaMcCounts{};
  for (int j = 0; j < n_counts; ++j) cv->c[j] = counts[j];
  cv->n = n_counts;
  *gv = QbaMcGrid{};
  for (int s = 0; s < n_scen; ++s) gv->s[s] = scen[s];
  gv->n = n_scen;
  return QBA_OK;
}

// The injected rows of the two list calls hold `need` entries (the count, or
// the last checkpoint) per row without overlapping.
static int lists_check(const char *who, int n, int64_t n_inst, uint64_t need, const uint8_t *lists, uint64_t ld,
                       uint64_t inst_stride) {
  if (need && n_inst && (!lists || ld < need || (n_inst > 1 && inst_stride < (uint64_t)(n + 1) * ld)))
    return qba_fail(QBA_EINVAL,
                    std::string(who) + ": need lists, ld >= the (last) count and inst_stride >= (n+1)*ld");
  return QBA_OK;
}

extern "C" int qba_montecarlo_lists(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                    uint64_t count, const uint8_t *lists, uint64_t ld, uint64_t inst_stride,
                                    int32_t *out, qba_stream stream) {
  const char *who = "qba_montecarlo_lists";
  int rc = qba_mc_check(who, ctx, n, n_dis, count >> 31 ? "count must be < 2^31" : nullptr, n_inst, out);
  if (rc || (rc = lists_check(who, n, n_inst, count, lists, ld, inst_stride)) || n_inst == 0) return rc;
  const int G = n + 1, w = 1 << qba_nq(n);
  const size_t lds = (size_t)(PROTO_S_WORDS + proto_box_words(G, w)) * sizeof(uint32_t);  // <= 34960 B
  return launch_chunks(ctx, n_inst, [&](int64_t first, dim3 grid) {
    hipLaunchKernelGGL(qba_k_mc_lists, grid, dim3(QBA_PROTO_BLOCK), lds, (hipStream_t)stream, n, n_dis, seed_base,
                       first, (uint32_t)count, lists, ld, inst_stride, out);
  });
}

extern "C" int qba_montecarlo_curve_lists(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                          const uint32_t *counts, int n_counts, const uint8_t *lists, uint64_t ld,
                                          uint64_t inst_stride, int32_t *out, qba_stream stream) {
  const char *who = "qba_montecarlo_curve_lists";
  QbaMcCounts cv;
  int rc = qba_mc_curve_check(who, ctx, n, n_dis, n_inst, counts, n_counts, out, &cv);
  if (rc || (rc = lists_check(who, n, n_inst, cv.c[cv.n - 1], lists, ld, inst_stride)) || n_inst == 0) return rc;
  const int G = n + 1, w = 1 << qba_nq(n);
  const size_t lds = (size_t)(PROTO_S_WORDS + ((proto_box_words(G, w) + 3) & ~3) + mc_acc_words(G, w)) *
                     sizeof(uint32_t);  // <= 37024 B
  return launch_chunks(ctx, n_inst, [&](int64_t first, dim3 grid) {
    hipLaunchKernelGGL(qba_k_mc_curve_lists, grid, dim3(QBA_PROTO_BLOCK), lds, (hipStream_t)stream, n, n_dis,
                       seed_base, first, n_inst, lists, ld, inst_stride, out, cv);
  });
}

// ---------------------------------------------------------------------------
// The same three calls under an adversary policy word (qba_proto_adv.h,
// DESIGN.md section 13.7): the kernels of qba_proto_adv.hip.  The word is
// checked where the count is, before ctx is looked at.
// ---------------------------------------------------------------------------
extern "C" int qba_protocol_batched_adv(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                        const int64_t *H, const int64_t *C, const int64_t *P, int32_t *out,
                                        qba_stream stream, uint32_t adv) {
  const char *who = "qba_protocol_batched_adv";
  if (int rc = qba_mc_check(who, ctx, n, n_dis, qba_adv_bad(adv), n_inst, out)) return rc;
  if (n_inst == 0) return QBA_OK;
  if (!H || !C || !P) return qba_fail(QBA_EINVAL, std::string(who) + ": a table pointer is NULL");
  const int G = n + 1, w = 1 << qba_nq(n);
  const size_t lds = (size_t)(PROTO_S_WORDS + proto_box_words(G, w)) * sizeof(uint32_t);  // <= 34960 B
  return launch_chunks(ctx, n_inst, [&](int64_t first, dim3 grid) {
    qba_launch_protocol_adv(grid, lds, (hipStream_t)stream, n, n_dis, seed_base, first, H, C, P, out, adv);
  });
}

extern "C" int qba_montecarlo_lists_adv(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                        uint64_t count, const uint8_t *lists, uint64_t ld, uint64_t inst_stride,
                                        int32_t *out, qba_stream stream, uint32_t adv) {
  const char *who = "qba_montecarlo_lists_adv";
  int rc = qba_mc_check(who, ctx, n, n_dis, count >> 31 ? "count must be < 2^31" : qba_adv_bad(adv), n_inst, out);
  if (rc || (rc = lists_check(who, n, n_inst, count, lists, ld, inst_stride)) || n_inst == 0) return rc;
  const int G = n + 1, w = 1 << qba_nq(n);
  const size_t lds = (size_t)(PROTO_S_WORDS + proto_box_words(G, w)) * sizeof(uint32_t);  // <= 34960 B
  return launch_chunks(ctx, n_inst, [&](int64_t first, dim3 grid) {
    qba_launch_mc_lists_adv(grid, lds, (hipStream_t)stream, n, n_dis, seed_base, first, (uint32_t)count, lists, ld,
                            inst_stride, out, adv);
  });
}

extern "C" int qba_montecarlo_curve_lists_adv(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                              const uint32_t *counts, int n_counts, const uint8_t *lists,
                                              uint64_t ld, uint64_t inst_stride, int32_t *out, qba_stream stream,
                                              uint32_t adv) {
  const char *who = "qba_montecarlo_curve_lists_adv";
  QbaMcCounts cv;
  int rc = qba_mc_curve_check(who, ctx, n, n_dis, n_inst, counts, n_counts, out, &cv, qba_adv_bad(adv));
  if (rc || (rc = lists_check(who, n, n_inst, cv.c[cv.n - 1], lists, ld, inst_stride)) || n_inst == 0) return rc;
  const int G = n + 1, w = 1 << qba_nq(n);
  const size_t lds = (size_t)(PROTO_S_WORDS + ((proto_box_words(G, w) + 3) & ~3) + mc_acc_words(G, w)) *
                     sizeof(uint32_t);  // <= 37024 B
  return launch_chunks(ctx, n_inst, [&](int64_t first, dim3 grid) {
    qba_launch_mc_curve_lists_adv(grid, lds, (hipStream_t)stream, n, n_dis, seed_base, first, n_inst, lists, ld,
                                  inst_stride, out, cv, adv);
  });
}

// qba_montecarlo_curve_lists_adv with colluding traitors (DESIGN.md section
// 13.10): the kernel of qba_proto_coal.hip, whose hold lists sit behind the
// accumulator area.  The coalition word is checked right after the policy word.
extern "C" int qba_montecarlo_curve_lists_coal(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                               const uint32_t *counts, int n_counts, const uint8_t *lists,
                                               uint64_t ld, uint64_t inst_stride, int32_t *out, qba_stream stream,
                                               uint32_t adv, uint32_t coal) {
  const char *who = "qba_montecarlo_curve_lists_coal";
  QbaMcCounts cv;
  const char *bad = qba_adv_bad(adv);
  int rc = qba_mc_curve_check(who, ctx, n, n_dis, n_inst, counts, n_counts, out, &cv, bad ? bad : qba_coal_bad(coal));
  if (rc || (rc = lists_check(who, n, n_inst, cv.c[cv.n - 1], lists, ld, inst_stride)) || n_inst == 0) return rc;
  const int G = n + 1, w = 1 << qba_nq(n);
  const size_t lds = (size_t)(PROTO_S_WORDS + ((proto_box_words(G, w) + 3) & ~3) + ((mc_acc_words(G, w) + 3) & ~3) +
                              proto_hold_words(G, w)) * sizeof(uint32_t);  // <= 38064 B
  return launch_chunks(ctx, n_inst, [&](int64_t first, dim3 grid) {
    qba_launch_mc_coal_lists(grid, lds, (hipStream_t)stream, n, n_dis, seed_base, first, n_inst, lists, ld,
                             inst_stride, out, cv, adv, coal);
  });
}

// qba_montecarlo_curve_lists_adv on a network that loses packets (DESIGN.md
// section 13.11): the kernel of qba_proto_net.hip, in that call's LDS layout.
// The network word is checked right after the policy word.
extern "C" int qba_montecarlo_curve_lists_net(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                              const uint32_t *counts, int n_counts, const uint8_t *lists, uint64_t ld,
                                              uint64_t inst_stride, int32_t *out, qba_stream stream, uint32_t adv,
                                              uint32_t net) {
  const char *who = "qba_montecarlo_curve_lists_net";
  QbaMcCounts cv;
  const char *bad = qba_adv_bad(adv);
  int rc = qba_mc_curve_check(who, ctx, n, n_dis, n_inst, counts, n_counts, out, &cv, bad ? bad : qba_net_bad(net));
  if (rc || (rc = lists_check(who, n, n_inst, cv.c[cv.n - 1], lists, ld, inst_stride)) || n_inst == 0) return rc;
  const int G = n + 1, w = 1 << qba_nq(n);
  const size_t lds = (size_t)(PROTO_S_WORDS + ((proto_box_words(G, w) + 3) & ~3) + mc_acc_words(G, w)) *
                     sizeof(uint32_t);  // the _adv curve call's: <= 37024 B
  return launch_chunks(ctx, n_inst, [&](int64_t first, dim3 grid) {
    qba_launch_mc_net_lists(grid, lds, (hipStream_t)stream, n, n_dis, seed_base, first, n_inst, lists, ld,
                            inst_stride, out, cv, adv, net);
  });
}

// qba_montecarlo_curve_lists_adv under a noise profile (DESIGN.md section
// 13.14): the kernel of qba_proto_nprof.hip, in that call's LDS layout, which
// XORs the profile's masks into the rows it reads.  The profile is checked
// right after the policy word.
extern "C" int qba_montecarlo_curve_lists_nprof(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                                const uint32_t *counts, int n_counts, const uint8_t *lists,
                                                uint64_t ld, uint64_t inst_stride, int32_t *out, qba_stream stream,
                                                uint32_t adv, const uint16_t *rates, int n_rates,
                                                uint32_t depol_q16) {
  const char *who = "qba_montecarlo_curve_lists_nprof";
  QbaMcCounts cv;
  const char *bad = qba_adv_bad(adv);
  int rc = qba_mc_curve_check(who, ctx, n, n_dis, n_inst, counts, n_counts, out, &cv,
                              bad ? bad : qba_nprof_bad(n, rates, n_rates, depol_q16));
  if (rc || (rc = lists_check(who, n, n_inst, cv.c[cv.n - 1], lists, ld, inst_stride)) || n_inst == 0) return rc;
  const QbaNoiseProfile P = qba_nprof_of(rates, n_rates, depol_q16);
  const int G = n + 1, w = 1 << qba_nq(n);
  const size_t lds = (size_t)(PROTO_S_WORDS + ((proto_box_words(G, w) + 3) & ~3) + mc_acc_words(G, w)) *
                     sizeof(uint32_t);  // the _adv curve call's: <= 37024 B
  return launch_chunks(ctx, n_inst, [&](int64_t first, dim3 grid) {
    qba_launch_nprof_lists(grid, lds, (hipStream_t)stream, n, n_dis, seed_base, first, n_inst, lists, ld,
                           inst_stride, out, cv, adv, P);
  });
}

// qba_montecarlo_curve_lists_adv under every scenario of a list at every
// checkpoint: the kernel of qba_proto_sweep.hip.
extern "C" int qba_montecarlo_sweep_lists(qba_ctx *ctx, int n, uint64_t seed_base, int64_t n_inst,
                                          const uint32_t *counts, int n_counts, const qba_mc_scenario *scen,
                                          int n_scen, const uint8_t *lists, uint64_t ld, uint64_t inst_stride,
                                          int32_t *out, qba_stream stream) {
  const char *who = "qba_montecarlo_sweep_lists";
  QbaMcCounts cv;
  QbaMcScen sv;
  int rc = qba_mc_sweep_check(who, ctx, n, n_inst, counts, n_counts, scen, n_scen, nullptr, out, &cv, &sv);
  if (rc || (rc = lists_check(who, n, n_inst, cv.c[cv.n - 1], lists, ld, inst_stride)) || n_inst == 0) return rc;
  const int G = n + 1, w = 1 << qba_nq(n);
  const size_t lds = (size_t)(PROTO_S_WORDS + ((proto_box_words(G, w) + 3) & ~3) + mc_acc_words(G, w)) *
                     sizeof(uint32_t);  // <= 37024 B
  return launch_chunks(ctx, n_inst, [&](int64_t first, dim3 grid) {
    qba_launch_mc_sweep_lists(grid, lds, (hipStream_t)stream, n, seed_base, first, n_inst, lists, ld, inst_stride,
                              out, cv, sv);
  });
}

// qba_montecarlo_curve_lists_net under every scenario of a list at every
// checkpoint: the kernel of qba_proto_grid.hip, in
// that call's LDS layout.
extern "C" int qba_montecarlo_grid_lists(qba_ctx *ctx, int n, uint64_t seed_base, int64_t n_inst,
                                         const uint32_t *counts, int n_counts, const qba_mc_grid_scenario *scen,
                                         int n_scen, const uint8_t *lists, uint64_t ld, uint64_t inst_stride,
                                         int32_t *out, qba_stream stream) {
  const char *who = "qba_montecarlo_grid_lists";
  QbaMcCounts cv;
  QbaMcGrid gv;
  int rc = qba_mc_grid_check(who, ctx, n, n_inst, counts, n_counts, scen, n_scen, nullptr, out, &cv, &gv);
  if (rc || (rc = lists_check(who, n, n_inst, cv.c[cv.n - 1], lists, ld, inst_stride)) || n_inst == 0) return rc;
  const int G = n + 1, w = 1 << qba_nq(n);
  const size_t lds = (size_t)(PROTO_S_WORDS + ((proto_box_words(G, w) + 3) & ~3) + mc_acc_words(G, w)) *
                     sizeof(uint32_t);  // <= 37024 B
  return launch_chunks(ctx, n_inst, [&](int64_t first, dim3 grid) {
    qba_launch_grid_lists(grid, lds, (hipStream_t)stream, n, seed_base, first, n_inst, lists, ld, inst_stride, out,
                          cv, gv);
  });
}
