// qba_lists_launch.h -- host side of the list kernels (no device code): which
// kernel of qba_lists_kern.h a call runs, with how much LDS and on what grid
// (the plan), and the launch itself -- synchronous with its reduce, deferred,
// or split into pair-bin parts.  Included after the kernels by
// qba_lists_inst.hip, once per n.
#pragma once
#include "qba_lists_kern.h"

// Persistent grid: every resident workgroup slot of the chip (LDS- and
// register-limited occupancy), fewer when the launch has less work.
static int grid_for(qba_ctx *ctx, const void *kern, size_t lds, uint64_t count, int qpt, int *cap_out, int bs) {
  // the occupancy query costs tens of microseconds: cached per (kernel, LDS)
  struct Occ { const void *k; size_t lds; int per_cu; };
  static thread_local Occ cache[16] = {};
  static thread_local int next = 0;
  int per_cu = 0;
  for (const Occ &o : cache)
    if (o.k == kern && o.lds == lds) per_cu = o.per_cu;
  if (per_cu == 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, bs, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    cache[next] = Occ{kern, lds, per_cu};
    next = (next + 1) % 16;
  }
  const uint64_t nquad = (count + 3) >> 2;
  // >= 2 quads (one wide thread-step) per thread: a small launch (configs[1],
  // 1e6 entries) spreads over 163 workgroups instead of 82
  uint64_t g = (nquad + (uint64_t)qpt * bs - 1) / ((uint64_t)qpt * bs);
  const uint64_t cap = (uint64_t)ctx->num_cus * (uint64_t)per_cu;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  *cap_out = (int)cap;
  return (int)g;
}

// qba_flush_deferred / qba_flush_pending: the pending call's reduction alone.
template <int NP>
static int qba_flush_def(qba_ctx *ctx) {
  const auto &p = ctx->pend;
  const QbaDefer d{p.slab, p.rows, 0, p.acc, p.sacc, p.H, p.C, p.P, p.stats};
  hipLaunchKernelGGL(qba_k_reduce_def<NP>, dim3(qba_def_wgs<NP>()), dim3(QBA_LBLOCK), qba_reduce_lds<NP>(QBA_LBLOCK),
                     p.stream, d);
  QBA_HIP(hipGetLastError());
  return QBA_OK;
}

// Sampler of the compiled pair: closed form when proven (n <= 11), else the
// canonical-table fast path, else the general alias-table path.
template <int NP>
static int sampler_of(const QbaProgramSet *hs) {
  if (NP <= QBA_CLOSED_MAX_N && hs->closed) return QBA_S_CLOSED;
  return hs->canonical ? QBA_S_FAST : QBA_S_GENERAL;
}

// LDS bytes of the staged tables for a sampling launch (the layout of qba_stage)
template <int NP>
static size_t table_lds(const QbaProgramSet *hs, int samp) {
  if (samp == QBA_S_CLOSED) return (size_t)((CF<NP>::WORDS + 3) & ~3) * sizeof(uint32_t);
  return (size_t)(((hs->any_nonuniform ? 3 : 1) * hs->table_total + 1) & ~1) * sizeof(uint64_t);
}

template <int NP>
static int check_closed(const QbaProgramSet *hs) {
  if (hs->closed && (hs->ra != CF<NP>::RA || hs->rb != CF<NP>::RB || hs->rc != CF<NP>::RC || hs->t32 != CF<NP>::T32 ||
                     hs->perm_words != CF<NP>::WORDS || hs->perm_off != (int32_t)QBA_PERM_OFF))
    return qba_fail(QBA_EINVAL, "closed-form program does not match the kernel's stage layout");
  return QBA_OK;
}

// Kernel picker.  A thread-step takes QPT quads of every row as one vector:
// 8 B of a byte row (QBA_WIDE_QPT quads), one 4-B word of a nibble row (2
// quads), when base and stride have that alignment ("wide"); one quad
// otherwise.  (The one-quad step on twice the workgroups for small launches
// shortens the list kernel -- 8.8 vs 10.1 us at 1e6 entries -- but its
// workgroups then share CUs with the deferred reduction's: 11.7 vs 10.3 us
// per configs[1] step, profiles/r3/r3m, r3n; rejected, tools/exp/rejected.)
constexpr int QBA_NIBBLE_QPT = 2;  // quads per thread-step of the wide kernels on nibble rows

static bool rows_wide(bool packed, const uint8_t *lists, uint64_t ld, uint64_t inst_stride = 0) {
  const uintptr_t va = packed ? 3 : 4 * QBA_WIDE_QPT - 1;  // row vectors need their natural alignment
  return !(reinterpret_cast<uintptr_t>(lists) & va) && !(ld & va) && !(inst_stride & va);
}

// Quads per thread a launch's grid is sized for: one thread-step of the
// picked kernel on nibble and unaligned rows, QBA_GRID_QPT (the measured grid
// of the 8-B step, not its QBA_WIDE_QPT) on aligned byte rows.
static constexpr int quads_per_thread(bool packed, bool wide) {
  return !wide ? 1 : packed ? QBA_NIBBLE_QPT : QBA_GRID_QPT;
}

// A kernel family F names its kernel of a step shape as F::at<QPT, PK>() (PK
// 1: nibble rows); the rule (packed, wide) -> (QPT, PK) is this function.
template <class F>
static const void *pick_kernel(bool packed, bool wide) {
  if (packed) return wide ? F::template at<QBA_NIBBLE_QPT, 1>() : F::template at<1, 1>();
  return wide ? F::template at<QBA_WIDE_QPT, 0>() : F::template at<1, 0>();
}

template <int NP, int M, int S, int CNT = 0>
struct QbaKLists {  // null: pair bins (CNT 1) on a step shape that has none (the check of byte rows)
  template <int QPT, int PK>
  static const void *at() {
    if constexpr (!CNT || QbaUsePB<NP, M, S, PK>::value) return (const void *)qba_k_lists<NP, M, S, QPT, PK, CNT>;
    return nullptr;
  }
};
template <int NP, int S>
struct QbaKDef {
  template <int QPT, int PK>
  static const void *at() { return (const void *)qba_k_lists_def<NP, S, QPT, PK>; }
};
template <int NP>
struct QbaKPbDef {
  template <int QPT, int PK>
  static const void *at() { return (const void *)qba_k_lists_pbdef<NP, QPT, PK>; }
};
// NOISE: the family's kernels take B.noise after the common arguments
template <int NP, int S>
struct QbaKBatched {
  static constexpr bool NOISE = false;
  template <int QPT, int PK>
  static const void *at() { return (const void *)qba_k_batched<NP, S, QPT, PK>; }
};
// No one-quad kernel on nibble rows: the batched calls refuse rows that are
// not 4-byte aligned, which is all rows_wide asks of nibble rows, so that step
// shape is never picked (qba_k_batched<NP, S, 1, 1> is as unreachable; it stays,
// being part of the code objects that must not change).
template <int NP, int S>
struct QbaKBatchedNoisy {
  static constexpr bool NOISE = true;
  template <int QPT, int PK>
  static const void *at() {
    if constexpr (QPT == 1 && PK == 1) return nullptr;
    else return (const void *)qba_k_batched_noisy<NP, S, QPT, PK>;
  }
};

// The kernel of a synchronous launch; null: a closed-form program beyond n = 11.
template <int NP>
static const void *lists_kernel(int mode, int samp, bool pb, bool packed, bool wide) {
  if (mode == 2) {
    const void *k = pick_kernel<QbaKLists<NP, 2, QBA_S_GENERAL>>(packed, wide);
    if constexpr (QbaUsePB<NP, 2, QBA_S_GENERAL, 1>::value)
      if (pb) k = pick_kernel<QbaKLists<NP, 2, QBA_S_GENERAL, 1>>(packed, wide);
    return k;
  }
  if (samp == QBA_S_CLOSED) {
    if constexpr (NP <= QBA_CLOSED_MAX_N) {
      const void *k = mode == 0 ? pick_kernel<QbaKLists<NP, 0, QBA_S_CLOSED>>(packed, wide)
                                : pick_kernel<QbaKLists<NP, 1, QBA_S_CLOSED>>(packed, wide);
      if constexpr (QbaUsePB<NP, 1, QBA_S_CLOSED, 0>::value)
        if (pb) k = pick_kernel<QbaKLists<NP, 1, QBA_S_CLOSED, 1>>(packed, wide);
      return k;
    }
    return nullptr;
  }
  if (samp == QBA_S_FAST)
    return mode == 0 ? pick_kernel<QbaKLists<NP, 0, QBA_S_FAST>>(packed, wide)
                     : pick_kernel<QbaKLists<NP, 1, QBA_S_FAST>>(packed, wide);
  return mode == 0 ? pick_kernel<QbaKLists<NP, 0, QBA_S_GENERAL>>(packed, wide)
                   : pick_kernel<QbaKLists<NP, 1, QBA_S_GENERAL>>(packed, wide);
}

// F<NP, S>'s kernel for the sampler; null: a closed-form program beyond n = 11
// (the other n have no closed-form kernels).
template <int NP, template <int, int> class F>
static const void *pick_sampler(int samp, bool packed, bool wide) {
  if (samp == QBA_S_CLOSED) {
    if constexpr (NP <= QBA_CLOSED_MAX_N) return pick_kernel<F<NP, QBA_S_CLOSED>>(packed, wide);
    return nullptr;
  }
  return samp == QBA_S_FAST ? pick_kernel<F<NP, QBA_S_FAST>>(packed, wide)
                            : pick_kernel<F<NP, QBA_S_GENERAL>>(packed, wide);
}

// The kernel of a deferred sample + check: a pair-bin launch defers into its
// own tail (qba_k_lists_pbdef), the others into qba_k_lists_def.
template <int NP>
static const void *deferred_kernel(int samp, bool pb, bool packed, bool wide) {
  if constexpr (QbaUsePB<NP, 1, QBA_S_CLOSED, 0>::value)
    if (pb) return pick_kernel<QbaKPbDef<NP>>(packed, wide);
  return pb ? nullptr : pick_sampler<NP, QbaKDef>(samp, packed, wide);
}

// The plan of one launch, filled once by plan_lists and only read after it
struct QbaShape {
  const void *kern = nullptr;
  size_t lds = 0;                    // dynamic LDS bytes
  int block = 0, grid = 0, cap = 0;  // threads per workgroup, list workgroups, the chip's resident slots for them
};
struct QbaPlan {
  int samp = QBA_S_GENERAL;
  bool pb = false, wide = false;  // counts with pair bins (QbaPB); rows_wide
  uint64_t pb_part = 0;           // pair bins: entries one launch may take (launch_parts splits a longer call)
  QbaShape sync;                  // qba_k_lists, then qba_k_reduce
  QbaShape def;                   // kern set: the reduction is deferred (qba_k_lists_def / qba_k_lists_pbdef)
};

static size_t lds_round(size_t lds) { return (lds + 15) & ~(size_t)15; }
static int lds_allow(const void *kern, size_t lds) {  // beyond the 64 KiB a kernel gets unasked
  if (lds > 65536) QBA_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return QBA_OK;
}

// Deferred reduction: the list kernel also reduces the pending deferred call
// (qba_def_wgs workgroups after its own) when both fit the chip's resident
// slots together; otherwise (def.kern stays null) the pending one is flushed
// and this call is reduced at once: its results are simply complete earlier.
template <int NP>
static int plan_deferred(qba_ctx *ctx, const QbaLaunch &L, size_t tables, QbaPlan &P) {
  QbaShape D = P.sync;
  D.kern = deferred_kernel<NP>(P.samp, P.pb, L.packed, P.wide);
  if (!D.kern) return QBA_OK;
  if (P.pb) {  // the list kernel's own launch shape; its LDS covers a reduce workgroup's scratch
    if (D.lds < qba_reduce_lds<NP>(QBA_LBLOCK)) D.lds = qba_reduce_lds<NP>(QBA_LBLOCK);
    if (int rc = lds_allow(D.kern, D.lds)) return rc;
  } else {
    // QBA_DBLOCK-thread workgroups (small launches: more, shorter workgroups;
    // 9.6 vs 10.5 us per configs[1] pass)
    D.block = QBA_DBLOCK;
    D.lds = tables + qba_count_lds<NP>(QBA_DBLOCK);
    D.lds = lds_round(D.lds < qba_reduce_lds<NP>(QBA_DBLOCK) ? qba_reduce_lds<NP>(QBA_DBLOCK) : D.lds);
    if (int rc = lds_allow(D.kern, D.lds)) return rc;
    D.grid = grid_for(ctx, D.kern, D.lds, L.count, quads_per_thread(L.packed, P.wide), &D.cap, QBA_DBLOCK);
    // a launch that would leave CUs idle spreads its units over one workgroup
    // per CU (wave-major units, qba_lists_body): the LDS work of its counting
    // is what bounds it (configs[1]: 163 -> 256 workgroups)
    if (D.grid < ctx->num_cus && ctx->num_cus + qba_def_wgs<NP>() <= D.cap) D.grid = ctx->num_cus;
    if (D.grid + qba_def_wgs<NP>() > D.cap) return QBA_OK;
  }
  P.def = D;
  return QBA_OK;
}

template <int NP>
static int plan_lists(qba_ctx *ctx, const QbaLaunch &L, QbaPlan &P) {
  const QbaProgramSet *hs = reinterpret_cast<const QbaProgramSet *>(ctx->prog_host[NP]);
  size_t tables = 0;
  if (L.mode != 2) {
    P.samp = sampler_of<NP>(hs);
    if (int rc = check_closed<NP>(hs)) return rc;
    tables = table_lds<NP>(hs, P.samp);
  }
  // the fused closed-form kernel and the check of nibble rows count with
  // pair bins (QbaPB, n = 11) when the launch is large enough to repay their
  // flush (a fixed ~2 us per launch: 1e6 entries 17.7 vs 15.0 us, 1.25e8
  // entries 298 vs 313 us, profiles/r4/small_launch); the tests' list_grid
  // knob (qba_test_set_knobs) forces them
  P.pb = ((L.mode == 1 && QbaUsePB<NP, 1, QBA_S_CLOSED, 0>::value && P.samp == QBA_S_CLOSED) ||
          (L.mode == 2 && QbaUsePB<NP, 2, QBA_S_GENERAL, 1>::value && L.packed)) &&
         (L.count >= ctx->pb_min || ctx->list_grid > 0);
  P.wide = rows_wide(L.packed, L.lists, L.ld);
  QbaShape &S = P.sync;
  S.block = QBA_LBLOCK;
  S.lds = lds_round(tables + (P.pb ? qba_pb_lds(QBA_LBLOCK) : L.mode != 0 ? qba_count_lds<NP>(QBA_LBLOCK) : 0));
  if (S.lds == 0) S.lds = 16;
  S.kern = lists_kernel<NP>(L.mode, P.samp, P.pb, L.packed, P.wide);
  if (!S.kern) return qba_fail(QBA_EUNSUPPORTED, "closed form beyond n = 11");
  if (int rc = lds_allow(S.kern, S.lds)) return rc;
  S.grid = grid_for(ctx, S.kern, S.lds, L.count, quads_per_thread(L.packed, P.wide), &S.cap, QBA_LBLOCK);
  if (ctx->list_grid > 0 && S.grid > ctx->list_grid) S.grid = ctx->list_grid;  // tests (qba_test_set_knobs)
  // pair bins: at most QBA_PB_BUDGET entries per workgroup and launch (QbaPB;
  // a grid capped by the tests' list_grid knob -- tests that force wraps --
  // at most 2^23, so group 0's 24-bit total, which counts every entry of the
  // workgroup once, stays exact)
  P.pb_part = ctx->list_grid ? (uint64_t)S.grid << QBA_PB_FORCED_LOG2 : (uint64_t)S.cap * QBA_PB_BUDGET;
  if (P.pb && L.count > P.pb_part) return QBA_OK;  // split: every part plans its own launch
  if (L.defer && L.mode == 1) return plan_deferred<NP>(ctx, L, tables, P);
  return QBA_OK;
}

// A pair-bin call of more than `part` entries, one launch per part.  Later
// parts accumulate; part boundaries are multiples of 2^18 entries, so the row
// alignment and the pair parity of `first` are those of the call; only the
// last part of a deferred call defers its reduction.
template <int NP>
static int launch_parts(qba_ctx *ctx, const QbaLaunch &L, uint64_t part) {
  QbaLaunch S = L;
  int rc = QBA_OK;
  for (uint64_t done = 0; !rc && done < L.count; done += S.count) {
    S.count = L.count - done < part ? L.count - done : part;
    S.defer = done + S.count >= L.count ? L.defer : 0;
    S.first = L.first + done;
    S.lists = L.lists + (L.packed ? done >> 1 : done);
    S.accumulate = done ? 1 : L.accumulate;
    S.stats_accumulate = done ? 1 : L.stats_accumulate;
    rc = qba_launch_lists<NP>(ctx, S);
  }
  return rc;
}

// The list kernel with the pending deferred call's reduction in its last
// workgroups; this call becomes the pending one.  The rules of ctx->pend:
//   * a pending call of another n or on another stream is flushed on its own;
//   * none may be pending across a graph-capture boundary (qba_flush_pending
//     refuses one recorded in another capture state, and so does this);
//   * the slab is double-buffered: this call's rows go to the half the
//     pending call's do not occupy;
//   * the pending call is flushed before the slab is reallocated.
template <int NP>
static int launch_deferred(qba_ctx *ctx, const QbaLaunch &L, const QbaShape &D) {
  using C = QCfg<NP>;
  auto &pd = ctx->pend;
  int rc = QBA_OK;
  if (pd.flush && (pd.flush != &qba_flush_def<NP> || pd.stream != L.stream))
    if ((rc = qba_flush_pending(ctx, L.stream))) return rc;
  unsigned long long cid = 0;
  const int captured = qba_capture_of(L.stream, &cid);
  if (pd.flush && (captured != ctx->pend_captured || (captured && cid != ctx->pend_capture_id)))
    return qba_fail(QBA_ESTATE, "a deferred reduction is pending across a graph-capture boundary: call "
                                "qba_flush_deferred before beginning and before ending a capture");
  if (!pd.flush && (rc = qba_slab_order(ctx, L.stream))) return rc;
  const size_t half_need = ((size_t)D.grid * C::NBP * sizeof(uint32_t) + 255) & ~(size_t)255;
  if (ctx->slab_bytes < 2 * half_need) {
    if ((rc = qba_flush_pending(ctx, L.stream))) return rc;
    if ((rc = qba_ensure_slab(ctx, 2 * half_need))) return rc;  // synchronises before a reallocation
  }
  const size_t half = (ctx->slab_bytes / 2) & ~(size_t)255;
  const int red = pd.flush ? qba_def_wgs<NP>() : 0;
  const int buf = pd.flush ? pd.buf ^ 1 : 0;
  uint32_t *slab = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(ctx->slab) + (size_t)buf * half);
  uint32_t k0 = (uint32_t)L.seed, k1 = (uint32_t)(L.seed >> 32), count = (uint32_t)L.count;
  QbaDefer d{pd.slab, pd.rows, red, pd.acc, pd.sacc, pd.H, pd.C, pd.P, pd.stats};
  QbaZero zero{L.H, L.C, L.P, L.stats, 0u};  // the reduction writes every output word itself
  void *args[] = {(void *)&L.ps, &k0, &k1, (void *)&L.first, &count, (void *)&L.lists, (void *)&L.ld, &slab, &zero, &d};
  QBA_HIP(hipLaunchKernel(D.kern, dim3(D.grid + red), dim3(D.block), args, D.lds, L.stream));
  QBA_HIP(hipGetLastError());
  pd.flush = &qba_flush_def<NP>;
  pd.slab = slab;
  pd.rows = D.grid;
  pd.acc = L.accumulate;
  pd.sacc = L.stats_accumulate;
  pd.buf = buf;
  pd.H = L.H;
  pd.C = L.C;
  pd.P = L.P;
  pd.stats = L.stats;
  pd.stream = L.stream;
  ctx->pend_captured = captured;
  ctx->pend_capture_id = cid;
  return qba_slab_done(ctx, L.stream);
}

// The list kernel and, for a counting mode, the reduce of its slab rows.
template <int NP>
static int launch_sync(qba_ctx *ctx, const QbaLaunch &L, const QbaShape &S) {
  using C = QCfg<NP>;
  uint32_t *slab = nullptr;
  if (L.mode != 0) {
    if (int rc = qba_flush_pending(ctx, L.stream)) return rc;
    if (int rc = qba_slab_order(ctx, L.stream)) return rc;
    if (int rc = qba_ensure_slab(ctx, (size_t)S.grid * C::NBP * sizeof(uint32_t))) return rc;
    slab = reinterpret_cast<uint32_t *>(ctx->slab);
  }
  uint32_t k0 = (uint32_t)L.seed, k1 = (uint32_t)(L.seed >> 32), count = (uint32_t)L.count;
  QbaZero zero{L.H, L.C, L.P, L.stats,
               (L.mode != 0 && !L.accumulate ? 1u : 0u) | (L.mode != 0 && !L.stats_accumulate ? 2u : 0u)};
  void *args[] = {(void *)&L.ps, &k0, &k1, (void *)&L.first, &count, (void *)&L.lists, (void *)&L.ld, &slab, &zero};
  QBA_HIP(hipLaunchKernel(S.kern, dim3(S.grid), dim3(S.block), args, S.lds, L.stream));
  QBA_HIP(hipGetLastError());
  if (L.mode == 0) return QBA_OK;
  // (qba_k_reduce_def as the synchronous reduce: 6.4 vs 5.5 us at 512 slab
  // rows, profiles/r3/r3p -- the atomic column reduce stays)
  const dim3 rgrid((C::NBP / 4 + 255) / 256, (S.grid + QBA_RED_ROWS - 1) / QBA_RED_ROWS);
  hipLaunchKernelGGL(qba_k_reduce<NP>, rgrid, dim3(256), 0, L.stream, slab, S.grid, L.H, L.C, L.P, L.stats);
  QBA_HIP(hipGetLastError());
  return qba_slab_done(ctx, L.stream);
}

template <int NP>
int qba_launch_lists(qba_ctx *ctx, const QbaLaunch &L) {
  QbaPlan P;
  if (int rc = plan_lists<NP>(ctx, L, P)) return rc;
  if (P.pb && L.count > P.pb_part) return launch_parts<NP>(ctx, L, P.pb_part);
  if (P.def.kern) return launch_deferred<NP>(ctx, L, P.def);
  return launch_sync<NP>(ctx, L, P.sync);
}

// The batched launch of kernel family F: qba_k_batched, or qba_k_batched_noisy,
// which takes B.noise after the same arguments and runs in the same shape.
template <int NP, template <int, int> class F>
static int launch_batched(qba_ctx *ctx, const QbaBatch &B) {
  const QbaProgramSet *hs = reinterpret_cast<const QbaProgramSet *>(ctx->prog_host[NP]);
  const int samp = sampler_of<NP>(hs);
  if (int rc = check_closed<NP>(hs)) return rc;
  const size_t lds = lds_round(table_lds<NP>(hs, samp) + qba_count_lds<NP>(QBA_BLOCK));
  // row vectors when every row start of every instance allows it
  const bool wide = rows_wide(B.packed, B.lists, B.ld, B.inst_stride);
  const int64_t cap = (int64_t)ctx->num_cus * 16;
  const int grid = (int)(B.n_inst < cap ? B.n_inst : cap);
  if (samp == QBA_S_CLOSED && NP > QBA_CLOSED_MAX_N) return qba_fail(QBA_EUNSUPPORTED, "closed form beyond n = 11");
  const void *kern = pick_sampler<NP, F>(samp, B.packed, wide);
  if (!kern) return qba_fail(QBA_EINVAL, "nibble rows must be 4-byte aligned");  // refused before (qba_lists.hip)
  if (int rc = lds_allow(kern, lds)) return rc;
  // (B's fields have the kernel arguments' types)
  constexpr int NARGS = 10 + (F<NP, QBA_S_GENERAL>::NOISE ? 1 : 0);
  const void *all[] = {&B.ps, &B.seed_base, &B.n_inst, &B.count, &B.lists, &B.ld, &B.inst_stride, &B.H, &B.C, &B.P,
                       &B.noise};
  void *args[NARGS];
  for (int i = 0; i < NARGS; ++i) args[i] = const_cast<void *>(all[i]);
  QBA_HIP(hipLaunchKernel(kern, dim3(grid), dim3(QBA_BLOCK), args, lds, B.stream));
  QBA_HIP(hipGetLastError());
  return QBA_OK;
}

// The noiseless kernels are instantiated by qba_lists_inst.hip, the noisy ones
// by qba_lists_noise_inst.hip: code objects of their own (as qba_mc_kern.h).
#ifndef QBA_BATCHED_NOISY_INST
template <int NP>
int qba_launch_batched(qba_ctx *ctx, const QbaBatch &B) {
  return launch_batched<NP, QbaKBatched>(ctx, B);
}
#else
template <int NP>
int qba_launch_batched_noisy(qba_ctx *ctx, const QbaBatch &B) {
  return launch_batched<NP, QbaKBatchedNoisy>(ctx, B);
}
#endif
