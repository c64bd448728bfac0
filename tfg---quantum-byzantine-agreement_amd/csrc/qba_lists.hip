// qba_lists.hip -- C ABI of the list kernels: argument checks, 2^31-entry
// launch chunks and dispatch to the per-n instantiations (qba_lists_inst.hip).
#include <type_traits>

#include "qba_lists.h"
#include "qba_proto_adv.h"
#include "qba_proto_coal.h"
#include "qba_proto_net.h"
#include "qba_noise_profile.h"

// Experiment builds only (tools/exp): restrict instantiation to one n.
#ifndef QBA_ONLY_N
#define QBA_ONLY_N 0
#endif

// 0 for a shipped build: no experiment switch in this object or in any
// per-n list-kernel object linked with it (qba_internal.h)
extern "C" int qba_build_flags(void) {
  int f = QBA_BUILD_EXPERIMENT_FLAGS;
#define QBA_FLAG(k) \
  if constexpr (QBA_ONLY_N == 0 || k == QBA_ONLY_N) f |= qba_lists_build_flags<k>();
  QBA_FLAG(1) QBA_FLAG(2) QBA_FLAG(3) QBA_FLAG(4) QBA_FLAG(5) QBA_FLAG(6) QBA_FLAG(7) QBA_FLAG(8)
  QBA_FLAG(9) QBA_FLAG(10) QBA_FLAG(11) QBA_FLAG(12) QBA_FLAG(13) QBA_FLAG(14) QBA_FLAG(15)
#undef QBA_FLAG
  return f;
}

static int nbins_of(int n) {  // QCfg<n>::NBP
  const int g = n + 1, q = qba_nq(n), w = 1 << q;
  return (w * g * (w + 1) + w * g * (g - 1) / 2 + 2 + 3) & ~3;
}

// packed: nibble rows, ld >= ceil(count / 2) bytes
static int check_common(qba_ctx *ctx, int n, const uint8_t *lists, uint64_t count, uint64_t ld,
                        const char *who, bool packed = false) {
  if (!ctx) return qba_fail(QBA_EINVAL, std::string(who) + ": ctx is NULL");
  if (n < 1 || n > QBA_MAX_PARTIES)
    return qba_fail(QBA_EUNSUPPORTED, std::string(who) + ": n_parties must be in [1, 15]");
  if (count == 0) return QBA_OK;
  if (!lists) return qba_fail(QBA_EINVAL, std::string(who) + ": lists is NULL");
  const uint64_t need = packed ? (count + 1) / 2 : count;
  if (ld < need || (ld & 3) || (reinterpret_cast<uintptr_t>(lists) & 3))
    return qba_fail(QBA_EINVAL, std::string(who) + (packed ? ": need ld >= (count + 1) / 2" : ": need ld >= count") +
                                    ", ld % 4 == 0 and a 4-byte aligned base");
  return qba_set_device(ctx);
}

static int need_program(qba_ctx *ctx, int n, const char *who) {
  if (!ctx->compiled[n][0] || !ctx->compiled[n][1])
    return qba_fail(QBA_ESTATE, std::string(who) + ": no resource program compiled for n=" +
                                    std::to_string(n) + " (call qba_resource_compile for both kinds)");
  return QBA_OK;
}

// f(std::integral_constant<int, n>()) for the n of a call: the per-n
// instantiations (an experiment build, QBA_ONLY_N, has those of one n only)
template <int K = 1, class F>
static int with_n(int n, const F &f) {
  if constexpr (K > QBA_MAX_PARTIES) {
    return qba_fail(QBA_EUNSUPPORTED, "n_parties must be in [1, 15]");
  } else {
    if (n != K) return with_n<K + 1>(n, f);
    if constexpr (QBA_ONLY_N == 0 || K == QBA_ONLY_N) return f(std::integral_constant<int, K>());
    return qba_fail(QBA_EUNSUPPORTED, "experiment build");
  }
}

static const char *bad_flip(uint32_t flip_q16) { return flip_q16 > 65535u ? "flip_q16 must be <= 65535" : nullptr; }

// The four batched calls: byte or nibble rows, noiseless (flip_q16 0: the
// noiseless kernel) or noisy.  flip_q16 is checked before ctx is looked at,
// as in the noisy Monte-Carlo calls.
static int batched(qba_ctx *ctx, int n, uint64_t seed_base, int64_t n_inst, uint64_t count, uint32_t flip_q16,
                   uint8_t *lists, uint64_t ld, uint64_t inst_stride, int64_t *H, int64_t *C, int64_t *P,
                   qba_stream stream, bool packed, const char *who) {
  if (const char *bad = bad_flip(flip_q16)) return qba_fail(QBA_EINVAL, std::string(who) + ": " + bad);
  int rc = check_common(ctx, n, lists, count, ld, who, packed);
  if (rc) return rc;
  if (n_inst < 0 || !H || !C || !P || (n_inst > 1 && inst_stride < (uint64_t)(n + 1) * ld) ||
      (inst_stride & 3) || count >= (1ull << 31))
    return qba_fail(QBA_EINVAL, std::string(who) + ": bad arguments (inst_stride >= (n+1)*ld, "
                                "multiple of 4; count < 2^31)");
  if (n_inst == 0 || count == 0) return QBA_OK;
  if ((rc = need_program(ctx, n, who))) return rc;
  QbaBatch B{n, (const QbaProgramSet *)ctx->prog_dev[n], seed_base, n_inst, count, lists, ld,
             inst_stride, H, C, P, (hipStream_t)stream, packed ? 1 : 0, {}};
  if (flip_q16) {
    B.noise = qba_noise_of(flip_q16);
    return with_n(n, [&](auto k) { return qba_launch_batched_noisy<decltype(k)::value>(ctx, B); });
  }
  return with_n(n, [&](auto k) { return qba_launch_batched<decltype(k)::value>(ctx, B); });
}

extern "C" int qba_sample_check_batched(qba_ctx *ctx, int n, uint64_t seed_base, int64_t n_inst, uint64_t count,
                                        uint8_t *lists, uint64_t ld, uint64_t inst_stride, int64_t *H, int64_t *C,
                                        int64_t *P, qba_stream stream) {
  return batched(ctx, n, seed_base, n_inst, count, 0u, lists, ld, inst_stride, H, C, P, stream, false,
                 "qba_sample_check_batched");
}

extern "C" int qba_sample_check_batched_noisy(qba_ctx *ctx, int n, uint64_t seed_base, int64_t n_inst, uint64_t count,
                                              uint32_t flip_q16, uint8_t *lists, uint64_t ld, uint64_t inst_stride,
                                              int64_t *H, int64_t *C, int64_t *P, qba_stream stream) {
  return batched(ctx, n, seed_base, n_inst, count, flip_q16, lists, ld, inst_stride, H, C, P, stream, false,
                 "qba_sample_check_batched_noisy");
}

extern "C" int qba_sample_check_batched_packed(qba_ctx *ctx, int n, uint64_t seed_base, int64_t n_inst, uint64_t count,
                                               uint8_t *packed, uint64_t ld, uint64_t inst_stride, int64_t *H,
                                               int64_t *C, int64_t *P, qba_stream stream) {
  return batched(ctx, n, seed_base, n_inst, count, 0u, packed, ld, inst_stride, H, C, P, stream, true,
                 "qba_sample_check_batched_packed");
}

extern "C" int qba_sample_check_batched_packed_noisy(qba_ctx *ctx, int n, uint64_t seed_base, int64_t n_inst,
                                                     uint64_t count, uint32_t flip_q16, uint8_t *packed, uint64_t ld,
                                                     uint64_t inst_stride, int64_t *H, int64_t *C, int64_t *P,
                                                     qba_stream stream) {
  return batched(ctx, n, seed_base, n_inst, count, flip_q16, packed, ld, inst_stride, H, C, P, stream, true,
                 "qba_sample_check_batched_packed_noisy");
}

// The two sampled calls behind their envelopes: M holds the checkpoints
static int mc_sampled(qba_ctx *ctx, int n, QbaMc &M) {
  if (int rc = need_program(ctx, n, M.who)) return rc;
  if (M.n_inst == 0) return QBA_OK;
  if (int rc = qba_set_device(ctx)) return rc;
  M.ps = (const QbaProgramSet *)ctx->prog_dev[n];
  if (M.use_adv) return with_n(n, [&](auto k) { return qba_launch_mc_adv<decltype(k)::value>(ctx, M); });
  if (M.noise.steps)
    return with_n(n, [&](auto k) { return qba_launch_mc_noisy<decltype(k)::value>(ctx, M); });
  return with_n(n, [&](auto k) { return qba_launch_mc<decltype(k)::value>(ctx, M); });
}

// The single-count and the curve call, noiseless (flip_q16 0: the noiseless
// kernel) or noisy, behind the names they are exported under.
// `adv` (NULL: no policy) picks the _adv kernels, under the policy word it points to.
static int mc_one(const char *who, qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst, uint64_t count,
                  uint32_t flip_q16, int32_t *out, qba_stream stream, const uint32_t *adv = nullptr) {
  QbaMc M{who, nullptr, seed_base, n_inst, n_dis, out, (hipStream_t)stream, {{(uint32_t)count}, 1}, 0, {},
          adv ? *adv : 0u, adv != nullptr};
  const char *bad = count >> 31 ? "count must be < 2^31" : bad_flip(flip_q16);
  if (!bad && adv) bad = qba_adv_bad(*adv);
  if (int rc = qba_mc_check(who, ctx, n, n_dis, bad, n_inst, out)) return rc;
  if (flip_q16) M.noise = qba_noise_of(flip_q16);
  return mc_sampled(ctx, n, M);
}

static int mc_curve(const char *who, qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                    const uint32_t *counts, int n_counts, uint32_t flip_q16, int32_t *out, qba_stream stream,
                    const uint32_t *adv = nullptr) {
  QbaMc M{who, nullptr, seed_base, n_inst, n_dis, out, (hipStream_t)stream, {}, 1, {}, adv ? *adv : 0u, adv != nullptr};
  const char *bad = bad_flip(flip_q16);
  if (!bad && adv) bad = qba_adv_bad(*adv);
  if (int rc = qba_mc_curve_check(who, ctx, n, n_dis, n_inst, counts, n_counts, out, &M.counts, bad)) return rc;
  if (flip_q16) M.noise = qba_noise_of(flip_q16);
  return mc_sampled(ctx, n, M);
}

extern "C" int qba_montecarlo_sampled(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                      uint64_t count, int32_t *out, qba_stream stream) {
  return mc_one("qba_montecarlo_sampled", ctx, n, n_dis, seed_base, n_inst, count, 0u, out, stream);
}

extern "C" int qba_montecarlo_sampled_noisy(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                            uint64_t count, uint32_t flip_q16, int32_t *out, qba_stream stream) {
  return mc_one("qba_montecarlo_sampled_noisy", ctx, n, n_dis, seed_base, n_inst, count, flip_q16, out, stream);
}

extern "C" int qba_montecarlo_curve_sampled(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                            const uint32_t *counts, int n_counts, int32_t *out,
                                            qba_stream stream) {
  return mc_curve("qba_montecarlo_curve_sampled", ctx, n, n_dis, seed_base, n_inst, counts, n_counts, 0u, out,
                  stream);
}

extern "C" int qba_montecarlo_curve_sampled_noisy(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                                  const uint32_t *counts, int n_counts, uint32_t flip_q16,
                                                  int32_t *out, qba_stream stream) {
  return mc_curve("qba_montecarlo_curve_sampled_noisy", ctx, n, n_dis, seed_base, n_inst, counts, n_counts, flip_q16,
                  out, stream);
}

// The two under an adversary policy word: the noisy
// calls' arguments, then the word, checked after flip_q16 and before ctx.
extern "C" int qba_montecarlo_sampled_adv(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                          uint64_t count, uint32_t flip_q16, int32_t *out, qba_stream stream,
                                          uint32_t adv) {
  return mc_one("qba_montecarlo_sampled_adv", ctx, n, n_dis, seed_base, n_inst, count, flip_q16, out, stream, &adv);
}

extern "C" int qba_montecarlo_curve_sampled_adv(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                                const uint32_t *counts, int n_counts, uint32_t flip_q16,
                                                int32_t *out, qba_stream stream, uint32_t adv) {
  return mc_curve("qba_montecarlo_curve_sampled_adv", ctx, n, n_dis, seed_base, n_inst, counts, n_counts, flip_q16,
                  out, stream, &adv);
}

// The curve call with colluding traitors: the _adv
// curve call's arguments, then the coalition word, checked right after the
// policy word and before ctx.
extern "C" int qba_montecarlo_curve_sampled_coal(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                                 const uint32_t *counts, int n_counts, uint32_t flip_q16,
                                                 int32_t *out, qba_stream stream, uint32_t adv, uint32_t coal) {
  const char *who = "qba_montecarlo_curve_sampled_coal";
  QbaMc M{who, nullptr, seed_base, n_inst, n_dis, out, (hipStream_t)stream, {}, 1, {}, adv, 1, {}, coal};
  const char *bad = bad_flip(flip_q16);
  if (!bad) bad = qba_adv_bad(adv);
  if (!bad) bad = qba_coal_bad(coal);
  if (int rc = qba_mc_curve_check(who, ctx, n, n_dis, n_inst, counts, n_counts, out, &M.counts, bad)) return rc;
  if (flip_q16) M.noise = qba_noise_of(flip_q16);
  if (int rc = need_program(ctx, n, who)) return rc;
  if (n_inst == 0) return QBA_OK;
  if (int rc = qba_set_device(ctx)) return rc;
  M.ps = (const QbaProgramSet *)ctx->prog_dev[n];
  return with_n(n, [&](auto k) { return qba_launch_mc_coal<decltype(k)::value>(ctx, M); });
}

// The curve call on a network that loses packets: the
// _adv curve call's arguments, then the network word, checked right after the
// policy word and before ctx.
extern "C" int qba_montecarlo_curve_sampled_net(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                                const uint32_t *counts, int n_counts, uint32_t flip_q16, int32_t *out,
                                                qba_stream stream, uint32_t adv, uint32_t net) {
  const char *who = "qba_montecarlo_curve_sampled_net";
  QbaMc M{who, nullptr, seed_base, n_inst, n_dis, out, (hipStream_t)stream, {}, 1, {}, adv, 1, {}, 0u, net};
  const char *bad = bad_flip(flip_q16);
  if (!bad) bad = qba_adv_bad(adv);
  if (!bad) bad = qba_net_bad(net);
  if (int rc = qba_mc_curve_check(who, ctx, n, n_dis, n_inst, counts, n_counts, out, &M.counts, bad)) return rc;
  if (flip_q16) M.noise = qba_noise_of(flip_q16);
  if (int rc = need_program(ctx, n, who)) return rc;
  if (n_inst == 0) return QBA_OK;
  if (int rc = qba_set_device(ctx)) return rc;
  M.ps = (const QbaProgramSet *)ctx->prog_dev[n];
  return with_n(n, [&](auto k) { return qba_launch_mc_net<decltype(k)::value>(ctx, M); });
}

// The curve call under a noise profile: the _adv
// curve call's arguments without flip_q16, then the profile, checked right
// after the policy word and before ctx.  The profile travels in the kernel
// arguments: nothing is allocated or copied.
extern "C" int qba_montecarlo_curve_sampled_nprof(qba_ctx *ctx, int n, int n_dis, uint64_t seed_base, int64_t n_inst,
                                                  const uint32_t *counts, int n_counts, int32_t *out,
                                                  qba_stream stream, uint32_t adv, const uint16_t *rates,
                                                  int n_rates, uint32_t depol_q16) {
  const char *who = "qba_montecarlo_curve_sampled_nprof";
  QbaMc M{who, nullptr, seed_base, n_inst, n_dis, out, (hipStream_t)stream, {}, 1, {}, adv, 1};
  const char *bad = qba_adv_bad(adv);
  if (!bad) bad = qba_nprof_bad(n, rates, n_rates, depol_q16);
  if (int rc = qba_mc_curve_check(who, ctx, n, n_dis, n_inst, counts, n_counts, out, &M.counts, bad)) return rc;
  const QbaNoiseProfile P = qba_nprof_of(rates, n_rates, depol_q16);
  if (int rc = need_program(ctx, n, who)) return rc;
  if (n_inst == 0) return QBA_OK;
  if (int rc = qba_set_device(ctx)) return rc;
  M.ps = (const QbaProgramSet *)ctx->prog_dev[n];
  return with_n(n, [&](auto k) { return qba_launch_mc_nprof<decltype(k)::value>(ctx, M, P); });
}

// The curve call under every scenario of a list: one
// pass over the entries, the rounds once per checkpoint and scenario.  Checked
// in the order counts, flip_q16, scenarios, ctx (qba_mc_sweep_check).
extern "C" int qba_montecarlo_sweep_sampled(qba_ctx *ctx, int n, uint64_t seed_base, int64_t n_inst,
                                            const uint32_t *counts, int n_counts, const qba_mc_scenario *scen,
                                            int n_scen, uint32_t flip_q16, int32_t *out, qba_stream stream) {
  const char *who = "qba_montecarlo_sweep_sampled";
  QbaMc M{who, nullptr, seed_base, n_inst, 0, out, (hipStream_t)stream, {}, 1, {}, 0u, 0, {}};
  if (int rc = qba_mc_sweep_check(who, ctx, n, n_inst, counts, n_counts, scen, n_scen, bad_flip(flip_q16), out,
                                  &M.counts, &M.scen))
    return rc;
  if (flip_q16) M.noise = qba_noise_of(flip_q16);
  if (int rc = need_program(ctx, n, who)) return rc;
  if (n_inst == 0) return QBA_OK;
  if (int rc = qba_set_device(ctx)) return rc;
  M.ps = (const QbaProgramSet *)ctx->prog_dev[n];
  return with_n(n, [&](auto k) { return qba_launch_mc_sweep<decltype(k)::value>(ctx, M); });
}

// The sweep call with a network word in every scenario (DESIGN.md section
// 13.12): one pass over the entries, the lossy-network rounds once per
// checkpoint and scenario.  Checked in the sweep call's order, a scenario
// n_dishonest, adv, then net (qba_mc_grid_check).
extern "C" int qba_montecarlo_grid_sampled(qba_ctx *ctx, int n, uint64_t seed_base, int64_t n_inst,
                                           const uint32_t *counts, int n_counts, const qba_mc_grid_scenario *scen,
                                           int n_scen, uint32_t flip_q16, int32_t *out, qba_stream stream) {
  const char *who = "qba_montecarlo_grid_sampled";
  QbaMc M{who, nullptr, seed_base, n_inst, 0, out, (hipStream_t)stream, {}, 1, {}, 0u, 0, {}, 0u, 0u, {}};
  if (int rc = qba_mc_grid_check(who, ctx, n, n_inst, counts, n_counts, scen, n_scen, bad_flip(flip_q16), out,
                                 &M.counts, &M.grid))
    return rc;
  if (flip_q16) M.noise = qba_noise_of(flip_q16);
  if (int rc = need_program(ctx, n, who)) return rc;
  if (n_inst == 0) return QBA_OK;
  if (int rc = qba_set_device(ctx)) return rc;
  M.ps = (const QbaProgramSet *)ctx->prog_dev[n];
  return with_n(n, [&](auto k) { return qba_launch_mc_grid<decltype(k)::value>(ctx, M); });
}

// The flips of the noisy Monte-Carlo calls into lists in the layout of
// qba_sample_check_batched, in place (qba_noise.hip); its argument checks,
// after flip_q16.  Needs no program: it samples nothing.
extern "C" int qba_noise_apply_batched(qba_ctx *ctx, int n, uint64_t seed_base, int64_t n_inst, uint64_t count,
                                       uint32_t flip_q16, uint8_t *lists, uint64_t ld, uint64_t inst_stride,
                                       qba_stream stream) {
  const char *who = "qba_noise_apply_batched";
  if (const char *bad = bad_flip(flip_q16)) return qba_fail(QBA_EINVAL, std::string(who) + ": " + bad);
  if (int rc = check_common(ctx, n, lists, count, ld, who)) return rc;
  if (n_inst < 0 || (n_inst > 1 && inst_stride < (uint64_t)(n + 1) * ld) || (inst_stride & 3) ||
      count >= (1ull << 31))
    return qba_fail(QBA_EINVAL, std::string(who) + ": bad arguments (inst_stride >= (n+1)*ld, "
                                "multiple of 4; count < 2^31)");
  if (n_inst == 0 || count == 0 || flip_q16 == 0) return QBA_OK;
  return qba_launch_noise_apply(n, seed_base, n_inst, count, flip_q16, lists, ld, inst_stride, (hipStream_t)stream);
}

// The masks of a noise profile into lists in that layout, in place
// (qba_proto_nprof.hip): the profile's checks first,
// as the profile curve calls make them, then qba_noise_apply_batched's.
extern "C" int qba_noise_profile_apply(qba_ctx *ctx, int n, uint64_t seed_base, int64_t n_inst, uint64_t count,
                                       const uint16_t *rates, int n_rates, uint32_t depol_q16, uint8_t *lists,
                                       uint64_t ld, uint64_t inst_stride, qba_stream stream) {
  const char *who = "qba_noise_profile_apply";
  if (n >= 1 && n <= QBA_MAX_PARTIES)  // n_parties itself is check_common's refusal
    if (const char *bad = qba_nprof_bad(n, rates, n_rates, depol_q16))
      return qba_fail(QBA_EINVAL, std::string(who) + ": " + bad);
  if (int rc = check_common(ctx, n, lists, count, ld, who)) return rc;
  if (n_inst < 0 || (n_inst > 1 && inst_stride < (uint64_t)(n + 1) * ld) || (inst_stride & 3) ||
      count >= (1ull << 31))
    return qba_fail(QBA_EINVAL, std::string(who) + ": bad arguments (inst_stride >= (n+1)*ld, "
                                "multiple of 4; count < 2^31)");
  const QbaNoiseProfile P = qba_nprof_of(rates, n_rates, depol_q16);
  if (n_inst == 0 || count == 0 || !(P.steps | P.depol)) return QBA_OK;
  return qba_launch_nprof_apply(n, seed_base, n_inst, count, P, lists, ld, inst_stride, (hipStream_t)stream);
}

static int mc_shape(const char *who, int n, int curve, int *waves, int64_t *lds_bytes, int *wgs_per_cu) {
  if (n < 1 || n > QBA_MAX_PARTIES || !waves || !lds_bytes || !wgs_per_cu)
    return qba_fail(QBA_EINVAL, std::string(who) + ": n_parties must be in [1, 15] and the outputs not NULL");
  return with_n(n, [&](auto k) {
    qba_mc_shape_n<decltype(k)::value>(curve, waves, lds_bytes, wgs_per_cu);
    return (int)QBA_OK;
  });
}

extern "C" int qba_montecarlo_curve_shape(int n, int *waves, int64_t *lds_bytes, int *wgs_per_cu) {
  return mc_shape("qba_montecarlo_curve_shape", n, 1, waves, lds_bytes, wgs_per_cu);
}

extern "C" int qba_montecarlo_shape(int n, int *waves, int64_t *lds_bytes, int *wgs_per_cu) {
  return mc_shape("qba_montecarlo_shape", n, 0, waves, lds_bytes, wgs_per_cu);
}

// The shape of the coalition kernel (its waves hold their hold lists too)
extern "C" int qba_montecarlo_coal_shape(int n, int *waves, int64_t *lds_bytes, int *wgs_per_cu) {
  if (n < 1 || n > QBA_MAX_PARTIES || !waves || !lds_bytes || !wgs_per_cu)
    return qba_fail(QBA_EINVAL, "qba_montecarlo_coal_shape: n_parties must be in [1, 15] and the outputs not NULL");
  return with_n(n, [&](auto k) {
    qba_mc_coal_shape_n<decltype(k)::value>(waves, lds_bytes, wgs_per_cu);
    return (int)QBA_OK;
  });
}

extern "C" int qba_montecarlo_program_shape(qba_ctx *ctx, int n, int curve, int *sampler, int *waves_compiled,
                                            int *waves_run, int64_t *lds_bytes, int *wgs_per_cu) {
  const char *who = "qba_montecarlo_program_shape";
  if (n < 1 || n > QBA_MAX_PARTIES || !sampler || !waves_compiled || !waves_run || !lds_bytes || !wgs_per_cu)
    return qba_fail(QBA_EINVAL, std::string(who) + ": n_parties must be in [1, 15] and the outputs not NULL");
  if (!ctx) return qba_fail(QBA_EINVAL, std::string(who) + ": ctx is NULL");
  if (int rc = need_program(ctx, n, who)) return rc;
  return with_n(n, [&](auto k) {
    return qba_mc_program_shape_n<decltype(k)::value>(ctx, curve, sampler, waves_compiled, waves_run, lds_bytes,
                                                      wgs_per_cu);
  });
}

// Launches of at most QBA_CHUNK entries (32-bit in-kernel offsets, u32 bins)
// that never cross a multiple of 2^33 entries (inside a launch the high word
// of the Philox pair counter e >> 1 is constant: qba_sample_quad keeps it in
// an SGPR); chunks after the first accumulate into the caller's counts.
//
// Nibble rows: every chunk boundary is an even column (whole bytes: chunk
// sizes are multiples of 4, and an even first makes the 2^33 split even; an
// odd first never takes the pair fast path, so it needs no split), so no
// byte is shared by two launches.
static int dispatch(qba_ctx *ctx, const QbaLaunch &L0) {
  QbaLaunch L = L0;
  uint64_t done = 0;
  int rc = QBA_OK;
  constexpr uint64_t PHI_SPAN = 1ull << 33;
  const bool pk = L0.packed != 0;
  const uintptr_t VA = pk ? 3 : 7;  // the wide step's row-vector alignment - 1
  do {
    L.count = L0.count - done < ctx->chunk ? L0.count - done : ctx->chunk;
    if (!pk || !((L0.first + done) & 1)) {
      const uint64_t to_span = PHI_SPAN - ((L0.first + done) & (PHI_SPAN - 1));
      if (L.count > to_span) L.count = to_span;
    }
    // A chunk that starts off the wide kernels' row alignment (8 B; 4 B for
    // nibble rows) -- the caller's first column, or the 2^33 split above --
    // is cut to the next aligned column, so that every later chunk of the
    // call runs the wide kernel (qba_launch_lists picks the narrow one for
    // unaligned rows); rows must be aligned to begin with (ld % 8 == 0).
    uint8_t *const at = L0.lists + (pk ? done >> 1 : done);
    const uintptr_t mis = reinterpret_cast<uintptr_t>(at) & VA;
    const uint64_t cut = pk ? 2 * (4 - mis) : 8 - mis;
    if (mis && !(L0.ld & VA) && L.count > cut) L.count = cut;
    L.first = L0.first + done;
    L.lists = at;
    L.accumulate = done ? 1 : L0.accumulate;
    L.stats_accumulate = done ? 1 : 0;
    rc = with_n(L.n, [&](auto k) { return qba_launch_lists<decltype(k)::value>(ctx, L); });
    done += L.count;
  } while (!rc && done < L0.count);
  return rc;
}

int qba_capture_of(hipStream_t s, unsigned long long *id) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  unsigned long long cid = 0;
  if (hipStreamGetCaptureInfo(s, &st, &cid) != hipSuccess) st = hipStreamCaptureStatusNone;
  *id = st == hipStreamCaptureStatusActive ? cid : 0ull;
  return st == hipStreamCaptureStatusActive ? 1 : 0;
}

// A pending deferred reduction may only be launched in the capture state it
// was recorded in: an eager one into an eager stream, a captured one into the
// same capture.  Otherwise the reduction would become a graph node that
// re-reduces an overwritten slab on every replay, or an eager launch would
// reduce the slab of a graph that has not run (include/qba.h).
static int pend_capture_ok(qba_ctx *ctx, hipStream_t s) {
  unsigned long long id = 0;
  const int cap = qba_capture_of(s, &id);
  if (cap == ctx->pend_captured && (!cap || id == ctx->pend_capture_id)) return QBA_OK;
  return qba_fail(QBA_ESTATE, ctx->pend_captured
                                  ? "a deferred reduction recorded inside a graph capture is still pending outside "
                                    "it: call qba_flush_deferred before ending the capture"
                                  : "a deferred reduction is pending from before a graph capture: call "
                                    "qba_flush_deferred before beginning the capture");
}

// Only eager streams are ordered here: inside a capture the graph's own
// dependencies order its nodes, and across a capture boundary the caller
// synchronises (include/qba.h).  The previous user's stream is never touched
// (it may be destroyed since): a counting launch on another stream than the
// previous one synchronises the device, which completes that stream's work.
// A stream switch is rare; an event recorded after every counting launch
// instead put a ~6 us marker between each launch and the next on the same
// stream (profiles/r5/slab_event).
//
// Streams are told apart by their handle values (hipStreamGetId, which would
// survive a handle's reuse, is a HIP 7.1 symbol that the HIP runtime PyTorch
// ships here lacks), so a stream must be synchronised before it is destroyed
// if this ctx counted on it (include/qba.h; PyTorch pools its streams and
// never destroys them).  The device synchronisation runs in relaxed capture
// mode, so a graph that another thread captures in global mode is neither
// invalidated nor waited for (a capture has no executing work).
static unsigned long long stream_key(hipStream_t s) { return reinterpret_cast<uintptr_t>(s) | (1ull << 63); }

int qba_slab_order(qba_ctx *ctx, hipStream_t stream) {
  unsigned long long id = 0;
  if (ctx->slab_set && ctx->slab_last != stream_key(stream) && !qba_capture_of(stream, &id)) {
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    QBA_HIP(hipThreadExchangeStreamCaptureMode(&mode));
    const hipError_t e = hipDeviceSynchronize();
    (void)hipThreadExchangeStreamCaptureMode(&mode);  // restore this thread's mode
    QBA_HIP(e);
    ctx->slab_set = false;
  }
  return QBA_OK;
}

int qba_slab_done(qba_ctx *ctx, hipStream_t stream) {
  unsigned long long id = 0;
  ctx->slab_set = !qba_capture_of(stream, &id);
  ctx->slab_last = stream_key(stream);
  return QBA_OK;
}

int qba_flush_pending(qba_ctx *ctx, hipStream_t next) {
  auto &pd = ctx->pend;
  if (!pd.flush) return QBA_OK;
  if (int rc = pend_capture_ok(ctx, pd.stream)) return rc;
  if (next != pd.stream)
    if (int rc = pend_capture_ok(ctx, next)) return rc;
  int (*f)(qba_ctx *) = pd.flush;
  int rc = f(ctx);
  pd.flush = nullptr;
  if (rc || (rc = qba_slab_done(ctx, pd.stream))) return rc;  // the reduction read the slab
  if (next != pd.stream) {  // the slab may be rewritten on `next`: after this reduction
    if (!ctx->def_ev) QBA_HIP(hipEventCreateWithFlags(&ctx->def_ev, hipEventDisableTiming));
    QBA_HIP(hipEventRecord(ctx->def_ev, pd.stream));
    QBA_HIP(hipStreamWaitEvent(next, ctx->def_ev, 0));
  }
  return QBA_OK;
}

extern "C" int qba_flush_deferred(qba_ctx *ctx) {
  if (!ctx) return qba_fail(QBA_EINVAL, "qba_flush_deferred: ctx is required");
  if (!ctx->pend.flush) return QBA_OK;
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  if ((rc = pend_capture_ok(ctx, ctx->pend.stream))) {
    // a captured reduction outside its capture cannot be launched any more:
    // it is dropped (that call's counts stay incomplete) and the ctx is usable
    if (ctx->pend_captured) ctx->pend.flush = nullptr;
    return rc;
  }
  return qba_flush_pending(ctx, ctx->pend.stream);
}

static int zero_counts(qba_ctx *ctx, int n, int64_t *H, int64_t *C, int64_t *P, hipStream_t s) {
  if (int rc = qba_flush_pending(ctx, s)) return rc;  // a pending reduction may target the same outputs
  const int g = n + 1, w = 1 << qba_nq(n);
  QBA_HIP(hipMemsetAsync(H, 0, sizeof(int64_t) * w * g * w, s));
  QBA_HIP(hipMemsetAsync(C, 0, sizeof(int64_t) * w * g * g, s));
  QBA_HIP(hipMemsetAsync(P, 0, sizeof(int64_t) * w, s));
  return QBA_OK;
}

// The list entry points below: argument checks, the rule for count == 0 (a
// counting call still zeroes its outputs, or lets a pending reduction that
// may target them finish) and the launch descriptor.  mode 0: sample, 1:
// sample + check, 2: check only, which samples nothing and needs no program.
enum { BYTE_ROWS = 0, NIBBLE_ROWS = 1, DEFER = 2 };
static int lists_call(const char *who, int mode, int how, qba_ctx *ctx, int n, uint64_t seed, uint64_t first,
                      uint64_t count, uint8_t *lists, uint64_t ld, int64_t *H, int64_t *C, int64_t *P,
                      int accumulate, qba_stream stream) {
  const bool packed = how & NIBBLE_ROWS;
  const hipStream_t s = (hipStream_t)stream;
  int rc = check_common(ctx, n, lists, count, ld, who, packed);
  if (rc) return rc;
  if (mode != 0) {
    if (!H || !C || !P) return qba_fail(QBA_EINVAL, std::string(who) + ": H, C and P are required");
    if (count == 0) return accumulate ? qba_flush_pending(ctx, s) : zero_counts(ctx, n, H, C, P, s);
  }
  if (count == 0) return QBA_OK;
  if (mode != 2 && (rc = need_program(ctx, n, who))) return rc;
  QbaLaunch L{};
  L.n = n;
  L.mode = mode;
  L.ps = mode != 2 ? (const QbaProgramSet *)ctx->prog_dev[n] : nullptr;
  L.seed = seed;
  L.first = first;
  L.count = count;
  L.lists = lists;
  L.ld = ld;
  L.H = H;
  L.C = C;
  L.P = P;
  L.stats = mode != 0 ? ctx->stats : nullptr;
  L.accumulate = accumulate;
  L.stream = s;
  L.packed = packed ? 1 : 0;
  L.defer = how & DEFER ? 1 : 0;
  return dispatch(ctx, L);
}

extern "C" int qba_sample(qba_ctx *ctx, int n, uint64_t seed, uint64_t first, uint64_t count, uint8_t *lists,
                          uint64_t ld, qba_stream stream) {
  return lists_call("qba_sample", 0, BYTE_ROWS, ctx, n, seed, first, count, lists, ld, nullptr, nullptr, nullptr, 0,
                    stream);
}

extern "C" int qba_sample_check(qba_ctx *ctx, int n, uint64_t seed, uint64_t first, uint64_t count, uint8_t *lists,
                                uint64_t ld, int64_t *H, int64_t *C, int64_t *P, int accumulate, qba_stream stream) {
  return lists_call("qba_sample_check", 1, BYTE_ROWS, ctx, n, seed, first, count, lists, ld, H, C, P, accumulate,
                    stream);
}

extern "C" int qba_sample_check_deferred(qba_ctx *ctx, int n, uint64_t seed, uint64_t first, uint64_t count,
                                         uint8_t *lists, uint64_t ld, int64_t *H, int64_t *C, int64_t *P,
                                         int accumulate, qba_stream stream) {
  return lists_call("qba_sample_check_deferred", 1, BYTE_ROWS | DEFER, ctx, n, seed, first, count, lists, ld, H, C, P,
                    accumulate, stream);
}

extern "C" int qba_check_counts(qba_ctx *ctx, int n, const uint8_t *lists, uint64_t count, uint64_t ld, int64_t *H,
                                int64_t *C, int64_t *P, int accumulate, qba_stream stream) {
  return lists_call("qba_check_counts", 2, BYTE_ROWS, ctx, n, 0, 0, count, const_cast<uint8_t *>(lists), ld, H, C, P,
                    accumulate, stream);
}

// ---- nibble rows ("packed lists", qba.h) ----------------------------------------
extern "C" int qba_sample_packed(qba_ctx *ctx, int n, uint64_t seed, uint64_t first, uint64_t count, uint8_t *packed,
                                 uint64_t ldp, qba_stream stream) {
  return lists_call("qba_sample_packed", 0, NIBBLE_ROWS, ctx, n, seed, first, count, packed, ldp, nullptr, nullptr,
                    nullptr, 0, stream);
}

extern "C" int qba_sample_check_packed(qba_ctx *ctx, int n, uint64_t seed, uint64_t first, uint64_t count,
                                       uint8_t *packed, uint64_t ldp, int64_t *H, int64_t *C, int64_t *P,
                                       int accumulate, qba_stream stream) {
  return lists_call("qba_sample_check_packed", 1, NIBBLE_ROWS, ctx, n, seed, first, count, packed, ldp, H, C, P,
                    accumulate, stream);
}

extern "C" int qba_sample_check_packed_deferred(qba_ctx *ctx, int n, uint64_t seed, uint64_t first, uint64_t count,
                                                uint8_t *packed, uint64_t ldp, int64_t *H, int64_t *C, int64_t *P,
                                                int accumulate, qba_stream stream) {
  return lists_call("qba_sample_check_packed_deferred", 1, NIBBLE_ROWS | DEFER, ctx, n, seed, first, count, packed, ldp,
                    H, C, P, accumulate, stream);
}

extern "C" int qba_check_counts_packed(qba_ctx *ctx, int n, const uint8_t *packed, uint64_t count, uint64_t ldp,
                                       int64_t *H, int64_t *C, int64_t *P, int accumulate, qba_stream stream) {
  return lists_call("qba_check_counts_packed", 2, NIBBLE_ROWS, ctx, n, 0, 0, count, const_cast<uint8_t *>(packed), ldp,
                    H, C, P, accumulate, stream);
}

// Byte rows <-> nibble rows, one packed byte per thread (conversion helpers,
// not on the hot path).  bad counts values > 15 (not representable; their
// nibble is stored as value & 15).
__global__ void qba_k_pack(const uint8_t *__restrict__ lists, uint64_t ld, uint64_t count, uint64_t nbytes,
                           uint64_t total, uint8_t *__restrict__ packed, uint64_t ldp,
                           unsigned long long *__restrict__ bad) {
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t g = t / nbytes, b = t - g * nbytes, c = 2 * b;
    const uint8_t *r = lists + g * ld;
    const uint32_t lo = r[c], hi = c + 1 < count ? r[c + 1] : 0u;
    if (bad && (lo > 15u || hi > 15u)) atomicAdd(bad, (unsigned long long)((lo > 15u) + (hi > 15u)));
    packed[g * ldp + b] = (uint8_t)((lo & 15u) | ((hi & 15u) << 4));
  }
}

__global__ void qba_k_unpack(const uint8_t *__restrict__ packed, uint64_t ldp, uint64_t count, uint64_t nbytes,
                             uint64_t total, uint8_t *__restrict__ lists, uint64_t ld) {
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t g = t / nbytes, b = t - g * nbytes, c = 2 * b;
    const uint32_t v = packed[g * ldp + b];
    uint8_t *r = lists + g * ld;
    r[c] = (uint8_t)(v & 15u);
    if (c + 1 < count) r[c + 1] = (uint8_t)(v >> 4);
  }
}

static int convert_args(qba_ctx *ctx, const void *a, const void *b, int rows, uint64_t count, uint64_t ld,
                        uint64_t ldp, const char *who) {
  if (!ctx || rows < 0 || (rows && count && (!a || !b)) || (rows && count && (ld < count || ldp < (count + 1) / 2)))
    return qba_fail(QBA_EINVAL, std::string(who) + ": bad arguments (ld >= count, ldp >= (count + 1) / 2)");
  return qba_set_device(ctx);
}

static dim3 convert_grid(uint64_t total) {
  const uint64_t b = (total + 255) / 256;
  return dim3((unsigned)(b < 65536 ? (b ? b : 1) : 65536));
}

extern "C" int qba_lists_pack(qba_ctx *ctx, const uint8_t *lists, uint64_t ld, int rows, uint64_t count,
                              uint8_t *packed, uint64_t ldp, int64_t *bad_dev, qba_stream stream) {
  int rc = convert_args(ctx, lists, packed, rows, count, ld, ldp, "qba_lists_pack");
  if (rc) return rc;
  if (bad_dev) QBA_HIP(hipMemsetAsync(bad_dev, 0, sizeof(int64_t), (hipStream_t)stream));
  const uint64_t nbytes = (count + 1) / 2, total = (uint64_t)rows * nbytes;
  if (total == 0) return QBA_OK;
  hipLaunchKernelGGL(qba_k_pack, convert_grid(total), dim3(256), 0, (hipStream_t)stream, lists, ld, count, nbytes,
                     total, packed, ldp, reinterpret_cast<unsigned long long *>(bad_dev));
  QBA_HIP(hipGetLastError());
  return QBA_OK;
}

extern "C" int qba_lists_unpack(qba_ctx *ctx, const uint8_t *packed, uint64_t ldp, int rows, uint64_t count,
                                uint8_t *lists, uint64_t ld, qba_stream stream) {
  int rc = convert_args(ctx, packed, lists, rows, count, ld, ldp, "qba_lists_unpack");
  if (rc) return rc;
  const uint64_t nbytes = (count + 1) / 2, total = (uint64_t)rows * nbytes;
  if (total == 0) return QBA_OK;
  hipLaunchKernelGGL(qba_k_unpack, convert_grid(total), dim3(256), 0, (hipStream_t)stream, packed, ldp, count,
                     nbytes, total, lists, ld);
  QBA_HIP(hipGetLastError());
  return QBA_OK;
}

extern "C" int qba_reserve(qba_ctx *ctx, int n, int64_t max_blocks) {
  if (!ctx || n < 1 || n > QBA_MAX_PARTIES || max_blocks < 1)
    return qba_fail(QBA_EINVAL, "qba_reserve: bad arguments");
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  if (ctx->pend.flush && (rc = qba_flush_pending(ctx, ctx->pend.stream))) return rc;  // before a reallocation
  return qba_ensure_slab(ctx, (size_t)max_blocks * nbins_of(n) * sizeof(uint32_t));
}

// ---------------------------------------------------------------------------
// Philox KAT helper
// ---------------------------------------------------------------------------
__global__ void qba_k_philox(const uint32_t *__restrict__ ctr, int64_t n, uint32_t k0, uint32_t k1,
                             uint32_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const QbaU4 r = qba_philox(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], k0, k1);
  out[4 * i] = r.x;
  out[4 * i + 1] = r.y;
  out[4 * i + 2] = r.z;
  out[4 * i + 3] = r.w;
}

extern "C" int qba_philox_dev(qba_ctx *ctx, const uint32_t *ctr, int64_t n, uint64_t key,
                              uint32_t *out, qba_stream stream) {
  if (!ctx || n < 0 || (n && (!ctr || !out))) return qba_fail(QBA_EINVAL, "qba_philox_dev: bad arguments");
  if (n == 0) return QBA_OK;
  int rc = qba_set_device(ctx);
  if (rc) return rc;
  hipLaunchKernelGGL(qba_k_philox, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, ctr, n, (uint32_t)key, (uint32_t)(key >> 32), out);
  QBA_HIP(hipGetLastError());
  return QBA_OK;
}
