/*
 * qba.h -- C ABI of libqba.so, the MI355X (gfx950) engine for the data-parallel
 * core of the quantum Byzantine agreement protocol of
 * Carl0sGV/TFG---Quantum-Byzantine-Agreement (tfg.py).
 *
 * The reference has no plugin/operator API; its hot path
 * sits behind (1) the qsimov gate/executor calls and (2) four module-level
 * functions plus four inline comprehensions.  Each entry point below names
 * the reference interface it replaces.  INTEGRATION.md shows the ctypes
 * binding a maintainer of tfg.py would add.
 *
 * Conventions
 *   - Every function returns QBA_OK (0) or a negative qba_status; the message
 *     of the last failure on the calling thread is qba_last_error().  No C++
 *     exception crosses this boundary.
 *   - All array arguments named *_dev are DEVICE pointers allocated by the
 *     caller (e.g. torch tensors' data_ptr()); *_host are host pointers.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream).  Work is
 *     enqueued asynchronously; functions documented as "synchronous" wait.
 *   - One qba_ctx per device; a ctx is not thread-safe (one host thread, or
 *     external locking).  The ctx owns only its scratch and compiled
 *     resource programs.
 *   - Lists are uint8 matrices lists[g][k] with row stride `ld` bytes:
 *     row g = measured group g (row 0 is what rank 1 calls Li, row 1 is Lc,
 *     row g>=2 is party g's list).  ld % 4 == 0 and the base
 *     pointer must be 4-byte aligned.
 *   - Packed lists (the *_packed entry points) hold the same matrix as NIBBLE
 *     rows: byte b of row g = value of column 2b (low nibble) | value of
 *     column 2b+1 (high nibble) << 4, row stride `ld` >= (count+1)/2 bytes
 *     (same alignment rules; a missing last column's nibble is 0).  Every
 *     sampled value is < w <= 16, so nothing is lost; the fused hot path
 *     writes half the bytes.  qba_lists_pack /
 *     qba_lists_unpack convert between the two layouts.
 *   - Count tensors are int64:  H[u][g][x] (w x (n+1) x w),
 *     C[u][g][h] ((w x (n+1) x (n+1)), symmetric, diagonal = |P_u|),
 *     P[u] = |P_u| (w).  Only Q-correlated positions (L0[k] != L1[k],
 *     tfg.py:327) are counted, binned by u = L1[k] (= Lc[k], tfg.py:182).
 */
#ifndef QBA_H
#define QBA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define QBA_API __attribute__((visibility("default")))
#else
#define QBA_API
#endif

typedef struct qba_ctx qba_ctx;
typedef void *qba_stream; /* hipStream_t */

typedef enum qba_status {
  QBA_OK = 0,
  QBA_EINVAL = -1,      /* bad argument */
  QBA_EHIP = -2,        /* HIP runtime failure */
  QBA_ENOMEM = -3,      /* device allocation failed */
  QBA_EUNSUPPORTED = -4,/* outside the supported envelope (e.g. n > 15) */
  QBA_ESTATE = -5       /* e.g. no resource program compiled for this n */
} qba_status;

enum { QBA_KIND_NOTQ = 0, QBA_KIND_Q = 1 };
enum { QBA_GATE_H = 0, QBA_GATE_X = 1 }; /* gate triples: {kind, target, control|-1} */

#define QBA_MAX_PARTIES 15 /* w <= 16: one nibble per group in the 64-bit outcome */

/* ---- library / context ---------------------------------------------------------- */
QBA_API const char *qba_last_error(void);
QBA_API int qba_version(void); /* major*10000 + minor*100 + patch */
/* Nonzero when any object of this library was compiled with an experiment
 * switch (tools/exp/build.sh A/B builds, some wrong by design); 0 for the
 * shipped build. */
QBA_API int qba_build_flags(void);
QBA_API int qba_init(int device, qba_ctx **out);
QBA_API int qba_destroy(qba_ctx *ctx);
/* Pre-allocate scratch for counts launches of up to `max_blocks` workgroups so
 * that later calls never allocate (required before hipGraph capture). */
QBA_API int qba_reserve(qba_ctx *ctx, int n_parties, int64_t max_blocks);

/* ---- (A1/A2) resource preparation: dense fp64 statevector, gfx950 kernels --------- */
/* Replaces qs.QGate(...).add_operation(...) + qs.Drewom().execute(...) state
 * preparation (tfg.py:15-65, 76, 80).  Qubit 0 is the MSB of a basis index. */
QBA_API int qba_sv_init(qba_ctx *ctx, double *sv_dev, int nqubits, qba_stream stream);
QBA_API int qba_sv_apply(qba_ctx *ctx, double *sv_dev, int nqubits, const int32_t *gates_host,
                 int n_gates, qba_stream stream);
/* |0...0> followed by the gate list, in the fewest passes: single-qubit gates
 * on qubits no CX has touched yet fold into the initial product state (one
 * write-only pass), then runs of H / X / shared-control CX gates are one pass
 * each.  Same result as qba_sv_init + qba_sv_apply (tfg.py:56-65, 43-52:
 * the whole H/X layer of both circuits folds into the init pass). */
QBA_API int qba_sv_prepare(qba_ctx *ctx, double *sv_dev, int nqubits, const int32_t *gates_host,
                   int n_gates, qba_stream stream);
/* Probabilities |a_i|^2 > eps, compacted in ascending index order.  Writes at
 * most `cap` (index, prob) pairs; *count_host receives the full support size.
 * Synchronous. */
QBA_API int qba_sv_support(qba_ctx *ctx, const double *sv_dev, int nqubits, double eps,
                   int64_t *idx_dev, double *prob_dev, int64_t cap, int64_t *count_host,
                   qba_stream stream);
/* Compile one of the two circuits of an n-party run into the sampler's
 * factored alias-table program.  `gates_host` is the reference's gate list
 * for that circuit (notQCorrelated, tfg.py:15-22, or qCorrelated, tfg.py:25-40);
 * for QBA_KIND_Q, `perm_host[g-1]` is the permutation the list was built
 * with: its X gates are verified to be the classical mask the sampler draws
 * afresh per entry.  The circuit is split into entangled registers, each is
 * simulated on the device, its support compacted and turned into an alias
 * table.  Synchronous. */
QBA_API int qba_resource_compile(qba_ctx *ctx, int n_parties, int kind, const int32_t *gates_host,
                         int n_gates, const int32_t *perm_host);
/* Export the compiled program for kind (for tests / the CPU twin):
 * factor descriptors (bits, uniform, table offset, u-word) and the tables. */
QBA_API int qba_program_export(qba_ctx *ctx, int n_parties, int kind, int32_t *n_factors,
                       int32_t *desc_host /* [16][6] */, uint64_t *pat_host,
                       uint64_t *apat_host, uint64_t *thr_host, int32_t table_cap,
                       int32_t *table_len);

/* Sampler selection of the compiled pair (synchronous, host only):
 * flags[0] = canonical table layout, flags[1] = closed form (n <= 11 and both
 * programs proven equal to tfg.py's circuits' distributions), flags[2] =
 * 2^32 mod n!, flags[3..5] = permutation stage sizes A, B, C. */
QBA_API int qba_program_flags(qba_ctx *ctx, int n_parties, int32_t *flags_host /* [6] */);

/* Host only (no device needed): the closed-form permutation stage tables for
 * n in [1, 11] (layout in csrc/qba_internal.h).  sizes[0..5] = RA, RB, RC,
 * word offset of B, word offset of C, total words; `words` may be NULL to
 * query the size. */
QBA_API int qba_perm_tables(int n_parties, uint32_t *words_host, int32_t cap, int32_t *sizes_host /* [6] */);

/* ---- (A3/A4) Born sampling: Philox4x32-10 keyed by the GLOBAL entry index -------- */
/* Replaces generacionListas (tfg.py:68-84) + measure_to_ints (tfg.py:128-129):
 * writes lists[g][k - first] for entries k in [first, first+count). */
QBA_API int qba_sample(qba_ctx *ctx, int n_parties, uint64_t seed, uint64_t first, uint64_t count,
               uint8_t *lists_dev, uint64_t ld, qba_stream stream);

/* ---- (A5-A8) checks, count mode -------------------------------------------------- */
/* One pass over the lists computing H, C, P (see conventions); replaces the
 * per-packet work of tfg.py:182, 189, 291-294, 327 and consistent() 87-98 in
 * canonical order.  accumulate != 0 adds into H/C/P instead of overwriting. */
QBA_API int qba_check_counts(qba_ctx *ctx, int n_parties, const uint8_t *lists_dev, uint64_t count,
                     uint64_t ld, int64_t *H_dev, int64_t *C_dev, int64_t *P_dev,
                     int accumulate, qba_stream stream);
/* Statistics of the last counts launch on this ctx (synchronous):
 * out[0] = Q-correlated entries that held a value >= w and were therefore
 * not counted (never happens for lists from qba_sample); out[1] = workgroups
 * of an n = 11 pair-bin kernel (the fused kernel from 2^24 entries, the
 * check of nibble rows) whose 8-bit pair bins wrapped and that recounted
 * their entries exactly from the stored rows.  Pair-bin launches give a
 * workgroup at most 2^18 entries (a larger call is split, later parts
 * accumulating), where no bin wraps for sampled lists; the test seam that
 * forces wraps and pair bins on small launches (qba_test_set_knobs' list_grid
 * and pb_min_entries) gives a workgroup at most 2^23 entries per launch, below
 * group 0's 24-bit total, so a wrap is always detected exactly. */
QBA_API int qba_last_stats(qba_ctx *ctx, int64_t *out2_host);
/* Fused sample + check: lists are written once and counted from registers. */
QBA_API int qba_sample_check(qba_ctx *ctx, int n_parties, uint64_t seed, uint64_t first,
                     uint64_t count, uint8_t *lists_dev, uint64_t ld, int64_t *H_dev,
                     int64_t *C_dev, int64_t *P_dev, int accumulate, qba_stream stream);

/* The same three passes over packed (nibble-row) lists; counts identical to
 * the byte-layout calls on the same entries.  qba_check_counts_packed cannot
 * see a value > 15 (not representable); values in [w, 15] are caught as in
 * qba_check_counts (qba_last_stats).  Every counting call tests Cond3
 * (tfg.py:96-98) on every Q-correlated entry: an entry whose values are not
 * pairwise distinct adds its equal pairs to C[u][g][h]. */
QBA_API int qba_sample_packed(qba_ctx *ctx, int n_parties, uint64_t seed, uint64_t first, uint64_t count,
                              uint8_t *packed_dev, uint64_t ld, qba_stream stream);
QBA_API int qba_sample_check_packed(qba_ctx *ctx, int n_parties, uint64_t seed, uint64_t first,
                                    uint64_t count, uint8_t *packed_dev, uint64_t ld, int64_t *H_dev,
                                    int64_t *C_dev, int64_t *P_dev, int accumulate, qba_stream stream);
QBA_API int qba_check_counts_packed(qba_ctx *ctx, int n_parties, const uint8_t *packed_dev, uint64_t count,
                                    uint64_t ld, int64_t *H_dev, int64_t *C_dev, int64_t *P_dev,
                                    int accumulate, qba_stream stream);
/* Deferred reduction, for back-to-back count passes (BASELINE configs[1]:
 * sizeL = 1e6 per pass, where the separate reduce launch is a third of the
 * pass).  Same arguments and results as qba_sample_check / _packed (tfg.py:
 * 68-84, 182, 189, 291-294, 327, consistent() 87-98), but the call's H, C, P
 * and qba_last_stats are complete only after the NEXT deferred call on this
 * ctx or qba_flush_deferred(ctx): the next call's list kernel reduces this
 * call's slab rows in workgroups of its own (two alternating slab buffers),
 * dispatched after its list workgroups into the CUs they leave idle.  A
 * small call whose list workgroups fill the chip, any non-deferred counting
 * call and qba_reserve flush the pending reduction first; a pending call on
 * another stream is flushed there and ordered by an event.  A pair-bin call
 * larger than one launch's per-workgroup budget (above ~1.3e8 entries at n =
 * 11) runs its earlier parts synchronously and defers only its last part's
 * reduction; its first part flushes a pending call and then overwrites the
 * outputs, so a pending call that shares this call's H/C/P buffers ends with
 * this call's counts in them (as it would after any later call into the same
 * buffers). */
QBA_API int qba_sample_check_deferred(qba_ctx *ctx, int n_parties, uint64_t seed, uint64_t first,
                                      uint64_t count, uint8_t *lists_dev, uint64_t ld, int64_t *H_dev,
                                      int64_t *C_dev, int64_t *P_dev, int accumulate, qba_stream stream);
QBA_API int qba_sample_check_packed_deferred(qba_ctx *ctx, int n_parties, uint64_t seed, uint64_t first,
                                             uint64_t count, uint8_t *packed_dev, uint64_t ld, int64_t *H_dev,
                                             int64_t *C_dev, int64_t *P_dev, int accumulate, qba_stream stream);
/* Launches the pending deferred reduction (if any) on its call's stream.
 * Graph capture: a deferred reduction must be launched in the capture state
 * it was recorded in, so call qba_flush_deferred before beginning a capture
 * and before ending one (the deferred calls inside a capture then form a
 * closed chain).  A call that would carry a pending reduction across a
 * capture boundary fails with QBA_ESTATE; qba_flush_deferred outside the
 * capture of a captured pending reduction drops it (QBA_ESTATE: that call's
 * counts stay incomplete).  Counting calls of one ctx on different streams
 * share its scratch: a counting call on another stream than the previous
 * one synchronises the device first (so do not switch a ctx's stream while
 * another thread captures a graph on this device; qba_last_stats and
 * qba_destroy flush a pending reduction first).  Streams are told apart by
 * their handle values: synchronise a stream that ran counting calls of this
 * ctx before destroying it, since a new stream may reuse the handle.  The
 * synchronisation runs in relaxed capture mode (a graph another thread
 * captures is left alone). */
QBA_API int qba_flush_deferred(qba_ctx *ctx);
/* Rows [0, rows) of `count` columns between the layouts.  pack: *bad_dev (may
 * be NULL) receives how many values were > 15 (stored as value & 15). */
QBA_API int qba_lists_pack(qba_ctx *ctx, const uint8_t *lists_dev, uint64_t ld, int rows, uint64_t count,
                           uint8_t *packed_dev, uint64_t ldp, int64_t *bad_dev, qba_stream stream);
QBA_API int qba_lists_unpack(qba_ctx *ctx, const uint8_t *packed_dev, uint64_t ldp, int rows, uint64_t count,
                             uint8_t *lists_dev, uint64_t ld, qba_stream stream);

/* Batched independent runs (BASELINE configs[3]: 4096 independent 7-party
 * instances per GPU).  Instance i uses Philox key seed_base + i over entries
 * [0, count); its lists start at lists_dev + i*inst_stride (rows ld apart) and
 * its counts at H_dev + i*w*(n+1)*w, C_dev + i*w*(n+1)^2, P_dev + i*w. */
QBA_API int qba_sample_check_batched(qba_ctx *ctx, int n_parties, uint64_t seed_base,
                                     int64_t n_instances, uint64_t count, uint8_t *lists_dev,
                                     uint64_t ld, uint64_t inst_stride, int64_t *H_dev,
                                     int64_t *C_dev, int64_t *P_dev, qba_stream stream);

/* The same over nibble rows (ld, inst_stride in bytes of packed rows). */
QBA_API int qba_sample_check_batched_packed(qba_ctx *ctx, int n_parties, uint64_t seed_base,
                                            int64_t n_instances, uint64_t count, uint8_t *packed_dev,
                                            uint64_t ld, uint64_t inst_stride, int64_t *H_dev,
                                            int64_t *C_dev, int64_t *P_dev, qba_stream stream);

/* The two calls above under qubit-flip noise: every measured bit of an entry
 * flips with probability flip_q16 / 65536 (the flips of
 * qba_montecarlo_sampled_noisy and qba_noise_apply_batched: entry e of
 * instance i draws them under key seed_base + i) as the entry is sampled, so
 * the rows written and the tables counted are those of the noisy entries --
 * what the noiseless call followed by qba_noise_apply_batched leaves in the
 * rows, with the tables to match.  flip_q16 = 0 launches the noiseless kernel;
 * flip_q16 > 65535 is QBA_EINVAL, checked before ctx is looked at; the other
 * arguments and checks are the noiseless calls'. */
QBA_API int qba_sample_check_batched_noisy(qba_ctx *ctx, int n_parties, uint64_t seed_base,
                                           int64_t n_instances, uint64_t count, uint32_t flip_q16,
                                           uint8_t *lists_dev, uint64_t ld, uint64_t inst_stride,
                                           int64_t *H_dev, int64_t *C_dev, int64_t *P_dev, qba_stream stream);
QBA_API int qba_sample_check_batched_packed_noisy(qba_ctx *ctx, int n_parties, uint64_t seed_base,
                                                  int64_t n_instances, uint64_t count, uint32_t flip_q16,
                                                  uint8_t *packed_dev, uint64_t ld, uint64_t inst_stride,
                                                  int64_t *H_dev, int64_t *C_dev, int64_t *P_dev,
                                                  qba_stream stream);

/* The protocol rounds of the batched instances, decided on the device from
 * their count tables (H_dev, C_dev, P_dev in the layout of
 * qba_sample_check_batched): replaces, per instance, the dishonest draw
 * (tfg.py:101-125), the commander's broadcast (166-196), the lieutenants'
 * rounds and decisions (266-306) and the round loop with its Success line
 * (337-363), in count mode's canonical order with barrier-epoch delivery.
 * Rank r of instance i draws from the Philox stream keyed seed_base + i
 * (csrc/qba_internal.h; disjoint from the sampler's counters), so the result
 * is the one of montecarlo.run_host, field by field.  Instance i writes
 * 4 + 5*(n+1) int32 at out_dev + i*(4 + 5*(n+1)):
 *   {success, dishonest-rank bitmask, empty-V_i rank bitmask, status}, then
 *   per rank r = 0..n {decision (-1 on an empty V_i), V_r bitmask, accept,
 *   reject, sent}  (rank 0: zeros; the commander's V is 0).
 * status bit 0 = a mailbox overflowed, bit 1 = an RNG retry cap (64 words) was
 * hit; with a nonzero status every other field of the instance is 0.
 * 1 <= n_parties <= 15 and 0 <= n_dishonest <= n_parties, else QBA_EINVAL
 * (checked before ctx, which may then be NULL).  One launch per 2^20
 * instances; asynchronous on `stream`, allocates nothing. */
QBA_API int qba_protocol_batched(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                 int64_t n_instances, const int64_t *H_dev, const int64_t *C_dev,
                                 const int64_t *P_dev, int32_t *out_dev, qba_stream stream);

/* The fused Monte-Carlo path: from lists to decision rows in one kernel, with
 * no list buffer and no count tables in between.  Everything the rounds
 * consult of an instance's tables is a bitwise reduction over its
 * Q-correlated entries (L0 != L1, u = L1), so a wavefront ORs / ANDs the
 * entries into masks in LDS and runs the rounds on those.  Both calls write
 * exactly the rows of qba_protocol_batched on the tables of the same lists
 * (row layout and status bits as above), instance i under key seed_base + i
 * (mod 2^64) for the sampler over entries [0, count) and for the protocol
 * streams.  count == 0 is valid: every P_u is empty.
 * n_parties, n_dishonest (as qba_protocol_batched) and count < 2^31 are
 * checked before ctx, else QBA_EINVAL.  Asynchronous on `stream`, allocate
 * nothing.
 *
 * qba_montecarlo_sampled samples the entries itself, bit for bit those of
 * qba_sample_check_batched; it needs both resource programs of n_parties
 * compiled (QBA_ESTATE otherwise). */
QBA_API int qba_montecarlo_sampled(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                   int64_t n_instances, uint64_t count, int32_t *out_dev, qba_stream stream);

/* qba_montecarlo_lists reads injected byte rows in the layout of
 * qba_sample_check_batched (instance i at lists_dev + i*inst_stride, rows ld
 * apart; ld >= count, inst_stride >= (n+1)*ld, no alignment required) and
 * needs no program.  status bit 2 (value 4): a list value >= w at a
 * Q-correlated position -- the lists count mode cannot evaluate
 * (qba_last_stats) -- and the instance's other fields are 0. */
QBA_API int qba_montecarlo_lists(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                 int64_t n_instances, uint64_t count, const uint8_t *lists_dev, uint64_t ld,
                                 uint64_t inst_stride, int32_t *out_dev, qba_stream stream);

/* The launch shape of qba_montecarlo_sampled for the circuits of
 * qba_resource_compile's standard programs: wavefronts per workgroup, dynamic
 * LDS bytes of a workgroup, and the workgroups a CU's 160 KiB hold (DESIGN.md
 * section 13).  Host only; ctx is not needed. */
QBA_API int qba_montecarlo_shape(int n_parties, int *waves, int64_t *lds_bytes, int *wgs_per_cu);

/* A whole sizeL curve in one pass: every instance decided at each of the
 * checkpoints counts_host[0] < counts_host[1] < ... < counts_host[n_counts-1]
 * < 2^31, 1 <= n_counts <= QBA_MC_CURVE_MAX (counts_host[0] may be 0).  The
 * entries [0, c) of an instance are the first c of any larger count and the
 * masks are monotone reductions over them, so one pass over [0, c_max) stops
 * at each checkpoint, runs the rounds on the masks so far and writes a row:
 * instance i at checkpoint j writes 4 + 5*(n+1) int32 at
 *   out_dev + ((int64_t)j * n_instances + i) * (4 + 5*(n+1)),
 * word for word (status included) the row of qba_montecarlo_sampled /
 * qba_montecarlo_lists with count = counts_host[j].  In the lists form a
 * value >= w at Q-correlated position k gives status 4 in exactly the
 * checkpoints with counts_host[j] > k.
 * n_parties, n_dishonest and then the checkpoint list (pointer not NULL,
 * n_counts in range, strictly increasing, last < 2^31) are checked before
 * ctx, else QBA_EINVAL; the lists form needs ld >= counts_host[n_counts-1].
 * n_instances == 0 writes nothing.  The checkpoints travel by value in the
 * kernel arguments: counts_host may be reused when the call returns.
 * Asynchronous on `stream`, allocate and copy nothing, legal in a stream
 * capture.  The sampled form needs both resource programs (QBA_ESTATE). */
#define QBA_MC_CURVE_MAX 32
QBA_API int qba_montecarlo_curve_sampled(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                         int64_t n_instances, const uint32_t *counts_host, int n_counts,
                                         int32_t *out_dev, qba_stream stream);
QBA_API int qba_montecarlo_curve_lists(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                       int64_t n_instances, const uint32_t *counts_host, int n_counts,
                                       const uint8_t *lists_dev, uint64_t ld, uint64_t inst_stride,
                                       int32_t *out_dev, qba_stream stream);
/* The launch shape of qba_montecarlo_curve_sampled, as qba_montecarlo_shape:
 * each wavefront also holds its running masks, 2*w*(n+1) + 2 words (DESIGN.md
 * section 13.2), so some n run fewer wavefronts per workgroup. */
QBA_API int qba_montecarlo_curve_shape(int n_parties, int *waves, int64_t *lds_bytes, int *wgs_per_cu);
/* The launch shape of the program compiled for n_parties in ctx right now
 * (qba_resource_compile; QBA_ESTATE without both kinds), as the launcher of
 * qba_montecarlo_sampled (curve == 0) or qba_montecarlo_curve_sampled
 * (curve != 0) would choose it: *sampler 0 general alias tables, 1 canonical
 * tables, 2 closed form; *waves_compiled the wavefronts per workgroup that
 * sampler's kernel is built and launched with; *waves_run those of them that
 * take instances (fewer when the program's tables are not the size the kernel
 * was built for and another split of the CU's LDS keeps more wavefronts
 * resident); *lds_bytes and *wgs_per_cu as qba_montecarlo_shape.  For the
 * standard programs waves_run == waves_compiled and the three values are those
 * of qba_montecarlo_shape / qba_montecarlo_curve_shape.  Host only: launches
 * nothing, touches no device. */
QBA_API int qba_montecarlo_program_shape(qba_ctx *ctx, int n_parties, int curve, int *sampler, int *waves_compiled,
                                         int *waves_run, int64_t *lds_bytes, int *wgs_per_cu);

/* Qubit-flip noise: every one of the (n+1)*nQ
 * measured bits of an entry flips independently with probability
 * flip_q16 / 65536, 0 <= flip_q16 <= 65535, before anything looks at the
 * entry.  Entry e of the instance keyed key = seed_base + i draws
 *   word(t) = output word t % 4 of philox4x32-10(ctr = {e_lo, e_hi, t / 4,
 *             0x4E4F4953}, key = {key_lo, key_hi}),
 * folds the bits of k = flip_q16 from its lowest set bit j0 upwards into 64
 * bits r, starting from 0:  x = word(2s) | word(2s+1) << 32;  r = bit j0 + s of
 * k ? r | x : r & x  for s = 0 .. 15 - j0, and XORs (r >> 4g) & (w - 1) into
 * the value of group g = 0 .. n.  Values stay below w.  The flips of entry e
 * depend on (key, e, flip_q16) alone.
 *
 * The two noisy Monte-Carlo calls are qba_montecarlo_sampled and
 * qba_montecarlo_curve_sampled on the noisy entries, drawn and flipped inside
 * the kernel: checks, their order, row layout, asynchrony and capture legality
 * are those calls'; flip_q16 > 65535 is QBA_EINVAL, checked after the count(s)
 * and before ctx.  flip_q16 == 0 runs the noiseless kernel. */
QBA_API int qba_montecarlo_sampled_noisy(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                         int64_t n_instances, uint64_t count, uint32_t flip_q16, int32_t *out_dev,
                                         qba_stream stream);
QBA_API int qba_montecarlo_curve_sampled_noisy(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                               int64_t n_instances, const uint32_t *counts_host, int n_counts,
                                               uint32_t flip_q16, int32_t *out_dev, qba_stream stream);
/* The same flips XORed in place into byte rows in the layout of
 * qba_sample_check_batched (instance i at lists_dev + i*inst_stride, rows ld
 * apart, entries [0, count); that call's checks of them, after flip_q16 >
 * 65535, which is checked first): the noisy lists themselves, from
 * qba_sample_check_batched or qba_sample before it.  Bytes at columns >= count
 * are not touched.  flip_q16 == 0 launches nothing.  Needs no program.
 * Asynchronous on `stream`. */
QBA_API int qba_noise_apply_batched(qba_ctx *ctx, int n_parties, uint64_t seed_base, int64_t n_instances,
                                    uint64_t count, uint32_t flip_q16, uint8_t *lists_dev, uint64_t ld,
                                    uint64_t inst_stride, qba_stream stream);

/* Adversary policies: the five deciding calls with the
 * dishonest parties' behaviour read from a 32-bit policy word `adv`, last in
 * the argument list.
 *   bits [0:5)  acts   the actions a dishonest lieutenant draws from, per
 *                      destination: 0 maybe do not send, 1 replace the order,
 *                      2 clear P, 3 clear L (tfg.py:266-286), 4 relay unchanged
 *   bits [8:10) order  what action 1 writes: 0 randint(n + 1) (tfg.py), 1 the
 *                      smallest order in [0, w) other than the packet's
 *                      current v (no draw), 2 randint(w)
 *   bit  12     fresh  0: a mutation stays for the later destinations of the
 *                      same broadcast (tfg.py); 1: every destination starts
 *                      from the packet as it was handed to the broadcast
 *   bit  16     comm   the dishonest commander's split: 0 dest <= (n + 1) / 2
 *                      gets v1, else v2 (tfg.py:166-185); 1 even dest gets v1
 * Per destination a dishonest lieutenant draws a = randint(popcount(acts)),
 * always, and its action is the a-th set bit of acts in ascending order;
 * action 0 then draws randint(2), action 1 what `order` says, the others
 * nothing.  QBA_ADV_REFERENCE (0xF) is the rule of the calls without a policy
 * and gives their rows word for word.  Any other bit set, acts == 0 or order
 * == 3 is QBA_EINVAL, checked after the count(s) and flip_q16 and before ctx;
 * every other check, its order, the row layout, asynchrony and capture
 * legality are those of the call without `_adv`.  The two sampled calls take
 * flip_q16 as the _noisy calls do (0: no noise) and run one kernel either way.
 * Specification: montecarlo.AdversaryParty. */
#define QBA_ADV_REFERENCE 0xFu
QBA_API int qba_protocol_batched_adv(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                     int64_t n_instances, const int64_t *H_dev, const int64_t *C_dev,
                                     const int64_t *P_dev, int32_t *out_dev, qba_stream stream, uint32_t adv);
QBA_API int qba_montecarlo_lists_adv(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                     int64_t n_instances, uint64_t count, const uint8_t *lists_dev, uint64_t ld,
                                     uint64_t inst_stride, int32_t *out_dev, qba_stream stream, uint32_t adv);
QBA_API int qba_montecarlo_curve_lists_adv(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                           int64_t n_instances, const uint32_t *counts_host, int n_counts,
                                           const uint8_t *lists_dev, uint64_t ld, uint64_t inst_stride,
                                           int32_t *out_dev, qba_stream stream, uint32_t adv);
QBA_API int qba_montecarlo_sampled_adv(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                       int64_t n_instances, uint64_t count, uint32_t flip_q16, int32_t *out_dev,
                                       qba_stream stream, uint32_t adv);
QBA_API int qba_montecarlo_curve_sampled_adv(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                             int64_t n_instances, const uint32_t *counts_host, int n_counts,
                                             uint32_t flip_q16, int32_t *out_dev, qba_stream stream, uint32_t adv);

/* A grid of scenarios per checkpoint in one pass.  A
 * scenario is a pair (n_dishonest, adv).  The two calls are
 * qba_montecarlo_curve_sampled_adv / qba_montecarlo_curve_lists_adv deciding
 * every instance at every checkpoint under every scenario scen_host[0 ..
 * n_scen): the entries are sampled (or read) and distilled once, and at each
 * checkpoint the rounds run once per scenario on the same masks.  Instance i at
 * checkpoint j under scenario s writes 4 + 5*(n+1) int32 at
 *   out_dev + (((int64_t)j * n_scen + s) * n_instances + i) * (4 + 5*(n+1)),
 * word for word (status included) the row the _adv curve call writes at
 * counts_host[j] with n_dishonest = scen_host[s].n_dishonest and adv =
 * scen_host[s].adv: out_dev is [n_counts][n_scen][n_instances][4 + 5*(n+1)],
 * contiguous, and qba_montecarlo_tally takes it as n_counts * n_scen slices.
 * Under one key the traitors at n_dishonest = k are the first k of those at
 * k + 1 (a partial Fisher-Yates), so scenarios that differ in n_dishonest run
 * on nested traitor sets, the same lists and the same commander's order.
 * Checked in this order, each QBA_EINVAL: n_parties; the checkpoint list as
 * the curve calls check it; flip_q16 (sampled form); scen_host not NULL and
 * 1 <= n_scen <= QBA_MC_SWEEP_MAX; n_counts * n_scen <= QBA_MC_CURVE_MAX;
 * then scenario 0, 1, ...: n_dishonest in [0, n_parties], then adv as the _adv
 * calls check it; then ctx, n_instances and out_dev as those calls.  Equal
 * scenarios are legal and give equal slices.  Both host arrays travel by
 * value in the kernel arguments and may be reused when the call returns.
 * Asynchronous on `stream`, allocate and copy nothing, legal in a stream
 * capture.  The launch shape of the sampled form is
 * qba_montecarlo_curve_shape's.  Specification: montecarlo.sweep_host. */
#define QBA_MC_SWEEP_MAX 16
typedef struct {
  int32_t n_dishonest;
  uint32_t adv;
} qba_mc_scenario;
QBA_API int qba_montecarlo_sweep_sampled(qba_ctx *ctx, int n_parties, uint64_t seed_base, int64_t n_instances,
                                         const uint32_t *counts_host, int n_counts,
                                         const qba_mc_scenario *scen_host, int n_scen, uint32_t flip_q16,
                                         int32_t *out_dev, qba_stream stream);
QBA_API int qba_montecarlo_sweep_lists(qba_ctx *ctx, int n_parties, uint64_t seed_base, int64_t n_instances,
                                       const uint32_t *counts_host, int n_counts, const qba_mc_scenario *scen_host,
                                       int n_scen, const uint8_t *lists_dev, uint64_t ld, uint64_t inst_stride,
                                       int32_t *out_dev, qba_stream stream);

/* The result rows of the calls above reduced on the device (DESIGN.md section
 * 13.3).  rows_dev is [n_slices][n_instances][4 + 5*(n+1)] int32, contiguous:
 * what a curve call writes, or with n_slices == 1 a single-count call.
 * tally_dev is [n_slices][QBA_MC_TALLY_WORDS] int64.  The call ADDS to it and
 * never clears it (the caller zeroes it once): two calls on the halves of a
 * row block leave the words of one call on the whole block.  Words of a slice:
 *    0 runs (rows seen, status rows included)     1 successes (word 0 != 0)
 *    2 rows with word 2 != 0 (an empty V_i)        3 rows with status != 0
 *    4 bitwise OR of every status seen
 *    5 rows with bit 1 of the dishonest mask set (a dishonest commander)
 *    6 the successes among them
 *    7, 8, 9 sums of accept, reject, sent over ranks 1..n
 *   10 capture matches (below)                     11..14 reserved, untouched
 *   15 honest decisions equal to -1                16 + v those equal to v < 16
 * Honest: ranks 1..n whose bit in word 1 is clear.  A row with status != 0
 * counts in words 0, 3 and 4 only, whatever its other fields hold.
 * Capture: a row matches when a condition selected in `select` holds.  With
 * select != 0 every matching row adds 1 to word 10; with slot = the word's
 * value before that add, slot < capture_cap stores the row's global index
 * inst_base + i at capture_dev[slice * capture_cap + slot], so slots continue
 * across calls.  At most capture_cap matches in a slice: the stored set is
 * exactly the matches, in any order; more: word 10 is still exact and the
 * buffer holds capture_cap distinct matching indices.  With select == 0 or
 * capture_cap == 0 nothing is stored and capture_dev may be NULL; with
 * select == 0 word 10 does not move.
 * Checked before ctx, else QBA_EINVAL naming the argument: 1 <= n_parties <=
 * 15, 1 <= n_slices <= QBA_MC_CURVE_MAX, n_instances >= 0 (0 does nothing),
 * 0 <= select <= 7, capture_cap >= 0, tally_dev not NULL, rows_dev not NULL
 * when n_instances > 0, capture_dev not NULL when select != 0 and
 * capture_cap > 0.  Asynchronous on `stream`, allocates and copies nothing. */
#define QBA_MC_TALLY_WORDS 32
#define QBA_MC_SEL_FAILED   1   /* status == 0 and success == 0 */
#define QBA_MC_SEL_EMPTY_VI 2   /* status == 0 and word 2 != 0  */
#define QBA_MC_SEL_STATUS   4   /* status != 0 */
QBA_API int qba_montecarlo_tally(qba_ctx *ctx, int n_parties, const int32_t *rows_dev,
                                 int64_t n_instances, int n_slices, uint64_t inst_base,
                                 int64_t *tally_dev, int select, int64_t *capture_dev,
                                 int64_t capture_cap, qba_stream stream);

/* A transcript of chosen runs.  The two calls re-run
 * the instances keyed seed_base + idx_dev[j] (mod 2^64), j in [0, n_idx), as
 * qba_montecarlo_sampled_adv / qba_montecarlo_lists_adv decide them (the lists
 * form: slot j reads lists_dev + j * inst_stride, and flip_q16 flips its
 * entries as the sampled form's) and write per slot j
 *   rows_dev   + j * (4 + 5*(n+1))        the result row, word for word the
 *                                         decision call's for that key
 *   counts_dev + j * (n+1)                int32: the events rank r = 0..n
 *                                         produced (rank 0: none)
 *   events_dev + ((j * (n+1) + r) * cap) * 2   uint32 {head, pkt}: the first
 *                                         min(count, cap) events of rank r, in
 *                                         the order the rank produced them
 * and nothing else: events past `cap` are counted, not stored.  A row with a
 * nonzero status has counts 0.
 *   head = kind [0:3) | round [3:8) | peer [8:12) | slot [12:17) | code [17:21)
 *          | len [21:26), every other bit 0; round 0 is the commander's epoch
 *   QBA_EV_RECV    a packet a lieutenant processes (the commander's: peer 1,
 *                  slot 0, round 0; then every mailbox packet of the rounds):
 *                  peer the source, slot the mailbox slot read, len the lists
 *                  after the own tuple joined, code 0 accepted and v added to
 *                  V_i; 1, 2, 3 the first of Cond1, Cond2, Cond3 (tfg.py:87-98)
 *                  that fails; 4 consistent but v already in V_i; 5 consistent
 *                  and new but len != round + 1.  Codes 0, 4, 5 are the row's
 *                  accept, codes 1-3 its reject.
 *   QBA_EV_SEND    a destination a broadcast visits, the commander's n - 1
 *                  sends included (round 0): peer the destination, code the
 *                  drawn action 0..4 or QBA_EV_HONEST, len the lists of the
 *                  packet sent, slot the mailbox slot written,
 *                  QBA_EV_SLOT_MUTED for a send action 0 suppressed,
 *                  QBA_EV_SLOT_FULL for one dropped on a full mailbox.  Events
 *                  with slot < 30 are the row's sent.
 *   QBA_EV_DECIDE  the last event of every rank 1..n: pkt the decision as
 *                  uint32, len popcount(V_i)
 *   pkt (RECV: as read; SEND: after the traitor's mutation) = v [0:4) | P's u
 *   [4:8) | P cleared [8] | the tuples' u [9:13) | an empty tuple present [13] |
 *   mask of the tuples' representatives [16:32), with P's u zero under the
 *   cleared bit and the tuples' u zero under an empty mask.
 * n_match_dev (NULL: none): a device int64; slot j does nothing when j >=
 * min(n_idx, *n_match_dev), read when the kernel runs -- a tally's capture row
 * and its word 10 feed the call with no host round trip.
 * Checked in this order, each QBA_EINVAL: n_parties; count < 2^31; flip_q16 <=
 * 65535; n_dishonest in [0, n_parties]; adv as the _adv calls check it; n_idx
 * >= 0 and idx_dev not NULL when n_idx > 0; 1 <= cap <= QBA_TRACE_CAP_MAX;
 * rows_dev, counts_dev, events_dev not NULL when n_idx > 0; ctx; then (lists
 * form) lists_dev, ld and inst_stride as qba_montecarlo_lists.  Asynchronous on
 * `stream`, allocate and copy nothing, legal in a stream capture.  The launch
 * shape of the sampled form is qba_montecarlo_shape's.  Specification:
 * montecarlo.trace_host. */
#define QBA_EV_RECV 1u
#define QBA_EV_SEND 2u
#define QBA_EV_DECIDE 3u
#define QBA_EV_HONEST 7u
#define QBA_EV_SLOT_FULL 30u
#define QBA_EV_SLOT_MUTED 31u
#define QBA_TRACE_CAP_MAX 4096
QBA_API int qba_montecarlo_trace_sampled(qba_ctx *ctx, int n_parties, uint64_t seed_base, const int64_t *idx_dev,
                                         int64_t n_idx, const int64_t *n_match_dev, uint64_t count, int n_dishonest,
                                         uint32_t adv, uint32_t flip_q16, int64_t cap, int32_t *rows_dev,
                                         int32_t *counts_dev, uint32_t *events_dev, qba_stream stream);
QBA_API int qba_montecarlo_trace_lists(qba_ctx *ctx, int n_parties, uint64_t seed_base, const int64_t *idx_dev,
                                       int64_t n_idx, const int64_t *n_match_dev, uint64_t count, int n_dishonest,
                                       uint32_t adv, uint32_t flip_q16, int64_t cap, const uint8_t *lists_dev,
                                       uint64_t ld, uint64_t inst_stride, int32_t *rows_dev, int32_t *counts_dev,
                                       uint32_t *events_dev, qba_stream stream);

/* The transcript on a network that loses packets:
 * the two trace calls above with the network word `net` of the _net curve
 * calls appended after `stream`.  They re-run the instances as
 * qba_montecarlo_curve_sampled_net / qba_montecarlo_curve_lists_net decide them
 * at the one checkpoint `count`, and write the rows of those calls word for
 * word, with the events above and two more:
 *   QBA_EV_SLOT_LOST   the `slot` of a SEND event whose packet was handed to a
 *                      lossy link and lost in flight.  Such a send counts in
 *                      the row's sent and advances the link's seq; it takes no
 *                      mailbox slot, so the next send to that destination in
 *                      that round gets the slot this one would have had.  29
 *                      is below 30: SEND events with slot < 30 are still the
 *                      row's sent.  code is the drawn action or QBA_EV_HONEST,
 *                      len and pkt those of the packet as handed over, after a
 *                      traitor's mutation.  Under cmd the commander's round-0
 *                      SEND carries it too.
 *   QBA_EV_NO_PACKET   the `code` of the one RECV event of a lieutenant whose
 *                      commander packet was lost: round 0, peer 1, slot 0,
 *                      len 0, pkt 0.  Neither an accept nor a reject, as in the
 *                      row.  A lost lieutenant-to-lieutenant packet leaves no
 *                      event at the receiver.
 * A send that action 0 suppresses stays QBA_EV_SLOT_MUTED: it is not handed to
 * the link and seq does not move.  Every other event is bit for bit what the
 * calls above define, and with net == 0 the calls write their rows, counts and
 * events word for word.
 * The checks are those calls' in their order, with net checked as the _net
 * curve calls check it right after adv (before n_idx and idx_dev).
 * Asynchronous on `stream`, allocate and copy nothing, legal in a stream
 * capture; the launch shape of the sampled form is qba_montecarlo_shape's.
 * Specification: montecarlo.trace_net_host. */
#define QBA_EV_SLOT_LOST 29u
#define QBA_EV_NO_PACKET 6u
QBA_API int qba_montecarlo_trace_sampled_net(qba_ctx *ctx, int n_parties, uint64_t seed_base,
                                             const int64_t *idx_dev, int64_t n_idx, const int64_t *n_match_dev,
                                             uint64_t count, int n_dishonest, uint32_t adv, uint32_t flip_q16,
                                             int64_t cap, int32_t *rows_dev, int32_t *counts_dev,
                                             uint32_t *events_dev, qba_stream stream, uint32_t net);
QBA_API int qba_montecarlo_trace_lists_net(qba_ctx *ctx, int n_parties, uint64_t seed_base, const int64_t *idx_dev,
                                           int64_t n_idx, const int64_t *n_match_dev, uint64_t count,
                                           int n_dishonest, uint32_t adv, uint32_t flip_q16, int64_t cap,
                                           const uint8_t *lists_dev, uint64_t ld, uint64_t inst_stride,
                                           int32_t *rows_dev, int32_t *counts_dev, uint32_t *events_dev,
                                           qba_stream stream, uint32_t net);

/* ---- (A5-A8) checks, exact-order mode (bit-exact protocol parity) --------------- */
/* isQCorrList = {k : Li[k] != Lc[k]} (tfg.py:327) as ascending indices.
 * *count_host receives the number found; at most `cap` are written. Synchronous. */
QBA_API int qba_isq_indices(qba_ctx *ctx, const uint8_t *li_dev, const uint8_t *lc_dev, uint64_t count,
                    int64_t *idx_dev, int64_t cap, int64_t *count_host, qba_stream stream);
/* P = {x in order : Lc[x] == v} keeping the order of `order` (tfg.py:182).
 * Every index must lie in [0, lc_len) (QBA_EINVAL otherwise; nothing outside
 * Lc is read).  Synchronous. */
QBA_API int qba_select_eq(qba_ctx *ctx, const int64_t *order_dev, int64_t m, const uint8_t *lc_dev,
                  uint64_t lc_len, int64_t v, int64_t *out_dev, int64_t *count_host, qba_stream stream);
/* Host-pointer forms of the two (the protocol host's calls; synchronous):
 * idx_host / out_host receive the selected indices.  Inputs of at most 16384
 * items run as ONE single-workgroup launch through zero-copy pinned staging
 * (no copies), larger ones through the device compaction and one D2H. */
QBA_API int qba_isq_indices_host(qba_ctx *ctx, const uint8_t *li_dev, const uint8_t *lc_dev, uint64_t count,
                                 int64_t *idx_host, int64_t cap, int64_t *count_host, qba_stream stream);
QBA_API int qba_select_eq_host(qba_ctx *ctx, const int64_t *order_host, int64_t m, const uint8_t *lc_dev,
                               uint64_t lc_len, int64_t v, int64_t *out_host, int64_t *count_host,
                               qba_stream stream);
/* tuple(Li[j] for j in P) in the given order (tfg.py:189, 291). */
QBA_API int qba_gather(qba_ctx *ctx, const uint8_t *li_dev, uint64_t list_len, const int64_t *idx_dev,
               int64_t m, int64_t *out_dev, qba_stream stream);
/* consistent(v, L, w) conditions 2 and 3 (tfg.py:93-98) over m equal-length
 * tuples stored row-major [m][len] (Cond1 and the empty-L StopIteration stay
 * on the host).  *ok_host = 1 if consistent.  Synchronous. */
QBA_API int qba_consistent(qba_ctx *ctx, const int64_t *tuples_dev, int64_t m, int64_t len, int64_t v,
                   int64_t w, int32_t *ok_host, qba_stream stream);

/* One received packet in ONE launch (tfg.py:189-192 in step 3a, 291-294 in
 * step 3b): gathers the receiver's own tuple Li[j] for j in order (its set-
 * iteration order of P) and evaluates Cond2/Cond3 of consistent(v, L | {own},
 * w) (tfg.py:93-98) over the m received tuples of length len, with the set's
 * de-duplication of own.  stage_dev = [order (len) | tuples (m x len)].
 * out_dev (len + 3 + m int64): own tuple, then bad-index flag, received-
 * tuple violation flag, own Cond2 violation flag, and per received tuple the
 * number of positions equal to own; consistent <=> all flags 0 and every
 * count in {0, len} (the host adds Cond1).  Asynchronous on `stream`. */
QBA_API int qba_check_packet(qba_ctx *ctx, const uint8_t *li_dev, uint64_t list_len,
                             const int64_t *stage_dev, int64_t m, int64_t len, int64_t v, int64_t w,
                             int64_t *out_dev, qba_stream stream);

/* Exact-order consistent(v, L, w) (tfg.py:87-98) over m tuples gathered on
 * the device (SURVEY.md §8(b) qba_check_gather): T_a[k] = lists[party[a]][
 * idx[a][k]] (lists [rows][ld], list_len valid entries per row; idx [m][len]
 * row-major).  L is a set: identical tuples collapse (tfg.py:209, 240, 260).
 * *ok_dev = 1 consistent, 0 not, -1 an index or party out of range (nothing
 * outside the lists is read).  1 <= m <= 64 (m = 0 is the reference's
 * StopIteration, tfg.py:90: QBA_EINVAL).  Asynchronous on `stream`. */
QBA_API int qba_check_gather(qba_ctx *ctx, const uint8_t *lists_dev, uint64_t ld, int rows, uint64_t list_len,
                             const int64_t *idx_dev, const int32_t *party_dev, int64_t m, int64_t len,
                             int64_t v, int64_t w, int32_t *ok_dev, qba_stream stream);

/* Synchronous host-pointer form of qba_check_packet (the protocol's
 * per-packet call: one H2D through the context's pinned staging, one launch,
 * one D2H, one sync).  stage_host / out_host as above, in host memory. */
QBA_API int qba_check_packet_host(qba_ctx *ctx, const uint8_t *li_dev, uint64_t list_len,
                                  const int64_t *stage_host, int64_t m, int64_t len, int64_t v, int64_t w,
                                  int64_t *out_host, qba_stream stream);

/* A whole round of received packets (tfg.py:337-348 -> 289-294) in ONE host
 * round trip: k stages concatenated in stage_host (packet i: len_i*(m_i+1)
 * int64 = [order | rows], desc[i] = {m_i, len_i, v_i}); out_host receives the
 * k outputs concatenated (packet i: len_i + 3 + m_i int64, as
 * qba_check_packet).  One H2D, k launches, one D2H, one sync. */
QBA_API int qba_check_packets_host(qba_ctx *ctx, const uint8_t *li_dev, uint64_t list_len,
                                   const int64_t *stage_host, const int64_t *desc, int64_t k, int64_t w,
                                   int64_t *out_host, qba_stream stream);

/* ---- host-only: the exact-order protocol's set semantics (no device) -------------- */
/* Iteration order of CPython 3.10's set(keys) for int64 keys inserted in the
 * given order (tfg.py:240 P = set(buff); tfg.py:182 and 327 set
 * comprehensions): order_out[*n_out] = the distinct keys in slot order.
 * Replaces building the Python set and reading it back (tfg.py:189, 209, 291
 * iterate it).  order_out needs room for n keys. */
QBA_API int qba_host_pyset_order(const int64_t *keys, int64_t n, int64_t *order_out, int64_t *n_out);
/* hash(tuple(vals)) of CPython 3.10 (tuplehash over int elements): the set of
 * tuples L (tfg.py:189, 260, 291) orders and de-duplicates by it. */
QBA_API int qba_host_pytuple_hash(const int64_t *vals, int64_t n, int64_t *hash_out);

/* ---- wire-compatible codec (rawS layout, tfg.py:81-84, 128-129, 142-161) -------- */
QBA_API int qba_bits_to_values(qba_ctx *ctx, const int64_t *raw_dev, uint64_t count, int nq,
                       uint8_t *values_dev, qba_stream stream);
QBA_API int qba_values_to_bits(qba_ctx *ctx, const uint8_t *values_dev, uint64_t count, int nq,
                       int64_t *raw_dev, qba_stream stream);
/* rawS of a run (tfg.py:81-84, as rank 0 ships it at tfg.py:142-145): rows
 * [0, rows) of a lists matrix encoded to raw_host[rows][count*nq].  Sync. */
QBA_API int qba_lists_to_bits_host(qba_ctx *ctx, const uint8_t *lists_dev, uint64_t ld, int rows,
                                   uint64_t count, int nq, int64_t *raw_host, qba_stream stream);
/* measure_to_ints of a received row (tfg.py:158, 161) straight from the
 * receive buffer in host memory to a device list.  raw_host may be reused
 * as soon as the call returns; the decode is ordered on `stream` (small rows
 * are read from zero-copy staging without waiting; larger ones wait). */
QBA_API int qba_bits_to_values_host(qba_ctx *ctx, const int64_t *raw_host, uint64_t count, int nq,
                                    uint8_t *values_dev, qba_stream stream);

/* ---- multi-GPU: the count all-reduce over RCCL ---------------- */
/* The sizeL shards of one run live on G GPU-owner ranks; their int64 count
 * buffers [H | C | P] are summed with ONE all-reduce.  This replaces nothing
 * in tfg.py (the reference is single-process per party and never shards a
 * list); it is what a non-torch caller (the mpiexec host) uses where the
 * torch path calls torch.distributed.all_reduce.  Bootstrap: rank 0 calls
 * qba_rccl_unique_id, ships the 128 bytes to the other owners (e.g. over
 * MPI), every owner calls qba_rccl_init.  librccl is opened on first use;
 * QBA_EUNSUPPORTED without it. */
QBA_API int qba_rccl_unique_id(uint8_t *id_host /* [128] */);
QBA_API int qba_rccl_init(qba_ctx *ctx, const uint8_t *id_host, int nranks, int rank);
/* In place, sum over the communicator's ranks; asynchronous on `stream`. */
QBA_API int qba_allreduce_i64(qba_ctx *ctx, int64_t *buf_dev, int64_t count, qba_stream stream);

/* ---- helpers exported for tests ------------------------------------------------- */
/* Vose alias table over k probabilities (host): thr[i] in [0, 2^32] (2^32 =
 * always keep column i), alias[i] = column taken otherwise. */
QBA_API int qba_alias_build(const double *prob_host, int32_t k, uint64_t *thr_host, int32_t *alias_host);
/* Philox4x32-10 on the device for KATs: out[4*i..] = philox(ctr_i, key). */
QBA_API int qba_philox_dev(qba_ctx *ctx, const uint32_t *ctr_dev, int64_t n, uint64_t key,
                   uint32_t *out_dev, qba_stream stream);
/* Test seam: the launch-shape knobs the GPU tests use to reach the list
 * kernels' rare paths on small inputs (the library reads no environment
 * variable).  chunk_entries: entries per list-kernel launch (0 = the shipped
 * 2^31; else 4 .. 2^31, rounded down to a multiple of 4) -- chunk splits;
 * pb_min_entries: launches from this many entries count n = 11 in pair bins
 * (< 0 = the shipped 2^24); list_grid: > 0 caps the list kernels' workgroups
 * and forces pair bins, each workgroup taking up to 2^23 entries per launch
 * -- pair-bin wraps and their recount (0 = off).  Flushes a pending deferred
 * reduction first.  Results are bit-identical under every setting. */
QBA_API int qba_test_set_knobs(qba_ctx *ctx, uint64_t chunk_entries, int64_t pb_min_entries, int list_grid);

/* ---- colluding traitors -------------------------------- */
/* The two _adv curve calls with a second 32-bit word, `coal`, last: the
 * dishonest lieutenants withhold accepted packets from honest ones and inject
 * them in a late round R, padded with the coalition's tuples to the length that
 * round demands.
 *   bit  0       on       1: the traitors collude
 *   bits [4:6)   when     R: 0 n_dishonest + 1 (the last round), 1
 *                         max(1, n_dishonest) (the last round whose acceptances
 *                         are relayed)
 *   bits [8:10)  targets  the honest lieutenants packets are withheld from and
 *                         injected to: 0 all, 1 even ranks, 2 the lowest-ranked
 *   bit  12      starve   a dishonest commander sends v1 to every honest and v2
 *                         to every dishonest lieutenant
 * coal == 0 is no coalition: the call writes the rows of the _adv curve call
 * word for word.  Any other bit, when > 1, targets == 3 or a field set without
 * `on` is QBA_EINVAL (the message names the field), checked right after `adv`
 * and before ctx.  The out layout, every other check and its order, asynchrony
 * and capture legality are those of the _adv curve calls; a single sizeL is a
 * curve of one checkpoint; qba_montecarlo_tally takes the rows as they are.
 * The sampled kernel holds a wavefront's hold lists in LDS beside what the
 * curve kernels hold: qba_montecarlo_coal_shape reports its launch shape as
 * qba_montecarlo_curve_shape does theirs.  Specification:
 * montecarlo.CoalitionParty. */
QBA_API int qba_montecarlo_curve_sampled_coal(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                              int64_t n_instances, const uint32_t *counts_host, int n_counts,
                                              uint32_t flip_q16, int32_t *out_dev, qba_stream stream, uint32_t adv,
                                              uint32_t coal);
QBA_API int qba_montecarlo_curve_lists_coal(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                            int64_t n_instances, const uint32_t *counts_host, int n_counts,
                                            const uint8_t *lists_dev, uint64_t ld, uint64_t inst_stride,
                                            int32_t *out_dev, qba_stream stream, uint32_t adv, uint32_t coal);
QBA_API int qba_montecarlo_coal_shape(int n_parties, int *waves, int64_t *lds_bytes, int *wgs_per_cu);

/* ---- lossy links ---------------------------------------- */
/* The two _adv curve calls with a second 32-bit word, `net`, last: packets are
 * lost in flight.
 *   bits [0:16)  drop_q16  a packet on a lossy link is lost with probability
 *                          drop_q16 / 65536
 *   bit  16      cmd       1: the commander's n - 1 sends of epoch 0 cross a
 *                          lossy link too; 0: only lieutenant-to-lieutenant
 *                          packets do
 * net == 0 is the perfect network: the call writes the rows of the _adv curve
 * call word for word.  Any other bit, or cmd with drop_q16 == 0, is QBA_EINVAL
 * (the message names the field), checked right after `adv` and before ctx.
 *
 * Loss is a pure function of the packet, not a stream position: no existing
 * draw moves.  A packet is identified by the instance key
 * key = seed_base + i, the epoch e in which it is sent (0 for the commander's
 * epoch, including the relays lieutenants make after step 3a; r for round r),
 * src, dest, and seq = the number of packets src has already handed to the
 * link towards dest in epoch e (sends suppressed by action 0 are not handed
 * over and do not count).  It is lost iff
 *   (word(seq & 3) of philox4x32-10(ctr = {e, src | dest << 8, seq >> 2, 0x4E455457},
 *                                   key = {key_lo, key_hi}) & 0xFFFF) < drop_q16.
 * Counter word 3, 0x4E455457, is disjoint from the sampler's (0 or 1), the
 * protocol's (0x51424150) and the noise stream's (0x4E4F4953).  The test
 * applies to what the sender actually hands over, after a traitor's mutation,
 * whether the sender is honest or not.
 *
 * The sender cannot tell: the row's `sent` counts the packet and seq advances.
 * The packet takes no mailbox slot (the w-slot bound per (dest, src, round),
 * its bounds check and status bit 0 hold), and the receiver never sees it: no
 * accept, no reject, no V_i change, no relay.  Under cmd a lieutenant whose
 * commander packet is lost skips step 3a altogether and takes part in the
 * rounds with an empty V_i.  An honest lieutenant that ends with an empty V_i
 * decides -1 (row word 2, tally words 2 and 15), as before.
 *
 * The out layout, status bits, every other check and its order, asynchrony and
 * capture legality are those of the _adv curve calls; the calls allocate and
 * copy nothing; a single sizeL is a curve of one checkpoint;
 * qba_montecarlo_tally takes the rows as they are.  The kernels hold no LDS
 * beyond the _adv curve kernels': qba_montecarlo_curve_shape is their launch
 * shape.  Specification: montecarlo.NetParty, montecarlo.net_lost. */
QBA_API int qba_montecarlo_curve_sampled_net(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                             int64_t n_instances, const uint32_t *counts_host, int n_counts,
                                             uint32_t flip_q16, int32_t *out_dev, qba_stream stream, uint32_t adv,
                                             uint32_t net);
QBA_API int qba_montecarlo_curve_lists_net(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                           int64_t n_instances, const uint32_t *counts_host, int n_counts,
                                           const uint8_t *lists_dev, uint64_t ld, uint64_t inst_stride,
                                           int32_t *out_dev, qba_stream stream, uint32_t adv, uint32_t net);

/* A grid of (n_dishonest, adv, net) scenarios per checkpoint in one pass
 * (DESIGN.md section 13.12): the sweep calls with a network word in every
 * scenario.  The two calls are qba_montecarlo_curve_sampled_net /
 * qba_montecarlo_curve_lists_net deciding every instance at every checkpoint
 * under every scenario scen_host[0 .. n_scen): the entries are sampled (or
 * read) and distilled once, and at each checkpoint the rounds run once per
 * scenario on the same masks.  Instance i at checkpoint j under scenario s
 * writes 4 + 5*(n+1) int32 at
 *   out_dev + (((int64_t)j * n_scen + s) * n_instances + i) * (4 + 5*(n+1)),
 * word for word (status included) the row the _net curve call writes at
 * counts_host[j] with scenario s's n_dishonest, adv and net; at net == 0 that
 * is also the sweep call's slice.  out_dev is
 * [n_counts][n_scen][n_instances][4 + 5*(n+1)], contiguous, and
 * qba_montecarlo_tally takes it as n_counts * n_scen slices.
 * Under one key the lists, the traitor draw and the commander's order are the
 * same in every scenario, and a packet's loss word does not depend on
 * drop_q16: a packet lost at drop_q16 = K is lost at every K' >= K, so
 * scenarios that differ in drop_q16 alone lose nested sets of the packets they
 * have in common.
 * Checked in this order, each QBA_EINVAL: n_parties; the checkpoint list as
 * the curve calls check it; flip_q16 (sampled form); scen_host not NULL and
 * 1 <= n_scen <= QBA_MC_GRID_MAX; n_counts * n_scen <= QBA_MC_CURVE_MAX; then
 * scenario 0, 1, ...: n_dishonest in [0, n_parties], then adv as the _adv calls
 * check it, then net as the _net calls check it (the message names the first
 * bad scenario by index and the field); then ctx, n_instances and out_dev as
 * those calls.  Equal scenarios are legal and give equal slices.  Both host
 * arrays travel by value in the kernel arguments and may be reused when the
 * call returns.  Asynchronous on `stream`, allocate and copy nothing, legal in
 * a stream capture.  The launch shape of the sampled form is
 * qba_montecarlo_curve_shape's.  Specification: montecarlo.grid_host. */
#define QBA_MC_GRID_MAX 16
typedef struct {
  int32_t n_dishonest;
  uint32_t adv;
  uint32_t net;
} qba_mc_grid_scenario;
QBA_API int qba_montecarlo_grid_sampled(qba_ctx *ctx, int n_parties, uint64_t seed_base, int64_t n_instances,
                                        const uint32_t *counts_host, int n_counts,
                                        const qba_mc_grid_scenario *scen_host, int n_scen, uint32_t flip_q16,
                                        int32_t *out_dev, qba_stream stream);
QBA_API int qba_montecarlo_grid_lists(qba_ctx *ctx, int n_parties, uint64_t seed_base, int64_t n_instances,
                                      const uint32_t *counts_host, int n_counts,
                                      const qba_mc_grid_scenario *scen_host, int n_scen, const uint8_t *lists_dev,
                                      uint64_t ld, uint64_t inst_stride, int32_t *out_dev, qba_stream stream);

/* ---- noise profiles ------------------------------------- */
/* The two _adv curve calls with a noise profile in place of flip_q16: a flip
 * rate per list row and depolarised entries.
 *   rates_host[g], g = 0 .. n_parties   every measured bit of list row g flips
 *                          with probability rates_host[g] / 65536 (row 0: the
 *                          commander's list, row 1: Lc, row g >= 2: lieutenant g)
 *   depol_q16              with probability depol_q16 / 65536 the whole entry
 *                          is depolarised: a uniform value below w is XORed
 *                          into every row's value at once
 * Entry e of the instance keyed key = seed_base + i gets 64 bits r; row g's
 * value is XORed with (r >> 4g) & (w - 1), where the flip_q16 calls XOR theirs.
 * With word(t) = output word t % 4 of philox4x32-10(ctr = {e_lo, e_hi, t / 4,
 * 0x4E4F4953}, key = {key_lo, key_hi}), the noise stream of the flip_q16 calls:
 *   r = 0
 *   if any rate is not 0:
 *     j0 = the lowest set bit of any rate
 *     for s = 0 .. 15 - j0:
 *       x = word(2s) | word(2s+1) << 32
 *       M_s = nibble g is 0xF where bit (j0 + s) of rates_host[g] is set, else 0
 *       r = ((r | x) & M_s) | ((r & x) & ~M_s)
 *   if depol_q16 != 0:
 *     d = philox4x32-10(ctr = {e_lo, e_hi, 8, 0x4E4F4953}, key)
 *     if (d[0] & 0xFFFF) < depol_q16:  r ^= d[2] | d[3] << 32
 * Every bit of row g's mask is 1 with probability exactly rates_host[g] /
 * 65536 and a row with rate 0 keeps its values.  With every rate equal to k
 * and depol_q16 == 0 the rows are those of the _adv curve call at flip_q16 = k
 * word for word; the all-zero profile draws nothing and gives that call's rows
 * at flip_q16 = 0.  Noise never raises status bit 2.
 *
 * Checked right after `adv` and before ctx, each QBA_EINVAL naming the field:
 * n_rates == n_parties + 1, rates_host not NULL, depol_q16 <= 65535.  The out
 * layout, status bits, every other check and its order, asynchrony and capture
 * legality are those of the _adv curve calls; the profile travels by value in
 * the kernel arguments, rates_host may be reused when the call returns, and the
 * calls allocate and copy nothing; a single sizeL is a curve of one checkpoint;
 * qba_montecarlo_tally takes the rows as they are.  The kernels hold no LDS
 * beyond the _adv curve kernels': qba_montecarlo_curve_shape is their launch
 * shape.  Specification: montecarlo.noise_masks_profile. */
QBA_API int qba_montecarlo_curve_sampled_nprof(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                               int64_t n_instances, const uint32_t *counts_host, int n_counts,
                                               int32_t *out_dev, qba_stream stream, uint32_t adv,
                                               const uint16_t *rates_host, int n_rates, uint32_t depol_q16);
QBA_API int qba_montecarlo_curve_lists_nprof(qba_ctx *ctx, int n_parties, int n_dishonest, uint64_t seed_base,
                                             int64_t n_instances, const uint32_t *counts_host, int n_counts,
                                             const uint8_t *lists_dev, uint64_t ld, uint64_t inst_stride,
                                             int32_t *out_dev, qba_stream stream, uint32_t adv,
                                             const uint16_t *rates_host, int n_rates, uint32_t depol_q16);
/* The masks of a profile XORed in place into lists in the layout of
 * qba_sample_check_batched (qba_noise_apply_batched with a profile): the
 * profile is checked first, as above, then that call's arguments as it checks
 * them.  Asynchronous, allocates and copies nothing, legal in a stream
 * capture; needs no program. */
QBA_API int qba_noise_profile_apply(qba_ctx *ctx, int n_parties, uint64_t seed_base, int64_t n_instances,
                                    uint64_t count, const uint16_t *rates_host, int n_rates, uint32_t depol_q16,
                                    uint8_t *lists_dev, uint64_t ld, uint64_t inst_stride, qba_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* QBA_H */
