// qba_lists.h -- interface between the list-kernel dispatch (qba_lists.hip)
// and the per-n kernel instantiations (qba_lists_inst.hip, one object per n:
// the templates in qba_lists_kern.h are compiled 15 times in parallel).
#pragma once

#include "qba_internal.h"
#include "qba_noise.h"

struct QbaLaunch {
  int n;
  int mode;
  const QbaProgramSet *ps;
  uint64_t seed, first, count;
  uint8_t *lists;
  uint64_t ld;
  int64_t *H, *C, *P, *stats;
  int accumulate;
  hipStream_t stream;
  int stats_accumulate;
  int packed;  // nibble rows (qba.h "packed lists"): ld is the packed row stride in bytes
  int defer;   // MODE 1: reduction deferred to the next deferred call / qba_flush_deferred
};

struct QbaBatch {
  int n;
  const QbaProgramSet *ps;
  uint64_t seed_base;
  int64_t n_inst;
  uint64_t count;
  uint8_t *lists;
  uint64_t ld, inst_stride;
  int64_t *H, *C, *P;
  hipStream_t stream;
  int packed;      // nibble rows: ld / inst_stride in bytes of packed rows
  QbaNoise noise;  // read by the noisy kernels alone (qba_sample_check_batched*_noisy with flip_q16 > 0)
};

// qba_montecarlo_sampled and qba_montecarlo_curve_sampled (qba_mc_kern.h);
// fields have the kernel arguments' types.  The single-count call is the one
// with one checkpoint and `curve` 0, which picks its kernel.  `noise` is read by
// the noisy kernels alone (qba_montecarlo_*_noisy with flip_q16 > 0).
struct QbaMc {
  const char *who;  // the exported function, for messages
  const QbaProgramSet *ps;
  uint64_t seed_base;
  int64_t n_inst;
  int n_dis;
  int32_t *out;
  hipStream_t stream;
  QbaMcCounts counts;
  int curve;
  QbaNoise noise;
  uint32_t adv;  // the policy word, read by the _adv kernels alone (qba_montecarlo_*_adv), which take
                 // `noise` at run time: steps == 0 is no noise
  int use_adv;
  QbaMcScen scen;  // read by the sweep kernel alone (qba_montecarlo_sweep_sampled), which takes no n_dis / adv
  uint32_t coal;   // the coalition word, read by the coalition kernel alone (qba_montecarlo_curve_sampled_coal)
  uint32_t net;    // the network word, read by the lossy-network kernel alone (qba_montecarlo_curve_sampled_net)
  QbaMcGrid grid;  // read by the grid kernel alone (qba_montecarlo_grid_sampled), which takes no n_dis / adv / net
};

template <int NP>
int qba_launch_lists(qba_ctx *ctx, const QbaLaunch &L);
// Launch the pending deferred reduction (if any) on its stream; a later launch
// on stream `next` that reuses the slab then waits for it.
int qba_flush_pending(qba_ctx *ctx, hipStream_t next);
template <int NP>
int qba_launch_batched(qba_ctx *ctx, const QbaBatch &B);
// the same through the noisy kernels (qba_lists_noise_inst.hip)
template <int NP>
int qba_launch_batched_noisy(qba_ctx *ctx, const QbaBatch &B);
template <int NP>
int qba_launch_mc(qba_ctx *ctx, const QbaMc &M);
// the same through the noisy kernels (qba_mc_noise_inst.hip)
template <int NP>
int qba_launch_mc_noisy(qba_ctx *ctx, const QbaMc &M);
// the same through the adversary-policy kernels (qba_mc_adv_inst.hip)
template <int NP>
int qba_launch_mc_adv(qba_ctx *ctx, const QbaMc &M);
// the curve under every scenario of M.scen, through the sweep kernel (qba_mc_sweep_inst.hip)
template <int NP>
int qba_launch_mc_sweep(qba_ctx *ctx, const QbaMc &M);
// the curve under a policy and a coalition word, through the coalition kernel (qba_mc_coal_inst.hip)
template <int NP>
int qba_launch_mc_coal(qba_ctx *ctx, const QbaMc &M);
// qba_montecarlo_coal_shape (qba_mc_coal_inst.hip)
template <int NP>
void qba_mc_coal_shape_n(int *waves, int64_t *lds, int *wgs);
// the curve under a policy and a network word, through the lossy-network kernel (qba_mc_net_inst.hip)
template <int NP>
int qba_launch_mc_net(qba_ctx *ctx, const QbaMc &M);
// the curve under every scenario of M.grid, through the grid kernel (qba_mc_grid_inst.hip)
template <int NP>
int qba_launch_mc_grid(qba_ctx *ctx, const QbaMc &M);
// the curve under a policy and a noise profile (qba_noise_profile.h), through the noise-profile kernel
// (qba_mc_nprof_inst.hip); M.noise is not read
struct QbaNoiseProfile;
template <int NP>
int qba_launch_mc_nprof(qba_ctx *ctx, const QbaMc &M, const QbaNoiseProfile &P);
// qba_montecarlo_shape, or (curve) qba_montecarlo_curve_shape
template <int NP>
void qba_mc_shape_n(int curve, int *waves, int64_t *lds, int *wgs);
// qba_montecarlo_program_shape (qba_mc_kern.h); the program of NP is compiled
template <int NP>
int qba_mc_program_shape_n(qba_ctx *ctx, int curve, int *sampler, int *waves_compiled, int *waves_run, int64_t *lds,
                           int *wgs);
// QBA_BUILD_EXPERIMENT_FLAGS of the per-n object (qba_build_flags ORs them)
template <int NP>
int qba_lists_build_flags();
