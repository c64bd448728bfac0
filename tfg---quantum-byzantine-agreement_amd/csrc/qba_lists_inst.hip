// qba_lists_inst.hip -- one n's list kernels and launchers; built once per
// n = 1..15 with -DQBA_INST_N=n (csrc/Makefile), in parallel.
#include "qba_lists_kern.h"
#include "qba_lists_launch.h"
#include "qba_mc_kern.h"

#ifndef QBA_INST_N
#error "build with -DQBA_INST_N=<n>"
#endif

template int qba_launch_lists<QBA_INST_N>(qba_ctx *ctx, const QbaLaunch &L);
template int qba_launch_batched<QBA_INST_N>(qba_ctx *ctx, const QbaBatch &B);
template int qba_launch_mc<QBA_INST_N>(qba_ctx *ctx, const QbaMc &M);
template int qba_mc_program_shape_n<QBA_INST_N>(qba_ctx *ctx, int curve, int *sampler, int *waves_compiled,
                                                int *waves_run, int64_t *lds, int *wgs);
template void qba_mc_shape_n<QBA_INST_N>(int curve, int *waves, int64_t *lds, int *wgs);
template <> int qba_lists_build_flags<QBA_INST_N>() { return QBA_BUILD_EXPERIMENT_FLAGS; }
