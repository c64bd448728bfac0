// qba_mc_coal_inst.hip -- one n's fused Monte-Carlo kernel under a coalition
// word (qba_k_mc_coal_sampled: qba_mc_kern.h), its
// launcher and its shape query; built once per n = 1..15 with -DQBA_INST_N=n
// (csrc/Makefile), as the _adv kernels are, into code objects of its own.
#define QBA_MC_COAL_INST 1
#include "qba_lists_kern.h"
#include "qba_lists_launch.h"
#include "qba_mc_kern.h"

#ifndef QBA_INST_N
#error "build with -DQBA_INST_N=<n>"
#endif

template int qba_launch_mc_coal<QBA_INST_N>(qba_ctx *ctx, const QbaMc &M);
template void qba_mc_coal_shape_n<QBA_INST_N>(int *waves, int64_t *lds, int *wgs);
