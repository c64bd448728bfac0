// qba_mc_nprof_inst.hip -- one n's fused Monte-Carlo kernel under a noise
// profile (qba_k_nprof_sampled: qba_mc_kern.h) and its
// launcher; built once per n = 1..15 with -DQBA_INST_N=n (csrc/Makefile), as
// the _adv kernels are, into code objects of its own.
#define QBA_MC_NPROF_INST 1
#include "qba_lists_kern.h"
#include "qba_lists_launch.h"
#include "qba_mc_kern.h"

#ifndef QBA_INST_N
#error "build with -DQBA_INST_N=<n>"
#endif

template int qba_launch_mc_nprof<QBA_INST_N>(qba_ctx *ctx, const QbaMc &M, const QbaNoiseProfile &P);
