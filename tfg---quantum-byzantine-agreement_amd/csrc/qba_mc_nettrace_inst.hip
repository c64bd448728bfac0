// qba_mc_nettrace_inst.hip -- one n's fused Monte-Carlo trace kernel on a
// network that loses packets (qba_k_nettrace_sampled: qba_mc_kern.h, DESIGN.md
// section 13.13) and its launcher; built once per n = 1..15 with
// -DQBA_INST_N=n (csrc/Makefile), as the trace kernel is, into code objects of
// its own.
#define QBA_MC_NETTRACE_INST 1
#include "qba_lists_kern.h"
#include "qba_lists_launch.h"
#include "qba_mc_kern.h"

#ifndef QBA_INST_N
#error "build with -DQBA_INST_N=<n>"
#endif

template int qba_launch_mc_nettrace<QBA_INST_N>(qba_ctx *ctx, const QbaNetTrace &N);
