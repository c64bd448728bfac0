// qba_lists_noise_inst.hip -- one n's noisy batched kernels
// (qba_k_batched_noisy: qba_lists_step.h) and their launcher; built once per
// n = 1..15 with -DQBA_INST_N=n (csrc/Makefile), as the list kernels are, into
// code objects of its own.
#define QBA_BATCHED_NOISY_INST 1
#include "qba_lists_kern.h"
#include "qba_lists_launch.h"

#ifndef QBA_INST_N
#error "build with -DQBA_INST_N=<n>"
#endif

template int qba_launch_batched_noisy<QBA_INST_N>(qba_ctx *ctx, const QbaBatch &B);
