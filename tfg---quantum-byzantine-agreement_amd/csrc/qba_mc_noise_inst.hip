// qba_mc_noise_inst.hip -- one n's noisy fused Monte-Carlo kernels
// (qba_k_mc_sampled_noisy, qba_k_mc_curve_sampled_noisy: qba_mc_kern.h) and
// their launcher; built once per n = 1..15 with -DQBA_INST_N=n (csrc/Makefile),
// as the list kernels are, into code objects of its own.
#define QBA_MC_NOISY_INST 1
#include "qba_lists_kern.h"
#include "qba_lists_launch.h"
#include "qba_mc_kern.h"

#ifndef QBA_INST_N
#error "build with -DQBA_INST_N=<n>"
#endif

template int qba_launch_mc_noisy<QBA_INST_N>(qba_ctx *ctx, const QbaMc &M);
