// qba_mc_adv_inst.hip -- one n's fused Monte-Carlo kernels under an adversary
// policy (qba_k_mc_sampled_adv, qba_k_mc_curve_sampled_adv: qba_mc_kern.h,
// DESIGN.md section 13.7) and their launcher; built once per n = 1..15 with
// -DQBA_INST_N=n (csrc/Makefile), as the noisy kernels are, into code objects
// of its own.
#define QBA_MC_ADV_INST 1
#include "qba_lists_kern.h"
#include "qba_lists_launch.h"
#include "qba_mc_kern.h"

#ifndef QBA_INST_N
#error "build with -DQBA_INST_N=<n>"
#endif

template int qba_launch_mc_adv<QBA_INST_N>(qba_ctx *ctx, const QbaMc &M);
