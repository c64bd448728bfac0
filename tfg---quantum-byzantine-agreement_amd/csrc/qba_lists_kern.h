// qba_lists_kern.h -- the data-parallel hot path on gfx950: the device code
// only (its per-n launchers are qba_lists_launch.h; both are instantiated by
// qba_lists_inst.hip):
//   * Born sampling of list entries (tfg.py:68-84 + 128-129) from the compiled
//     factored alias-table program, Philox4x32-10 keyed by the global entry;
//   * the count-mode check pass (tfg.py:87-98, 182, 189, 291-294, 327):
//     per Q-correlated entry, H[u][g][x] += 1 for every group g and
//     C[u][g][h] += 1 for every equal pair, u = L1[k];
//   * the fused sample+check kernel that writes each list byte once and
//     counts from registers.
//
// Layout: lists[g][k] uint8, row stride ld (SoA: a party's list is one row).
// A thread owns 2 x 4 consecutive entries per step (8 B per row), so every row
// store / load of a wave is 512 contiguous bytes.  Histograms are privatised per
// workgroup in LDS and flushed as u32 partials to a slab that a second
// kernel reduces into int64 (bitwise reproducible, no global atomics).
//
// The code is in three headers: qba_lists_sample.h (the samplers),
// qba_lists_count.h (counting) and qba_lists_step.h (the steps and kernels).
#pragma once
#include "qba_lists_sample.h"
#include "qba_lists_count.h"
#include "qba_lists_step.h"
