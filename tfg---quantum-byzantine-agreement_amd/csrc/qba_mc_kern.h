// qba_mc_kern.h -- the fused Monte-Carlo kernel (qba_montecarlo_sampled): a
// wavefront samples the entries of one instance, distils them into the masks
// the protocol rounds consult (mc_entry, qba_proto_rounds.h), runs the rounds
// and writes the instance's result row.  No list, no histogram and no int64
// table leaves the CU.  Included after the list kernels by qba_lists_inst.hip,
// once per n.  DESIGN.md section 13.
//
// The entries are those of qba_k_batched, bit for bit: instance i draws entry
// e of [0, count) with Philox key seed_base + i (qba_entry_d; the closed-form
// sampler takes a pair's two entries from its one block, as qba_sample_quad).
//
// LDS of a workgroup: the sampler's tables, staged once (qba_stage) and shared
// by its waves, then per wave a ProtoShared and the mailbox.  The waves are
// independent after the staging barrier (proto_sync<false>): wave v of
// workgroup b owns instances b * waves + v, + gridDim.x * waves, ..., so a
// ragged last group of instances just leaves some waves with one trip fewer.
#pragma once
#include "qba_lists_launch.h"
#include "qba_noise.h"
#include "qba_proto_adv.h"
#include "qba_proto_rounds.h"

constexpr size_t QBA_MC_CU_LDS = 160 * 1024;  // LDS of a CU, and the most one workgroup may take
constexpr int QBA_MC_CU_WAVES = 16;           // resident waves per CU the shapes are chosen for (<= 128 VGPRs)

struct QbaMcShape {
  int waves;   // per workgroup; 0: the tables leave no room for a wave
  size_t lds;  // dynamic LDS bytes of a workgroup
  int wgs;     // workgroups a CU holds
};

__host__ __device__ constexpr size_t qba_mc_wave_lds(int G, int w) {
  return (size_t)(PROTO_S_WORDS + ((proto_box_words(G, w) + 3) & ~3)) * sizeof(uint32_t);
}

// Waves per workgroup, at most max_waves: the count that keeps the most waves
// resident on a CU (up to QBA_MC_CU_WAVES); among equals the largest, which
// stages the fewest copies of the tables.
// `extra`: bytes a wave holds beside its ProtoShared and mailbox (the curve
// kernel's accumulator area)
__host__ __device__ constexpr QbaMcShape qba_mc_shape(size_t tables, int G, int w, int max_waves, size_t extra = 0) {
  QbaMcShape best{0, 0, 0};
  int best_res = 0;
  for (int nw = 1; nw <= max_waves; ++nw) {
    const size_t lds = tables + (size_t)nw * (qba_mc_wave_lds(G, w) + extra);
    if (lds > QBA_MC_CU_LDS) break;
    int wgs = (int)(QBA_MC_CU_LDS / lds);
    const int by_waves = QBA_MC_CU_WAVES / nw > 1 ? QBA_MC_CU_WAVES / nw : 1;
    if (wgs > by_waves) wgs = by_waves;
    const int res = wgs * nw;
    if (res >= best_res) {
      best_res = res;
      best = QbaMcShape{nw, lds, wgs};
    }
  }
  return best;
}

// Table bytes the per-n wave count is compiled for: the closed-form stage
// tables, else the canonical program's (uniform byte factors, the last of
// LASTB bits, and the Q factor: table_lds of that program).  A program with
// tables of another size may run fewer waves of the same kernel (qba_launch_mc).
template <int NP, int SAMP>
constexpr size_t qba_mc_tables() {
  using C = QCfg<NP>;
  if (SAMP == QBA_S_CLOSED) return (size_t)((CF<NP>::WORDS + 3) & ~3) * sizeof(uint32_t);
  return (size_t)(((C::NFB - 1) * 256 + (1 << C::LASTB) + C::W + 1) & ~1) * sizeof(uint64_t);
}
template <int NP, int SAMP, int NW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, NW * 64)))
    qba_k_mc_sampled(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, int64_t n_inst, uint32_t count,
                     int n_dis, int nw_run, int32_t *__restrict__ out) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *waves = qba_stage<NP, 1, SAMP, NW * 64>(ps, lds, pat, apat, thr, pl);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)__lane_id();
  if (wv >= nw_run) return;  // tables larger than the shape was compiled for: fewer waves have room
  uint32_t *mine = waves + (size_t)wv * (qba_mc_wave_lds(C::G, C::W) / sizeof(uint32_t));
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(mine);
  uint32_t *box = mine + PROTO_S_WORDS;
  const int64_t stride = (int64_t)gridDim.x * nw_run;
  for (int64_t inst = (int64_t)blockIdx.x * nw_run + wv; inst < n_inst; inst += stride) {
    const uint64_t key = seed_base + (uint64_t)inst;
    const uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
    proto_sync<false>();  // the previous instance's row stores have read S
    mc_begin(S, box, C::G, C::W, lane);
    proto_sync<false>();
    uint32_t seen = 0, bad = 0;
    if constexpr (SAMP == QBA_S_CLOSED) {
      // lane l takes pairs l, l + 64, ...: one Philox block, two entries (the
      // second half of the last block of an odd count stays unused)
      const uint32_t npair = (count + 1u) >> 1;
      for (uint32_t p = (uint32_t)lane; p < npair; p += 64u) {
        const QbaU4 x = qba_philox(p, 0u, 0u, 0u, k0, k1);
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
          if (2u * p + h >= count) break;
          uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
          qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, (uint64_t)p, h, k0, k1, pl, d);
#pragma unroll
          for (int i = 0; i < ND; ++i) D[i] = d[i];
          mc_entry<false>(S, box, D, C::G, C::W, seen, bad);
        }
      }
    } else {
      for (uint32_t e = (uint32_t)lane; e < count; e += 64u) {
        uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
        qba_entry_d<NP, SAMP>((uint64_t)e, k0, k1, ps, pat, apat, thr, pl, d);
#pragma unroll
        for (int i = 0; i < ND; ++i) D[i] = d[i];
        mc_entry<false>(S, box, D, C::G, C::W, seen, bad);
      }
    }
    mc_flags(box, C::G, C::W, seen, bad);
    proto_sync<false>();
    uint32_t st;
    const uint32_t pnz = mc_finish<false>(S, box, C::G, C::W, lane, st);
    proto_sync<false>();
    proto_rounds<false>(S, box, NP, n_dis, key, pnz, st, lane, out + inst * (int64_t)(4 + 5 * C::G));
  }
}

// qba_k_mc_sampled_noisy: qba_k_mc_sampled with the flips of DESIGN.md section
// 13.5 (qba_noise.h) put into every entry between the sampler and mc_entry.
// Noise costs registers and Philox blocks and no LDS, so the launch shape is
// the noiseless kernel's.  It is kept as its own text, as mc_entry is: with one
// body behind both kernels the compiler emitted other code for qba_k_mc_sampled
// at every n, and the existing kernels stay byte for byte what they were.
template <int NP, int SAMP, int NW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, NW * 64)))
    qba_k_mc_sampled_noisy(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, int64_t n_inst, uint32_t count,
                           int n_dis, int nw_run, int32_t *__restrict__ out, const QbaNoise nz) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *waves = qba_stage<NP, 1, SAMP, NW * 64>(ps, lds, pat, apat, thr, pl);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)__lane_id();
  if (wv >= nw_run) return;  // tables larger than the shape was compiled for: fewer waves have room
  uint32_t *mine = waves + (size_t)wv * (qba_mc_wave_lds(C::G, C::W) / sizeof(uint32_t));
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(mine);
  uint32_t *box = mine + PROTO_S_WORDS;
  const int64_t stride = (int64_t)gridDim.x * nw_run;
  for (int64_t inst = (int64_t)blockIdx.x * nw_run + wv; inst < n_inst; inst += stride) {
    const uint64_t key = seed_base + (uint64_t)inst;
    const uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
    proto_sync<false>();  // the previous instance's row stores have read S
    mc_begin(S, box, C::G, C::W, lane);
    proto_sync<false>();
    uint32_t seen = 0, bad = 0;
    if constexpr (SAMP == QBA_S_CLOSED) {
      // lane l takes pairs l, l + 64, ...: one Philox block, two entries (the
      // second half of the last block of an odd count stays unused)
      const uint32_t npair = (count + 1u) >> 1;
      for (uint32_t p = (uint32_t)lane; p < npair; p += 64u) {
        const QbaU4 x = qba_philox(p, 0u, 0u, 0u, k0, k1);
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
          if (2u * p + h >= count) break;
          uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
          qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, (uint64_t)p, h, k0, k1, pl, d);
#pragma unroll
          for (int i = 0; i < ND; ++i) D[i] = d[i];
          qba_noise_d<C::G, C::W>(qba_noise_r(2u * p + h, 0u, k0, k1, nz), D);
          mc_entry<false>(S, box, D, C::G, C::W, seen, bad);
        }
      }
    } else {
      for (uint32_t e = (uint32_t)lane; e < count; e += 64u) {
        uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
        qba_entry_d<NP, SAMP>((uint64_t)e, k0, k1, ps, pat, apat, thr, pl, d);
#pragma unroll
        for (int i = 0; i < ND; ++i) D[i] = d[i];
        qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
        mc_entry<false>(S, box, D, C::G, C::W, seen, bad);
      }
    }
    mc_flags(box, C::G, C::W, seen, bad);
    proto_sync<false>();
    uint32_t st;
    const uint32_t pnz = mc_finish<false>(S, box, C::G, C::W, lane, st);
    proto_sync<false>();
    proto_rounds<false>(S, box, NP, n_dis, key, pnz, st, lane, out + inst * (int64_t)(4 + 5 * C::G));
  }
}

// ---------------------------------------------------------------------------
// qba_montecarlo_curve_sampled: the same instances decided at every checkpoint
// c_0 < c_1 < ... of one pass over their entries.
// Entry e depends on e and the key alone, so the entries at count c are the
// first c of any larger count, and the masks are monotone reductions over them:
// the wave keeps running masks in an accumulator area of its own
// (mc_acc_begin, qba_proto_rounds.h) behind its mailbox, adds the entries of
// the segment [c_(j-1), c_j), and at c_j turns a copy into S.tab / S.rep and
// runs the rounds into row j -- which seed their streams from the key alone,
// so row j is the row of qba_k_mc_sampled at count c_j.
// ---------------------------------------------------------------------------
__host__ __device__ constexpr size_t qba_mc_acc_lds(int G, int w) {
  return (size_t)((mc_acc_words(G, w) + 3) & ~3) * sizeof(uint32_t);
}
template <int NP, int SAMP, int NW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, NW * 64)))
    qba_k_mc_curve_sampled(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, int64_t n_inst, int n_dis,
                           int nw_run, int32_t *__restrict__ out, const QbaMcCounts cv) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  constexpr size_t WAVE_WORDS = (qba_mc_wave_lds(C::G, C::W) + qba_mc_acc_lds(C::G, C::W)) / sizeof(uint32_t);
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *waves = qba_stage<NP, 1, SAMP, NW * 64>(ps, lds, pat, apat, thr, pl);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)__lane_id();
  if (wv >= nw_run) return;
  uint32_t *mine = waves + (size_t)wv * WAVE_WORDS;
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(mine);
  uint32_t *box = mine + PROTO_S_WORDS;
  uint32_t *acc = mine + qba_mc_wave_lds(C::G, C::W) / sizeof(uint32_t);
  uint32_t *mcw = acc + C::W * C::G;  // the AND words and the flags, as mc_entry addresses them
  const int64_t stride = (int64_t)gridDim.x * nw_run;
  for (int64_t inst = (int64_t)blockIdx.x * nw_run + wv; inst < n_inst; inst += stride) {
    const uint64_t key = seed_base + (uint64_t)inst;
    const uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
    mc_acc_begin(acc, C::G, C::W, lane);  // nothing but the segments touches the area
    uint32_t seen = 0, bad = 0, lo = 0;
    for (int j = 0; j < cv.n; ++j) {
      const uint32_t hi = cv.c[j];
      proto_sync<false>();  // the area is set up; the previous row's stores have read S
      if constexpr (SAMP == QBA_S_CLOSED) {
        // pairs [lo / 2, ceil(hi / 2)), lane l the l-th, l + 64-th, ... of them;
        // a checkpoint at an odd count splits a pair, whose block is then drawn
        // in both segments and gives each its half
        const uint32_t pend = (hi + 1u) >> 1;
        for (uint32_t p = (lo >> 1) + (uint32_t)lane; p < pend; p += 64u) {
          const QbaU4 x = qba_philox(p, 0u, 0u, 0u, k0, k1);
#pragma unroll
          for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t e = 2u * p + h;
            if (e < lo || e >= hi) continue;
            uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
            qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, (uint64_t)p, h, k0, k1, pl, d);
#pragma unroll
            for (int i = 0; i < ND; ++i) D[i] = d[i];
            mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
          }
        }
      } else {
        for (uint32_t e = lo + (uint32_t)lane; e < hi; e += 64u) {
          uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
          qba_entry_d<NP, SAMP>((uint64_t)e, k0, k1, ps, pat, apat, thr, pl, d);
#pragma unroll
          for (int i = 0; i < ND; ++i) D[i] = d[i];
          mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
        }
      }
      mc_flags(mcw, C::G, C::W, seen, bad);
      proto_sync<false>();
      uint32_t st;
      const uint32_t pnz = mc_acc_finish<false>(S, acc, C::G, C::W, lane, st);
      proto_sync<false>();
      proto_rounds<false>(S, box, NP, n_dis, key, pnz, st, lane,
                          out + ((int64_t)j * n_inst + inst) * (int64_t)(4 + 5 * C::G));
      lo = hi;
    }
    proto_sync<false>();  // the last finish has read the area
  }
}

// qba_k_mc_curve_sampled_noisy: the same for the curve kernel.  The flips of
// entry e depend on the key and e alone, so the prefix property holds.
template <int NP, int SAMP, int NW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, NW * 64)))
    qba_k_mc_curve_sampled_noisy(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, int64_t n_inst, int n_dis,
                                 int nw_run, int32_t *__restrict__ out, const QbaMcCounts cv, const QbaNoise nz) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  constexpr size_t WAVE_WORDS = (qba_mc_wave_lds(C::G, C::W) + qba_mc_acc_lds(C::G, C::W)) / sizeof(uint32_t);
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *waves = qba_stage<NP, 1, SAMP, NW * 64>(ps, lds, pat, apat, thr, pl);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)__lane_id();
  if (wv >= nw_run) return;
  uint32_t *mine = waves + (size_t)wv * WAVE_WORDS;
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(mine);
  uint32_t *box = mine + PROTO_S_WORDS;
  uint32_t *acc = mine + qba_mc_wave_lds(C::G, C::W) / sizeof(uint32_t);
  uint32_t *mcw = acc + C::W * C::G;  // the AND words and the flags, as mc_entry addresses them
  const int64_t stride = (int64_t)gridDim.x * nw_run;
  for (int64_t inst = (int64_t)blockIdx.x * nw_run + wv; inst < n_inst; inst += stride) {
    const uint64_t key = seed_base + (uint64_t)inst;
    const uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
    mc_acc_begin(acc, C::G, C::W, lane);  // nothing but the segments touches the area
    uint32_t seen = 0, bad = 0, lo = 0;
    for (int j = 0; j < cv.n; ++j) {
      const uint32_t hi = cv.c[j];
      proto_sync<false>();  // the area is set up; the previous row's stores have read S
      if constexpr (SAMP == QBA_S_CLOSED) {
        // pairs [lo / 2, ceil(hi / 2)), lane l the l-th, l + 64-th, ... of them;
        // a checkpoint at an odd count splits a pair, whose block is then drawn
        // in both segments and gives each its half
        const uint32_t pend = (hi + 1u) >> 1;
        for (uint32_t p = (lo >> 1) + (uint32_t)lane; p < pend; p += 64u) {
          const QbaU4 x = qba_philox(p, 0u, 0u, 0u, k0, k1);
#pragma unroll
          for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t e = 2u * p + h;
            if (e < lo || e >= hi) continue;
            uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
            qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, (uint64_t)p, h, k0, k1, pl, d);
#pragma unroll
            for (int i = 0; i < ND; ++i) D[i] = d[i];
            qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
            mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
          }
        }
      } else {
        for (uint32_t e = lo + (uint32_t)lane; e < hi; e += 64u) {
          uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
          qba_entry_d<NP, SAMP>((uint64_t)e, k0, k1, ps, pat, apat, thr, pl, d);
#pragma unroll
          for (int i = 0; i < ND; ++i) D[i] = d[i];
          qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
          mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
        }
      }
      mc_flags(mcw, C::G, C::W, seen, bad);
      proto_sync<false>();
      uint32_t st;
      const uint32_t pnz = mc_acc_finish<false>(S, acc, C::G, C::W, lane, st);
      proto_sync<false>();
      proto_rounds<false>(S, box, NP, n_dis, key, pnz, st, lane,
                          out + ((int64_t)j * n_inst + inst) * (int64_t)(4 + 5 * C::G));
      lo = hi;
    }
    proto_sync<false>();  // the last finish has read the area
  }
}


// ---------------------------------------------------------------------------
// qba_k_mc_sampled_adv / qba_k_mc_curve_sampled_adv: the two sampled kernels
// with the rounds under an adversary policy word (proto_rounds_adv,
// qba_proto_adv.h).  They take the noise of 13.5 at run
// time: nz.steps == 0 (flip_q16 == 0) skips the draw under a wave-uniform
// branch, so one instantiation per (n, sampler, form) serves both.  The policy
// is a scalar and takes no LDS: the launch shape is the noiseless kernel's.
// Texts of their own, instantiated by qba_mc_adv_inst.hip alone.
// ---------------------------------------------------------------------------
template <int NP, int SAMP, int NW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, NW * 64)))
    qba_k_mc_sampled_adv(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, int64_t n_inst, uint32_t count,
                           int n_dis, int nw_run, int32_t *__restrict__ out, const QbaNoise nz, uint32_t adv) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *waves = qba_stage<NP, 1, SAMP, NW * 64>(ps, lds, pat, apat, thr, pl);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)__lane_id();
  if (wv >= nw_run) return;  // tables larger than the shape was compiled for: fewer waves have room
  uint32_t *mine = waves + (size_t)wv * (qba_mc_wave_lds(C::G, C::W) / sizeof(uint32_t));
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(mine);
  uint32_t *box = mine + PROTO_S_WORDS;
  const int64_t stride = (int64_t)gridDim.x * nw_run;
  for (int64_t inst = (int64_t)blockIdx.x * nw_run + wv; inst < n_inst; inst += stride) {
    const uint64_t key = seed_base + (uint64_t)inst;
    const uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
    proto_sync<false>();  // the previous instance's row stores have read S
    mc_begin(S, box, C::G, C::W, lane);
    proto_sync<false>();
    uint32_t seen = 0, bad = 0;
    if constexpr (SAMP == QBA_S_CLOSED) {
      // lane l takes pairs l, l + 64, ...: one Philox block, two entries (the
      // second half of the last block of an odd count stays unused)
      const uint32_t npair = (count + 1u) >> 1;
      for (uint32_t p = (uint32_t)lane; p < npair; p += 64u) {
        const QbaU4 x = qba_philox(p, 0u, 0u, 0u, k0, k1);
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
          if (2u * p + h >= count) break;
          uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
          qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, (uint64_t)p, h, k0, k1, pl, d);
#pragma unroll
          for (int i = 0; i < ND; ++i) D[i] = d[i];
          if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(2u * p + h, 0u, k0, k1, nz), D);
          mc_entry<false>(S, box, D, C::G, C::W, seen, bad);
        }
      }
    } else {
      for (uint32_t e = (uint32_t)lane; e < count; e += 64u) {
        uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
        qba_entry_d<NP, SAMP>((uint64_t)e, k0, k1, ps, pat, apat, thr, pl, d);
#pragma unroll
        for (int i = 0; i < ND; ++i) D[i] = d[i];
        if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
        mc_entry<false>(S, box, D, C::G, C::W, seen, bad);
      }
    }
    mc_flags(box, C::G, C::W, seen, bad);
    proto_sync<false>();
    uint32_t st;
    const uint32_t pnz = mc_finish<false>(S, box, C::G, C::W, lane, st);
    proto_sync<false>();
    proto_rounds_adv<false>(S, box, NP, n_dis, key, pnz, st, lane, out + inst * (int64_t)(4 + 5 * C::G), adv);
  }
}

template <int NP, int SAMP, int NW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, NW * 64)))
    qba_k_mc_curve_sampled_adv(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, int64_t n_inst, int n_dis,
                                 int nw_run, int32_t *__restrict__ out, const QbaMcCounts cv, const QbaNoise nz,
                               uint32_t adv) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  constexpr size_t WAVE_WORDS = (qba_mc_wave_lds(C::G, C::W) + qba_mc_acc_lds(C::G, C::W)) / sizeof(uint32_t);
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *waves = qba_stage<NP, 1, SAMP, NW * 64>(ps, lds, pat, apat, thr, pl);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)__lane_id();
  if (wv >= nw_run) return;
  uint32_t *mine = waves + (size_t)wv * WAVE_WORDS;
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(mine);
  uint32_t *box = mine + PROTO_S_WORDS;
  uint32_t *acc = mine + qba_mc_wave_lds(C::G, C::W) / sizeof(uint32_t);
  uint32_t *mcw = acc + C::W * C::G;  // the AND words and the flags, as mc_entry addresses them
  const int64_t stride = (int64_t)gridDim.x * nw_run;
  for (int64_t inst = (int64_t)blockIdx.x * nw_run + wv; inst < n_inst; inst += stride) {
    const uint64_t key = seed_base + (uint64_t)inst;
    const uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
    mc_acc_begin(acc, C::G, C::W, lane);  // nothing but the segments touches the area
    uint32_t seen = 0, bad = 0, lo = 0;
    for (int j = 0; j < cv.n; ++j) {
      const uint32_t hi = cv.c[j];
      proto_sync<false>();  // the area is set up; the previous row's stores have read S
      if constexpr (SAMP == QBA_S_CLOSED) {
        // pairs [lo / 2, ceil(hi / 2)), lane l the l-th, l + 64-th, ... of them;
        // a checkpoint at an odd count splits a pair, whose block is then drawn
        // in both segments and gives each its half
        const uint32_t pend = (hi + 1u) >> 1;
        for (uint32_t p = (lo >> 1) + (uint32_t)lane; p < pend; p += 64u) {
          const QbaU4 x = qba_philox(p, 0u, 0u, 0u, k0, k1);
#pragma unroll
          for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t e = 2u * p + h;
            if (e < lo || e >= hi) continue;
            uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
            qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, (uint64_t)p, h, k0, k1, pl, d);
#pragma unroll
            for (int i = 0; i < ND; ++i) D[i] = d[i];
            if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
            mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
          }
        }
      } else {
        for (uint32_t e = lo + (uint32_t)lane; e < hi; e += 64u) {
          uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
          qba_entry_d<NP, SAMP>((uint64_t)e, k0, k1, ps, pat, apat, thr, pl, d);
#pragma unroll
          for (int i = 0; i < ND; ++i) D[i] = d[i];
          if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
          mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
        }
      }
      mc_flags(mcw, C::G, C::W, seen, bad);
      proto_sync<false>();
      uint32_t st;
      const uint32_t pnz = mc_acc_finish<false>(S, acc, C::G, C::W, lane, st);
      proto_sync<false>();
      proto_rounds_adv<false>(S, box, NP, n_dis, key, pnz, st, lane,
                              out + ((int64_t)j * n_inst + inst) * (int64_t)(4 + 5 * C::G), adv);
      lo = hi;
    }
    proto_sync<false>();  // the last finish has read the area
  }
}


// ---------------------------------------------------------------------------
// qba_k_mc_sweep_sampled: qba_k_mc_curve_sampled_adv deciding each checkpoint
// under every scenario (n_dishonest, adv) of `sv`.
// The running masks become S.tab / S.rep once per checkpoint and every
// scenario's rounds run on them: proto_rounds_adv reads tab and rep through
// proto_check's `const ProtoShared &` and writes only S.dis_mask, S.cv, S.cnt,
// S.dec and the mailbox, each set again from the key before it is read; pnz
// and st are values.  So row (j, s) is the row of qba_k_mc_curve_sampled_adv at
// checkpoint j with scenario s's arguments.  The scenarios are kernel
// arguments (wave-uniform scalars) and take no LDS: the launch shape is the
// curve kernels'.  A text of its own, instantiated by qba_mc_sweep_inst.hip.
// ---------------------------------------------------------------------------
template <int NP, int SAMP, int NW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, NW * 64)))
    qba_k_mc_sweep_sampled(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, int64_t n_inst, int nw_run,
                           int32_t *__restrict__ out, const QbaMcCounts cv, const QbaNoise nz, const QbaMcScen sv) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  constexpr size_t WAVE_WORDS = (qba_mc_wave_lds(C::G, C::W) + qba_mc_acc_lds(C::G, C::W)) / sizeof(uint32_t);
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *waves = qba_stage<NP, 1, SAMP, NW * 64>(ps, lds, pat, apat, thr, pl);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)__lane_id();
  if (wv >= nw_run) return;
  uint32_t *mine = waves + (size_t)wv * WAVE_WORDS;
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(mine);
  uint32_t *box = mine + PROTO_S_WORDS;
  uint32_t *acc = mine + qba_mc_wave_lds(C::G, C::W) / sizeof(uint32_t);
  uint32_t *mcw = acc + C::W * C::G;  // the AND words and the flags, as mc_entry addresses them
  const int64_t stride = (int64_t)gridDim.x * nw_run;
  for (int64_t inst = (int64_t)blockIdx.x * nw_run + wv; inst < n_inst; inst += stride) {
    const uint64_t key = seed_base + (uint64_t)inst;
    const uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
    mc_acc_begin(acc, C::G, C::W, lane);  // nothing but the segments touches the area
    uint32_t seen = 0, bad = 0, lo = 0;
    for (int j = 0; j < cv.n; ++j) {
      const uint32_t hi = cv.c[j];
      proto_sync<false>();  // the area is set up; the previous row's stores have read S
      if constexpr (SAMP == QBA_S_CLOSED) {
        // pairs [lo / 2, ceil(hi / 2)), lane l the l-th, l + 64-th, ... of them;
        // a checkpoint at an odd count splits a pair, whose block is then drawn
        // in both segments and gives each its half
        const uint32_t pend = (hi + 1u) >> 1;
        for (uint32_t p = (lo >> 1) + (uint32_t)lane; p < pend; p += 64u) {
          const QbaU4 x = qba_philox(p, 0u, 0u, 0u, k0, k1);
#pragma unroll
          for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t e = 2u * p + h;
            if (e < lo || e >= hi) continue;
            uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
            qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, (uint64_t)p, h, k0, k1, pl, d);
#pragma unroll
            for (int i = 0; i < ND; ++i) D[i] = d[i];
            if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
            mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
          }
        }
      } else {
        for (uint32_t e = lo + (uint32_t)lane; e < hi; e += 64u) {
          uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
          qba_entry_d<NP, SAMP>((uint64_t)e, k0, k1, ps, pat, apat, thr, pl, d);
#pragma unroll
          for (int i = 0; i < ND; ++i) D[i] = d[i];
          if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
          mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
        }
      }
      mc_flags(mcw, C::G, C::W, seen, bad);
      proto_sync<false>();
      uint32_t st;
      const uint32_t pnz = mc_acc_finish<false>(S, acc, C::G, C::W, lane, st);
      for (int s = 0; s < sv.n; ++s) {
        proto_sync<false>();  // tab and rep are set; the previous scenario's row stores have read S
        proto_rounds_adv<false>(S, box, NP, sv.s[s].n_dishonest, key, pnz, st, lane,
                                out + (((int64_t)j * sv.n + s) * n_inst + inst) * (int64_t)(4 + 5 * C::G),
                                sv.s[s].adv);
      }
      lo = hi;
    }
    proto_sync<false>();  // the last finish has read the area
  }
}


// ---------------------------------------------------------------------------
// qba_k_trace_sampled: qba_k_mc_sampled_adv re-running chosen instances with
// the transcript of their rounds (proto_rounds_trace, qba_proto_trace.h;
// DESIGN.md section 13.9).  Slot j of `idx` is the instance keyed seed_base +
// idx[j]: it samples, flips and distils what that instance of
// qba_k_mc_sampled_adv does and writes row j, counts[j][n + 1] and the first
// `cap` events of every rank to events[j][n + 1][cap][2].  n_match (NULL: no
// limit) points to the number of slots that hold an index, read on the device:
// a tally's capture row and its match count feed the call as they lie.  The
// event stores take no LDS: the launch shape is the noiseless kernel's.  A text
// of its own, seen by qba_mc_trace_inst.hip alone.
// ---------------------------------------------------------------------------
#if defined(QBA_MC_TRACE_INST)
#include "qba_proto_trace.h"
template <int NP, int SAMP, int NW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, NW * 64)))
    qba_k_trace_sampled(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, const int64_t *__restrict__ idx,
                        int64_t n_idx, const int64_t *__restrict__ n_match, uint32_t count, int n_dis, int nw_run,
                        int32_t *__restrict__ rows, int32_t *__restrict__ counts, uint32_t *__restrict__ events,
                        const QbaNoise nz, uint32_t adv, uint32_t cap) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *waves = qba_stage<NP, 1, SAMP, NW * 64>(ps, lds, pat, apat, thr, pl);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)__lane_id();
  if (wv >= nw_run) return;  // tables larger than the shape was compiled for: fewer waves have room
  uint32_t *mine = waves + (size_t)wv * (qba_mc_wave_lds(C::G, C::W) / sizeof(uint32_t));
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(mine);
  uint32_t *box = mine + PROTO_S_WORDS;
  int64_t lim = n_idx;
  if (n_match) {
    const int64_t m = *n_match;
    lim = m < lim ? (m < 0 ? 0 : m) : lim;
  }
  const int64_t stride = (int64_t)gridDim.x * nw_run;
  for (int64_t j = (int64_t)blockIdx.x * nw_run + wv; j < lim; j += stride) {
    const uint64_t key = seed_base + (uint64_t)idx[j];
    const uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
    proto_sync<false>();  // the previous slot's row stores have read S
    mc_begin(S, box, C::G, C::W, lane);
    proto_sync<false>();
    uint32_t seen = 0, bad = 0;
    if constexpr (SAMP == QBA_S_CLOSED) {
      // lane l takes pairs l, l + 64, ...: one Philox block, two entries (the
      // second half of the last block of an odd count stays unused)
      const uint32_t npair = (count + 1u) >> 1;
      for (uint32_t p = (uint32_t)lane; p < npair; p += 64u) {
        const QbaU4 x = qba_philox(p, 0u, 0u, 0u, k0, k1);
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
          if (2u * p + h >= count) break;
          uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
          qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, (uint64_t)p, h, k0, k1, pl, d);
#pragma unroll
          for (int i = 0; i < ND; ++i) D[i] = d[i];
          if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(2u * p + h, 0u, k0, k1, nz), D);
          mc_entry<false>(S, box, D, C::G, C::W, seen, bad);
        }
      }
    } else {
      for (uint32_t e = (uint32_t)lane; e < count; e += 64u) {
        uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
        qba_entry_d<NP, SAMP>((uint64_t)e, k0, k1, ps, pat, apat, thr, pl, d);
#pragma unroll
        for (int i = 0; i < ND; ++i) D[i] = d[i];
        if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
        mc_entry<false>(S, box, D, C::G, C::W, seen, bad);
      }
    }
    mc_flags(box, C::G, C::W, seen, bad);
    proto_sync<false>();
    uint32_t st;
    const uint32_t pnz = mc_finish<false>(S, box, C::G, C::W, lane, st);
    proto_sync<false>();
    // lane r <= n owns events[j][r][0 .. cap); the other lanes store nothing
    uint2 *ev = lane < C::G ? reinterpret_cast<uint2 *>(events) + (j * C::G + lane) * (int64_t)cap : nullptr;
    proto_rounds_trace<false>(S, box, NP, n_dis, key, pnz, st, lane, rows + j * (int64_t)(4 + 5 * C::G), adv, ev, cap,
                              counts + j * C::G);
  }
}
#endif

// ---------------------------------------------------------------------------
// qba_k_mc_coal_sampled: qba_k_mc_curve_sampled_adv with the rounds under a
// coalition word (proto_rounds_coal, qba_proto_coal.h; DESIGN.md section
// 13.10).  A wave's hold lists, [G][w] words, sit behind its accumulator area:
// the launch shape is QbaMcCoalKern's, with that much more LDS per wave.  Only
// the curve form exists; a single count is a curve of one checkpoint.  A text
// of its own, seen by qba_mc_coal_inst.hip alone.
// ---------------------------------------------------------------------------
#if defined(QBA_MC_COAL_INST)
#include "qba_proto_coal.h"
__host__ __device__ constexpr size_t qba_mc_hold_lds(int G, int w) {
  return (size_t)proto_hold_words(G, w) * sizeof(uint32_t);
}
template <int NP, int SAMP, int NW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, NW * 64)))
    qba_k_mc_coal_sampled(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, int64_t n_inst, int n_dis,
                          int nw_run, int32_t *__restrict__ out, const QbaMcCounts cv, const QbaNoise nz, uint32_t adv,
                          uint32_t coal) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  constexpr size_t WAVE_WORDS =
      (qba_mc_wave_lds(C::G, C::W) + qba_mc_acc_lds(C::G, C::W) + qba_mc_hold_lds(C::G, C::W)) / sizeof(uint32_t);
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *waves = qba_stage<NP, 1, SAMP, NW * 64>(ps, lds, pat, apat, thr, pl);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)__lane_id();
  if (wv >= nw_run) return;
  uint32_t *mine = waves + (size_t)wv * WAVE_WORDS;
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(mine);
  uint32_t *box = mine + PROTO_S_WORDS;
  uint32_t *acc = mine + qba_mc_wave_lds(C::G, C::W) / sizeof(uint32_t);
  uint32_t *mcw = acc + C::W * C::G;  // the AND words and the flags, as mc_entry addresses them
  uint32_t *hold = acc + qba_mc_acc_lds(C::G, C::W) / sizeof(uint32_t);
  const int64_t stride = (int64_t)gridDim.x * nw_run;
  for (int64_t inst = (int64_t)blockIdx.x * nw_run + wv; inst < n_inst; inst += stride) {
    const uint64_t key = seed_base + (uint64_t)inst;
    const uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
    mc_acc_begin(acc, C::G, C::W, lane);  // nothing but the segments touches the area
    uint32_t seen = 0, bad = 0, lo = 0;
    for (int j = 0; j < cv.n; ++j) {
      const uint32_t hi = cv.c[j];
      proto_sync<false>();  // the area is set up; the previous row's stores have read S
      if constexpr (SAMP == QBA_S_CLOSED) {
        // pairs [lo / 2, ceil(hi / 2)), lane l the l-th, l + 64-th, ... of them;
        // a checkpoint at an odd count splits a pair, whose block is then drawn
        // in both segments and gives each its half
        const uint32_t pend = (hi + 1u) >> 1;
        for (uint32_t p = (lo >> 1) + (uint32_t)lane; p < pend; p += 64u) {
          const QbaU4 x = qba_philox(p, 0u, 0u, 0u, k0, k1);
#pragma unroll
          for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t e = 2u * p + h;
            if (e < lo || e >= hi) continue;
            uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
            qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, (uint64_t)p, h, k0, k1, pl, d);
#pragma unroll
            for (int i = 0; i < ND; ++i) D[i] = d[i];
            if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
            mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
          }
        }
      } else {
        for (uint32_t e = lo + (uint32_t)lane; e < hi; e += 64u) {
          uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
          qba_entry_d<NP, SAMP>((uint64_t)e, k0, k1, ps, pat, apat, thr, pl, d);
#pragma unroll
          for (int i = 0; i < ND; ++i) D[i] = d[i];
          if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
          mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
        }
      }
      mc_flags(mcw, C::G, C::W, seen, bad);
      proto_sync<false>();
      uint32_t st;
      const uint32_t pnz = mc_acc_finish<false>(S, acc, C::G, C::W, lane, st);
      proto_sync<false>();
      proto_rounds_coal<false>(S, box, hold, NP, n_dis, key, pnz, st, lane,
                               out + ((int64_t)j * n_inst + inst) * (int64_t)(4 + 5 * C::G), adv, coal);
      lo = hi;
    }
    proto_sync<false>();  // the last finish has read the area
  }
}
#endif

// ---------------------------------------------------------------------------
// qba_k_nettrace_sampled: qba_k_trace_sampled with the rounds on a network
// that loses packets (proto_rounds_nettrace, qba_proto_nettrace.h; DESIGN.md
// section 13.13): the same slots, idx / n_match handling, outputs and launch
// shape, and the network word of qba_k_mc_net_sampled, a scalar.  A text of its
// own, seen by qba_mc_nettrace_inst.hip alone.
// ---------------------------------------------------------------------------
#if defined(QBA_MC_NETTRACE_INST)
#include "qba_proto_nettrace.h"
template <int NP, int SAMP, int NW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, NW * 64)))
    qba_k_nettrace_sampled(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, const int64_t *__restrict__ idx,
                           int64_t n_idx, const int64_t *__restrict__ n_match, uint32_t count, int n_dis, int nw_run,
                           int32_t *__restrict__ rows, int32_t *__restrict__ counts, uint32_t *__restrict__ events,
                           const QbaNoise nz, uint32_t adv, uint32_t cap, uint32_t net) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *waves = qba_stage<NP, 1, SAMP, NW * 64>(ps, lds, pat, apat, thr, pl);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)__lane_id();
  if (wv >= nw_run) return;  // tables larger than the shape was compiled for: fewer waves have room
  uint32_t *mine = waves + (size_t)wv * (qba_mc_wave_lds(C::G, C::W) / sizeof(uint32_t));
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(mine);
  uint32_t *box = mine + PROTO_S_WORDS;
  int64_t lim = n_idx;
  if (n_match) {
    const int64_t m = *n_match;
    lim = m < lim ? (m < 0 ? 0 : m) : lim;
  }
  const int64_t stride = (int64_t)gridDim.x * nw_run;
  for (int64_t j = (int64_t)blockIdx.x * nw_run + wv; j < lim; j += stride) {
    const uint64_t key = seed_base + (uint64_t)idx[j];
    const uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
    proto_sync<false>();  // the previous slot's row stores have read S
    mc_begin(S, box, C::G, C::W, lane);
    proto_sync<false>();
    uint32_t seen = 0, bad = 0;
    if constexpr (SAMP == QBA_S_CLOSED) {
      // lane l takes pairs l, l + 64, ...: one Philox block, two entries (the
      // second half of the last block of an odd count stays unused)
      const uint32_t npair = (count + 1u) >> 1;
      for (uint32_t p = (uint32_t)lane; p < npair; p += 64u) {
        const QbaU4 x = qba_philox(p, 0u, 0u, 0u, k0, k1);
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
          if (2u * p + h >= count) break;
          uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
          qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, (uint64_t)p, h, k0, k1, pl, d);
#pragma unroll
          for (int i = 0; i < ND; ++i) D[i] = d[i];
          if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(2u * p + h, 0u, k0, k1, nz), D);
          mc_entry<false>(S, box, D, C::G, C::W, seen, bad);
        }
      }
    } else {
      for (uint32_t e = (uint32_t)lane; e < count; e += 64u) {
        uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
        qba_entry_d<NP, SAMP>((uint64_t)e, k0, k1, ps, pat, apat, thr, pl, d);
#pragma unroll
        for (int i = 0; i < ND; ++i) D[i] = d[i];
        if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
        mc_entry<false>(S, box, D, C::G, C::W, seen, bad);
      }
    }
    mc_flags(box, C::G, C::W, seen, bad);
    proto_sync<false>();
    uint32_t st;
    const uint32_t pnz = mc_finish<false>(S, box, C::G, C::W, lane, st);
    proto_sync<false>();
    // lane r <= n owns events[j][r][0 .. cap); the other lanes store nothing
    uint2 *ev = lane < C::G ? reinterpret_cast<uint2 *>(events) + (j * C::G + lane) * (int64_t)cap : nullptr;
    proto_rounds_nettrace<false>(S, box, NP, n_dis, key, pnz, st, lane, rows + j * (int64_t)(4 + 5 * C::G), adv, net,
                                 ev, cap, counts + j * C::G);
  }
}
#endif

// ---------------------------------------------------------------------------
// qba_k_mc_net_sampled: qba_k_mc_curve_sampled_adv with the rounds on a network
// that loses packets (proto_rounds_net, qba_proto_net.h; DESIGN.md section
// 13.11).  The network word is a scalar and the rounds' seq counters are a
// register pair: no LDS beyond the curve kernels', so the launch shape is
// theirs.  Only the curve form exists; a single count is a curve of one
// checkpoint.  A text of its own, seen by qba_mc_net_inst.hip alone.
// ---------------------------------------------------------------------------
#if defined(QBA_MC_NET_INST)
#include "qba_proto_net.h"
template <int NP, int SAMP, int NW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, NW * 64)))
    qba_k_mc_net_sampled(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, int64_t n_inst, int n_dis,
                         int nw_run, int32_t *__restrict__ out, const QbaMcCounts cv, const QbaNoise nz, uint32_t adv,
                         uint32_t net) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  constexpr size_t WAVE_WORDS = (qba_mc_wave_lds(C::G, C::W) + qba_mc_acc_lds(C::G, C::W)) / sizeof(uint32_t);
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *waves = qba_stage<NP, 1, SAMP, NW * 64>(ps, lds, pat, apat, thr, pl);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)__lane_id();
  if (wv >= nw_run) return;
  uint32_t *mine = waves + (size_t)wv * WAVE_WORDS;
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(mine);
  uint32_t *box = mine + PROTO_S_WORDS;
  uint32_t *acc = mine + qba_mc_wave_lds(C::G, C::W) / sizeof(uint32_t);
  uint32_t *mcw = acc + C::W * C::G;  // the AND words and the flags, as mc_entry addresses them
  const int64_t stride = (int64_t)gridDim.x * nw_run;
  for (int64_t inst = (int64_t)blockIdx.x * nw_run + wv; inst < n_inst; inst += stride) {
    const uint64_t key = seed_base + (uint64_t)inst;
    const uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
    mc_acc_begin(acc, C::G, C::W, lane);  // nothing but the segments touches the area
    uint32_t seen = 0, bad = 0, lo = 0;
    for (int j = 0; j < cv.n; ++j) {
      const uint32_t hi = cv.c[j];
      proto_sync<false>();  // the area is set up; the previous row's stores have read S
      if constexpr (SAMP == QBA_S_CLOSED) {
        // pairs [lo / 2, ceil(hi / 2)), lane l the l-th, l + 64-th, ... of them;
        // a checkpoint at an odd count splits a pair, whose block is then drawn
        // in both segments and gives each its half
        const uint32_t pend = (hi + 1u) >> 1;
        for (uint32_t p = (lo >> 1) + (uint32_t)lane; p < pend; p += 64u) {
          const QbaU4 x = qba_philox(p, 0u, 0u, 0u, k0, k1);
#pragma unroll
          for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t e = 2u * p + h;
            if (e < lo || e >= hi) continue;
            uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
            qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, (uint64_t)p, h, k0, k1, pl, d);
#pragma unroll
            for (int i = 0; i < ND; ++i) D[i] = d[i];
            if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
            mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
          }
        }
      } else {
        for (uint32_t e = lo + (uint32_t)lane; e < hi; e += 64u) {
          uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
          qba_entry_d<NP, SAMP>((uint64_t)e, k0, k1, ps, pat, apat, thr, pl, d);
#pragma unroll
          for (int i = 0; i < ND; ++i) D[i] = d[i];
          if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
          mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
        }
      }
      mc_flags(mcw, C::G, C::W, seen, bad);
      proto_sync<false>();
      uint32_t st;
      const uint32_t pnz = mc_acc_finish<false>(S, acc, C::G, C::W, lane, st);
      proto_sync<false>();
      proto_rounds_net<false>(S, box, NP, n_dis, key, pnz, st, lane,
                              out + ((int64_t)j * n_inst + inst) * (int64_t)(4 + 5 * C::G), adv, net);
      lo = hi;
    }
    proto_sync<false>();  // the last finish has read the area
  }
}
#endif

// ---------------------------------------------------------------------------
// qba_k_grid_sampled: qba_k_mc_sweep_sampled with a network word in every
// scenario and the rounds of qba_k_mc_net_sampled (proto_rounds_net,
// qba_proto_net.h).  The running masks become S.tab /
// S.rep once per checkpoint and every scenario's rounds run on them:
// proto_rounds_net reads tab and rep through proto_check's `const ProtoShared &`
// and writes only S.dis_mask, S.cv (every dest on every run, the lost-commander
// sentinel included), S.cnt, S.dec and the mailbox, each set again from the key
// before it is read; its seq counters are a register it resets per epoch; pnz
// and st are values.  So row (j, s) is the row of qba_k_mc_net_sampled at
// checkpoint j with scenario s's arguments.  Every scenario runs
// proto_rounds_net, a perfect one too: its drop_q16 is wave-uniform, and at 0
// no loss block is drawn.  The scenarios are kernel arguments, read in the loop
// as wave-uniform scalars, and take no LDS: the launch shape is the curve
// kernels'.  A text of its own, seen by qba_mc_grid_inst.hip alone.
// ---------------------------------------------------------------------------
#if defined(QBA_MC_GRID_INST)
#include "qba_proto_net.h"
template <int NP, int SAMP, int NW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, NW * 64)))
    qba_k_grid_sampled(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, int64_t n_inst, int nw_run,
                       int32_t *__restrict__ out, const QbaMcCounts cv, const QbaNoise nz, const QbaMcGrid gv) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  constexpr size_t WAVE_WORDS = (qba_mc_wave_lds(C::G, C::W) + qba_mc_acc_lds(C::G, C::W)) / sizeof(uint32_t);
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *waves = qba_stage<NP, 1, SAMP, NW * 64>(ps, lds, pat, apat, thr, pl);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)__lane_id();
  if (wv >= nw_run) return;
  uint32_t *mine = waves + (size_t)wv * WAVE_WORDS;
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(mine);
  uint32_t *box = mine + PROTO_S_WORDS;
  uint32_t *acc = mine + qba_mc_wave_lds(C::G, C::W) / sizeof(uint32_t);
  uint32_t *mcw = acc + C::W * C::G;  // the AND words and the flags, as mc_entry addresses them
  const int64_t stride = (int64_t)gridDim.x * nw_run;
  for (int64_t inst = (int64_t)blockIdx.x * nw_run + wv; inst < n_inst; inst += stride) {
    const uint64_t key = seed_base + (uint64_t)inst;
    const uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
    mc_acc_begin(acc, C::G, C::W, lane);  // nothing but the segments touches the area
    uint32_t seen = 0, bad = 0, lo = 0;
    for (int j = 0; j < cv.n; ++j) {
      const uint32_t hi = cv.c[j];
      proto_sync<false>();  // the area is set up; the previous row's stores have read S
      if constexpr (SAMP == QBA_S_CLOSED) {
        // pairs [lo / 2, ceil(hi / 2)), lane l the l-th, l + 64-th, ... of them;
        // a checkpoint at an odd count splits a pair, whose block is then drawn
        // in both segments and gives each its half
        const uint32_t pend = (hi + 1u) >> 1;
        for (uint32_t p = (lo >> 1) + (uint32_t)lane; p < pend; p += 64u) {
          const QbaU4 x = qba_philox(p, 0u, 0u, 0u, k0, k1);
#pragma unroll
          for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t e = 2u * p + h;
            if (e < lo || e >= hi) continue;
            uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
            qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, (uint64_t)p, h, k0, k1, pl, d);
#pragma unroll
            for (int i = 0; i < ND; ++i) D[i] = d[i];
            if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
            mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
          }
        }
      } else {
        for (uint32_t e = lo + (uint32_t)lane; e < hi; e += 64u) {
          uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
          qba_entry_d<NP, SAMP>((uint64_t)e, k0, k1, ps, pat, apat, thr, pl, d);
#pragma unroll
          for (int i = 0; i < ND; ++i) D[i] = d[i];
          if (nz.steps) qba_noise_d<C::G, C::W>(qba_noise_r(e, 0u, k0, k1, nz), D);
          mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
        }
      }
      mc_flags(mcw, C::G, C::W, seen, bad);
      proto_sync<false>();
      uint32_t st;
      const uint32_t pnz = mc_acc_finish<false>(S, acc, C::G, C::W, lane, st);
#pragma nounroll
      for (int s = 0; s < gv.n; ++s) {
        proto_sync<false>();  // tab and rep are set; the previous scenario's row stores have read S
        proto_rounds_net<false>(S, box, NP, gv.s[s].n_dishonest, key, pnz, st, lane,
                                out + (((int64_t)j * gv.n + s) * n_inst + inst) * (int64_t)(4 + 5 * C::G),
                                gv.s[s].adv, gv.s[s].net);
      }
      lo = hi;
    }
    proto_sync<false>();  // the last finish has read the area
  }
}
#endif

// ---------------------------------------------------------------------------
// qba_k_nprof_sampled: qba_k_mc_curve_sampled_adv with the masks of a noise
// profile (qba_nprof_r, qba_noise_profile.h) where
// that kernel XORs the flips of section 13.5: a rate per list row and
// depolarised entries instead of the one flip_q16.  The profile is a kernel
// argument (its ladder masks are read as wave-uniform scalars) and takes no
// LDS: the launch shape is the curve kernels'.  The rounds are
// proto_rounds_adv.  Only the curve form exists; a single count is a curve of
// one checkpoint.  A text of its own, seen by qba_mc_nprof_inst.hip alone.
// ---------------------------------------------------------------------------
#if defined(QBA_MC_NPROF_INST)
#include "qba_noise_profile.h"
template <int NP, int SAMP, int NW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, NW * 64)))
    qba_k_nprof_sampled(const QbaProgramSet *__restrict__ ps, uint64_t seed_base, int64_t n_inst, int n_dis,
                        int nw_run, int32_t *__restrict__ out, const QbaMcCounts cv, uint32_t adv,
                        const QbaNoiseProfile np) {
  using C = QCfg<NP>;
  constexpr int ND = CF<NP>::ND;
  constexpr size_t WAVE_WORDS = (qba_mc_wave_lds(C::G, C::W) + qba_mc_acc_lds(C::G, C::W)) / sizeof(uint32_t);
  extern __shared__ __align__(16) uint64_t lds[];
  const uint64_t *pat, *apat, *thr;
  const uint32_t *pl;
  uint32_t *waves = qba_stage<NP, 1, SAMP, NW * 64>(ps, lds, pat, apat, thr, pl);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)__lane_id();
  if (wv >= nw_run) return;
  uint32_t *mine = waves + (size_t)wv * WAVE_WORDS;
  ProtoShared &S = *reinterpret_cast<ProtoShared *>(mine);
  uint32_t *box = mine + PROTO_S_WORDS;
  uint32_t *acc = mine + qba_mc_wave_lds(C::G, C::W) / sizeof(uint32_t);
  uint32_t *mcw = acc + C::W * C::G;  // the AND words and the flags, as mc_entry addresses them
  const bool noisy = (np.steps | np.depol) != 0u;
  const int64_t stride = (int64_t)gridDim.x * nw_run;
  for (int64_t inst = (int64_t)blockIdx.x * nw_run + wv; inst < n_inst; inst += stride) {
    const uint64_t key = seed_base + (uint64_t)inst;
    const uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
    mc_acc_begin(acc, C::G, C::W, lane);  // nothing but the segments touches the area
    uint32_t seen = 0, bad = 0, lo = 0;
    for (int j = 0; j < cv.n; ++j) {
      const uint32_t hi = cv.c[j];
      proto_sync<false>();  // the area is set up; the previous row's stores have read S
      if constexpr (SAMP == QBA_S_CLOSED) {
        // pairs [lo / 2, ceil(hi / 2)), lane l the l-th, l + 64-th, ... of them;
        // a checkpoint at an odd count splits a pair, whose block is then drawn
        // in both segments and gives each its half
        const uint32_t pend = (hi + 1u) >> 1;
        for (uint32_t p = (lo >> 1) + (uint32_t)lane; p < pend; p += 64u) {
          const QbaU4 x = qba_philox(p, 0u, 0u, 0u, k0, k1);
#pragma unroll
          for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t e = 2u * p + h;
            if (e < lo || e >= hi) continue;
            uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
            qba_closed_half<NP>(h ? x.z : x.x, h ? x.w : x.y, (uint64_t)p, h, k0, k1, pl, d);
#pragma unroll
            for (int i = 0; i < ND; ++i) D[i] = d[i];
            if (noisy) qba_noise_d<C::G, C::W>(qba_nprof_r(e, 0u, k0, k1, np), D);
            mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
          }
        }
      } else {
        for (uint32_t e = lo + (uint32_t)lane; e < hi; e += 64u) {
          uint32_t d[ND], D[4] = {0u, 0u, 0u, 0u};
          qba_entry_d<NP, SAMP>((uint64_t)e, k0, k1, ps, pat, apat, thr, pl, d);
#pragma unroll
          for (int i = 0; i < ND; ++i) D[i] = d[i];
          if (noisy) qba_noise_d<C::G, C::W>(qba_nprof_r(e, 0u, k0, k1, np), D);
          mc_entry_at<false>(acc, C::G, mcw, D, C::G, C::W, seen, bad);
        }
      }
      mc_flags(mcw, C::G, C::W, seen, bad);
      proto_sync<false>();
      uint32_t st;
      const uint32_t pnz = mc_acc_finish<false>(S, acc, C::G, C::W, lane, st);
      proto_sync<false>();
      proto_rounds_adv<false>(S, box, NP, n_dis, key, pnz, st, lane,
                              out + ((int64_t)j * n_inst + inst) * (int64_t)(4 + 5 * C::G), adv);
      lo = hi;
    }
    proto_sync<false>();  // the last finish has read the area
  }
}
#endif

// The sampled kernel of (NP, SAMP) for one count (qba_k_mc_sampled) or for a
// curve (qba_k_mc_curve_sampled), or (NOISE) the noisy form of either, as the
// host sees it; everything below is written once over this.  The noisy kernels
// keep the launch shape of the noiseless ones: noise takes no LDS.
template <int NP, int SAMP_, bool CURVE_, bool NOISE_ = false, bool ADV_ = false>
struct QbaMcKern {
  using C = QCfg<NP>;
  static constexpr int SAMP = SAMP_;
  static constexpr bool CURVE = CURVE_;
  static constexpr bool NOISE = NOISE_;
  static constexpr bool ADV = ADV_;  // the _adv kernels: noise at run time, then the policy word
  // LDS of a wave beside its ProtoShared and mailbox
  static constexpr size_t EXTRA = CURVE ? qba_mc_acc_lds(C::G, C::W) : 0;
  // waves per workgroup the kernel is compiled for
  static constexpr int NW = qba_mc_shape(qba_mc_tables<NP, SAMP>(), C::G, C::W, 16, EXTRA).waves;
  static_assert(NW >= 1, "no room for a wave beside the tables");
  static const void *kernel() {
    if constexpr (CURVE && ADV)
      return (const void *)qba_k_mc_curve_sampled_adv<NP, SAMP, NW>;
    else if constexpr (ADV)
      return (const void *)qba_k_mc_sampled_adv<NP, SAMP, NW>;
    else if constexpr (CURVE && NOISE)
      return (const void *)qba_k_mc_curve_sampled_noisy<NP, SAMP, NW>;
    else if constexpr (NOISE)
      return (const void *)qba_k_mc_sampled_noisy<NP, SAMP, NW>;
    else if constexpr (CURVE)
      return (const void *)qba_k_mc_curve_sampled<NP, SAMP, NW>;
    else  // not instantiated for a curve's NW
      return (const void *)qba_k_mc_sampled<NP, SAMP, NW>;
  }
  // The shape a program with `tables` bytes of staged tables runs the kernel
  // in: at most the compiled wave count (the launcher and both shape queries
  // ask here).
  static QbaMcShape run_shape(size_t tables) { return qba_mc_shape(tables, C::G, C::W, NW, EXTRA); }
};

// The launch of one sampler's kernel: full workgroups of its compiled wave
// count, of which nw_run work; persistent over the instances.
template <class K>
static int qba_launch_mc_s(qba_ctx *ctx, const QbaMc &M, size_t tables) {
  const QbaMcShape sh = K::run_shape(tables);
  if (sh.waves < 1)
    return qba_fail(QBA_EUNSUPPORTED, std::string(M.who) + ": the program's tables leave no LDS for a wave");
  if (int rc = lds_allow(K::kernel(), sh.lds)) return rc;
  const int64_t need = (M.n_inst + sh.waves - 1) / sh.waves, cap = (int64_t)ctx->num_cus * sh.wgs;
  const int grid = (int)(need < cap ? need : cap);
  const int nw_run = sh.waves;
  // qba_k_mc_sampled takes the one count where qba_k_mc_curve_sampled takes them all, last;
  // the noisy forms take the noise after that, the _adv forms the noise and then the policy word
  const void *one[] = {&M.ps, &M.seed_base, &M.n_inst, &M.counts.c[0], &M.n_dis, &nw_run, &M.out, &M.noise, &M.adv};
  const void *all[] = {&M.ps, &M.seed_base, &M.n_inst, &M.n_dis, &nw_run, &M.out, &M.counts, &M.noise, &M.adv};
  QBA_HIP(hipLaunchKernel(K::kernel(), dim3(grid), dim3(K::NW * 64), const_cast<void **>(K::CURVE ? all : one), sh.lds,
                          M.stream));
  QBA_HIP(hipGetLastError());
  return QBA_OK;
}

// f(std::integral_constant<int, SAMP>(), tables) for the program compiled for
// NP: its sampler, as qba_launch_batched chooses it, and the bytes of its
// staged tables.
template <int NP, class F>
static int qba_mc_with_program(qba_ctx *ctx, const F &f) {
  const QbaProgramSet *hs = reinterpret_cast<const QbaProgramSet *>(ctx->prog_host[NP]);
  const int samp = sampler_of<NP>(hs);
  if (int rc = check_closed<NP>(hs)) return rc;
  const size_t tables = table_lds<NP>(hs, samp);
  if (samp == QBA_S_CLOSED) {
    if constexpr (NP <= QBA_CLOSED_MAX_N) return f(std::integral_constant<int, QBA_S_CLOSED>(), tables);
    return qba_fail(QBA_EUNSUPPORTED, "closed form beyond n = 11");
  }
  if (samp == QBA_S_FAST) return f(std::integral_constant<int, QBA_S_FAST>(), tables);
  return f(std::integral_constant<int, QBA_S_GENERAL>(), tables);
}

// f(std::bool_constant<curve>()).  The single-count branch stands first, and
// callers choose the sampler inside f: the compiler then instantiates, and lays
// out in the code object, the three single-count kernels before the curve
// kernels, the order tools/codeobj_diff.py finds them in since both exist.
template <class F>
static int qba_mc_with_curve(bool curve, const F &f) {
  if (!curve) return f(std::false_type());
  return f(std::true_type());
}

// f(QbaMcKern of the program compiled for NP, tables)
template <int NP, bool NOISE = false, bool ADV = false, class F>
static int qba_mc_with_kern(qba_ctx *ctx, bool curve, const F &f) {
  return qba_mc_with_curve(curve, [&](auto c) {
    return qba_mc_with_program<NP>(ctx, [&](auto s, size_t tables) {
      return f(QbaMcKern<NP, decltype(s)::value, decltype(c)::value, NOISE, ADV>(), tables);
    });
  });
}

// The noiseless kernels are instantiated by qba_lists_inst.hip, the noisy ones
// by qba_mc_noise_inst.hip: code objects of their own, so that those of the
// list kernels stay what they were; the _adv ones by qba_mc_adv_inst.hip, the
// sweep kernel by qba_mc_sweep_inst.hip, the trace kernel by qba_mc_trace_inst.hip,
// the coalition kernel by qba_mc_coal_inst.hip, the lossy-network kernel by
// qba_mc_net_inst.hip, the grid kernel by qba_mc_grid_inst.hip, the
// lossy-network trace kernel by qba_mc_nettrace_inst.hip, the noise-profile
// kernel by qba_mc_nprof_inst.hip.
#if defined(QBA_MC_TRACE_INST)
// The trace kernel of (NP, SAMP): the single-count _adv kernels' description
// (wave count, run_shape) with its own kernel and argument list.
template <int NP, int SAMP>
struct QbaMcTraceKern : QbaMcKern<NP, SAMP, false, false, true> {
  using Base = QbaMcKern<NP, SAMP, false, false, true>;
  static const void *kernel() { return (const void *)qba_k_trace_sampled<NP, SAMP, Base::NW>; }
};
template <int NP>
int qba_launch_mc_trace(qba_ctx *ctx, const QbaTrace &T) {
  return qba_mc_with_program<NP>(ctx, [&](auto s, size_t tables) -> int {
    using K = QbaMcTraceKern<NP, decltype(s)::value>;
    const QbaMcShape sh = K::run_shape(tables);
    if (sh.waves < 1)
      return qba_fail(QBA_EUNSUPPORTED, std::string(T.who) + ": the program's tables leave no LDS for a wave");
    if (int rc = lds_allow(K::kernel(), sh.lds)) return rc;
    const int64_t need = (T.n_idx + sh.waves - 1) / sh.waves, cap = (int64_t)ctx->num_cus * sh.wgs;
    const int grid = (int)(need < cap ? need : cap);
    const int nw_run = sh.waves;
    const void *args[] = {&T.ps,   &T.seed_base, &T.idx,    &T.n_idx, &T.n_match, &T.count, &T.n_dis,
                          &nw_run, &T.rows,      &T.counts, &T.events, &T.noise,  &T.adv,   &T.cap};
    QBA_HIP(hipLaunchKernel(K::kernel(), dim3(grid), dim3(K::NW * 64), const_cast<void **>(args), sh.lds, T.stream));
    QBA_HIP(hipGetLastError());
    return QBA_OK;
  });
}
#elif defined(QBA_MC_SWEEP_INST)
// The sweep kernel of (NP, SAMP): the curve kernels' description (wave count,
// EXTRA, run_shape) with its own kernel and argument list.
template <int NP, int SAMP>
struct QbaMcSweepKern : QbaMcKern<NP, SAMP, true, false, true> {
  using Base = QbaMcKern<NP, SAMP, true, false, true>;
  static const void *kernel() { return (const void *)qba_k_mc_sweep_sampled<NP, SAMP, Base::NW>; }
};
template <int NP>
int qba_launch_mc_sweep(qba_ctx *ctx, const QbaMc &M) {
  return qba_mc_with_program<NP>(ctx, [&](auto s, size_t tables) -> int {
    using K = QbaMcSweepKern<NP, decltype(s)::value>;
    const QbaMcShape sh = K::run_shape(tables);
    if (sh.waves < 1)
      return qba_fail(QBA_EUNSUPPORTED, std::string(M.who) + ": the program's tables leave no LDS for a wave");
    if (int rc = lds_allow(K::kernel(), sh.lds)) return rc;
    const int64_t need = (M.n_inst + sh.waves - 1) / sh.waves, cap = (int64_t)ctx->num_cus * sh.wgs;
    const int grid = (int)(need < cap ? need : cap);
    const int nw_run = sh.waves;
    const void *args[] = {&M.ps, &M.seed_base, &M.n_inst, &nw_run, &M.out, &M.counts, &M.noise, &M.scen};
    QBA_HIP(hipLaunchKernel(K::kernel(), dim3(grid), dim3(K::NW * 64), const_cast<void **>(args), sh.lds, M.stream));
    QBA_HIP(hipGetLastError());
    return QBA_OK;
  });
}
#elif defined(QBA_MC_COAL_INST)
// The coalition kernel of (NP, SAMP): the curve _adv kernels' description with
// the hold lists added to a wave's LDS (so a wave count of its own), its own
// kernel and argument list.
template <int NP, int SAMP>
struct QbaMcCoalKern : QbaMcKern<NP, SAMP, true, false, true> {
  using C = QCfg<NP>;
  static constexpr size_t EXTRA = qba_mc_acc_lds(C::G, C::W) + qba_mc_hold_lds(C::G, C::W);
  static constexpr int NW = qba_mc_shape(qba_mc_tables<NP, SAMP>(), C::G, C::W, 16, EXTRA).waves;
  static_assert(NW >= 1, "no room for a wave beside the tables");
  static const void *kernel() { return (const void *)qba_k_mc_coal_sampled<NP, SAMP, NW>; }
  static QbaMcShape run_shape(size_t tables) { return qba_mc_shape(tables, C::G, C::W, NW, EXTRA); }
};
template <int NP>
int qba_launch_mc_coal(qba_ctx *ctx, const QbaMc &M) {
  return qba_mc_with_program<NP>(ctx, [&](auto s, size_t tables) -> int {
    using K = QbaMcCoalKern<NP, decltype(s)::value>;
    const QbaMcShape sh = K::run_shape(tables);
    if (sh.waves < 1)
      return qba_fail(QBA_EUNSUPPORTED, std::string(M.who) + ": the program's tables leave no LDS for a wave");
    if (int rc = lds_allow(K::kernel(), sh.lds)) return rc;
    const int64_t need = (M.n_inst + sh.waves - 1) / sh.waves, cap = (int64_t)ctx->num_cus * sh.wgs;
    const int grid = (int)(need < cap ? need : cap);
    const int nw_run = sh.waves;
    const void *args[] = {&M.ps, &M.seed_base, &M.n_inst, &M.n_dis, &nw_run, &M.out, &M.counts, &M.noise, &M.adv,
                          &M.coal};
    QBA_HIP(hipLaunchKernel(K::kernel(), dim3(grid), dim3(K::NW * 64), const_cast<void **>(args), sh.lds, M.stream));
    QBA_HIP(hipGetLastError());
    return QBA_OK;
  });
}
// qba_montecarlo_coal_shape: the shape of the shipped programs' kernel
template <int NP>
void qba_mc_coal_shape_n(int *waves, int64_t *lds, int *wgs) {
  constexpr int SAMP = NP <= QBA_CLOSED_MAX_N ? QBA_S_CLOSED : QBA_S_FAST;
  const QbaMcShape sh = QbaMcCoalKern<NP, SAMP>::run_shape(qba_mc_tables<NP, SAMP>());
  *waves = sh.waves;
  *lds = (int64_t)sh.lds;
  *wgs = sh.wgs;
}
#elif defined(QBA_MC_NET_INST)
// The lossy-network kernel of (NP, SAMP): the curve _adv kernels' description
// (wave count, EXTRA, run_shape) with its own kernel and argument list.
template <int NP, int SAMP>
struct QbaMcNetKern : QbaMcKern<NP, SAMP, true, false, true> {
  using Base = QbaMcKern<NP, SAMP, true, false, true>;
  static const void *kernel() { return (const void *)qba_k_mc_net_sampled<NP, SAMP, Base::NW>; }
};
template <int NP>
int qba_launch_mc_net(qba_ctx *ctx, const QbaMc &M) {
  return qba_mc_with_program<NP>(ctx, [&](auto s, size_t tables) -> int {
    using K = QbaMcNetKern<NP, decltype(s)::value>;
    const QbaMcShape sh = K::run_shape(tables);
    if (sh.waves < 1)
      return qba_fail(QBA_EUNSUPPORTED, std::string(M.who) + ": the program's tables leave no LDS for a wave");
    if (int rc = lds_allow(K::kernel(), sh.lds)) return rc;
    const int64_t need = (M.n_inst + sh.waves - 1) / sh.waves, cap = (int64_t)ctx->num_cus * sh.wgs;
    const int grid = (int)(need < cap ? need : cap);
    const int nw_run = sh.waves;
    const void *args[] = {&M.ps, &M.seed_base, &M.n_inst, &M.n_dis, &nw_run, &M.out, &M.counts, &M.noise, &M.adv,
                          &M.net};
    QBA_HIP(hipLaunchKernel(K::kernel(), dim3(grid), dim3(K::NW * 64), const_cast<void **>(args), sh.lds, M.stream));
    QBA_HIP(hipGetLastError());
    return QBA_OK;
  });
}
#elif defined(QBA_MC_GRID_INST)
// The grid kernel of (NP, SAMP): the curve _adv kernels' description (wave
// count, EXTRA, run_shape) with its own kernel and argument list.
template <int NP, int SAMP>
struct QbaMcGridKern : QbaMcKern<NP, SAMP, true, false, true> {
  using Base = QbaMcKern<NP, SAMP, true, false, true>;
  static const void *kernel() { return (const void *)qba_k_grid_sampled<NP, SAMP, Base::NW>; }
};
template <int NP>
int qba_launch_mc_grid(qba_ctx *ctx, const QbaMc &M) {
  return qba_mc_with_program<NP>(ctx, [&](auto s, size_t tables) -> int {
    using K = QbaMcGridKern<NP, decltype(s)::value>;
    const QbaMcShape sh = K::run_shape(tables);
    if (sh.waves < 1)
      return qba_fail(QBA_EUNSUPPORTED, std::string(M.who) + ": the program's tables leave no LDS for a wave");
    if (int rc = lds_allow(K::kernel(), sh.lds)) return rc;
    const int64_t need = (M.n_inst + sh.waves - 1) / sh.waves, cap = (int64_t)ctx->num_cus * sh.wgs;
    const int grid = (int)(need < cap ? need : cap);
    const int nw_run = sh.waves;
    const void *args[] = {&M.ps, &M.seed_base, &M.n_inst, &nw_run, &M.out, &M.counts, &M.noise, &M.grid};
    QBA_HIP(hipLaunchKernel(K::kernel(), dim3(grid), dim3(K::NW * 64), const_cast<void **>(args), sh.lds, M.stream));
    QBA_HIP(hipGetLastError());
    return QBA_OK;
  });
}
#elif defined(QBA_MC_NETTRACE_INST)
// The lossy-network trace kernel of (NP, SAMP): the single-count _adv kernels'
// description (wave count, run_shape), as the trace kernel's, with its own
// kernel and argument list.
template <int NP, int SAMP>
struct QbaMcNetTraceKern : QbaMcKern<NP, SAMP, false, false, true> {
  using Base = QbaMcKern<NP, SAMP, false, false, true>;
  static const void *kernel() { return (const void *)qba_k_nettrace_sampled<NP, SAMP, Base::NW>; }
};
template <int NP>
int qba_launch_mc_nettrace(qba_ctx *ctx, const QbaNetTrace &N) {
  const QbaTrace &T = N.t;
  return qba_mc_with_program<NP>(ctx, [&](auto s, size_t tables) -> int {
    using K = QbaMcNetTraceKern<NP, decltype(s)::value>;
    const QbaMcShape sh = K::run_shape(tables);
    if (sh.waves < 1)
      return qba_fail(QBA_EUNSUPPORTED, std::string(T.who) + ": the program's tables leave no LDS for a wave");
    if (int rc = lds_allow(K::kernel(), sh.lds)) return rc;
    const int64_t need = (T.n_idx + sh.waves - 1) / sh.waves, cap = (int64_t)ctx->num_cus * sh.wgs;
    const int grid = (int)(need < cap ? need : cap);
    const int nw_run = sh.waves;
    const void *args[] = {&T.ps,   &T.seed_base, &T.idx,    &T.n_idx,  &T.n_match, &T.count, &T.n_dis, &nw_run,
                          &T.rows, &T.counts,    &T.events, &T.noise,  &T.adv,     &T.cap,   &N.net};
    QBA_HIP(hipLaunchKernel(K::kernel(), dim3(grid), dim3(K::NW * 64), const_cast<void **>(args), sh.lds, T.stream));
    QBA_HIP(hipGetLastError());
    return QBA_OK;
  });
}
#elif defined(QBA_MC_NPROF_INST)
// The noise-profile kernel of (NP, SAMP): the curve _adv kernels' description
// (wave count, EXTRA, run_shape) with its own kernel and argument list.
template <int NP, int SAMP>
struct QbaMcNprofKern : QbaMcKern<NP, SAMP, true, false, true> {
  using Base = QbaMcKern<NP, SAMP, true, false, true>;
  static const void *kernel() { return (const void *)qba_k_nprof_sampled<NP, SAMP, Base::NW>; }
};
template <int NP>
int qba_launch_mc_nprof(qba_ctx *ctx, const QbaMc &M, const QbaNoiseProfile &P) {
  return qba_mc_with_program<NP>(ctx, [&](auto s, size_t tables) -> int {
    using K = QbaMcNprofKern<NP, decltype(s)::value>;
    const QbaMcShape sh = K::run_shape(tables);
    if (sh.waves < 1)
      return qba_fail(QBA_EUNSUPPORTED, std::string(M.who) + ": the program's tables leave no LDS for a wave");
    if (int rc = lds_allow(K::kernel(), sh.lds)) return rc;
    const int64_t need = (M.n_inst + sh.waves - 1) / sh.waves, cap = (int64_t)ctx->num_cus * sh.wgs;
    const int grid = (int)(need < cap ? need : cap);
    const int nw_run = sh.waves;
    const void *args[] = {&M.ps, &M.seed_base, &M.n_inst, &M.n_dis, &nw_run, &M.out, &M.counts, &M.adv, &P};
    QBA_HIP(hipLaunchKernel(K::kernel(), dim3(grid), dim3(K::NW * 64), const_cast<void **>(args), sh.lds, M.stream));
    QBA_HIP(hipGetLastError());
    return QBA_OK;
  });
}
#elif defined(QBA_MC_ADV_INST)
template <int NP>
int qba_launch_mc_adv(qba_ctx *ctx, const QbaMc &M) {
  return qba_mc_with_kern<NP, false, true>(ctx, M.curve, [&](auto k, size_t tables) {
    return qba_launch_mc_s<decltype(k)>(ctx, M, tables);
  });
}
#elif !defined(QBA_MC_NOISY_INST)
template <int NP>
int qba_launch_mc(qba_ctx *ctx, const QbaMc &M) {
  return qba_mc_with_kern<NP>(ctx, M.curve, [&](auto k, size_t tables) {
    return qba_launch_mc_s<decltype(k)>(ctx, M, tables);
  });
}
#else
template <int NP>
int qba_launch_mc_noisy(qba_ctx *ctx, const QbaMc &M) {
  return qba_mc_with_kern<NP, true>(ctx, M.curve, [&](auto k, size_t tables) {
    return qba_launch_mc_s<decltype(k)>(ctx, M, tables);
  });
}
#endif

static int qba_mc_put_shape(const QbaMcShape &sh, int *waves, int64_t *lds, int *wgs) {
  *waves = sh.waves;
  *lds = (int64_t)sh.lds;
  *wgs = sh.wgs;
  return QBA_OK;
}

// qba_montecarlo_shape / _curve_shape: the shape of the shipped programs'
// kernel (closed form up to n = 11, else the canonical tables of qba_mc_tables)
template <int NP>
void qba_mc_shape_n(int curve, int *waves, int64_t *lds, int *wgs) {
  constexpr int SAMP = NP <= QBA_CLOSED_MAX_N ? QBA_S_CLOSED : QBA_S_FAST;
  qba_mc_with_curve(curve, [&](auto c) {
    using K = QbaMcKern<NP, SAMP, decltype(c)::value>;
    return qba_mc_put_shape(K::run_shape(qba_mc_tables<NP, SAMP>()), waves, lds, wgs);
  });
}

// qba_montecarlo_program_shape: what qba_launch_mc would run the program
// compiled for NP in, from the same sampler choice, table bytes and kernel
// description; launches nothing.
template <int NP>
int qba_mc_program_shape_n(qba_ctx *ctx, int curve, int *sampler, int *waves_compiled, int *waves_run, int64_t *lds,
                           int *wgs) {
  return qba_mc_with_kern<NP>(ctx, curve, [&](auto k, size_t tables) {
    using K = decltype(k);
    *sampler = K::SAMP;
    *waves_compiled = K::NW;
    return qba_mc_put_shape(K::run_shape(tables), waves_run, lds, wgs);
  });
}
