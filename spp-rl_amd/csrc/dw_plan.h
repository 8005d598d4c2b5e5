// The weight-gradient job descriptor (dw.hip) and the host arithmetic that plans a job set: sample splits, the
// slab arena and the item table.  Plain C++17, nothing from HIP: the host API (finalize_dw), the kernels (the
// descriptor and dw_red_group) and a plain g++ program (tests/dw_plan_dump.cpp) read the same header.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "intmath.h"

#if defined(__HIPCC__)
#define SPP_HD __host__ __device__
#else
#define SPP_HD
#endif

// bf16 sets' 256 x 256 bf16-operand weight gradients on the LDS-staged k_dw_big16 (0: k_dw<true>, the A/B)
#ifndef SPP_DW_BIG16
#define SPP_DW_BIG16 1
#endif

namespace spp {

// weight-gradient GEMM job (dw.hip)
struct DwJob {
  const float* A;   // delta [N][Bp]
  const float* X0;  // input segment 0 [K0][Bp]
  const float* X1;  // input segment 1 [K1][Bp] (may be null)
  float* dW;        // rows [0, nrow2) of [N][K0+K1], canonical
  float* db;        // [nrow2] or null
  float* dW2;       // rows [nrow2, N) (second output, e.g. the log-std head), or null
  float* db2;
  float* slab;      // split partials [nsplit * wsplit][slab_stride]
  int64_t slab_stride;
  int N, K0, K1, Bp;
  int split_len, nsplit, nrow2;
  int wsplit;       // 4: output <= 128x128, the 4 waves of an item split its samples (one slab each); else 1
  int bf16;         // 1: bf16 MFMA (operands rounded to bf16 in registers, fp32 accumulation)
  int a_bf, x_bf;   // (bf16 only) A / X rows hold bf16 elements ([rows][Bp] __bf16), else fp32
  int fused;        // 1: no work items -- a phase kernel writes the nsplit slabs (per wave); only reduced
};

// k_dw_reduce: lanes that sum one output element of a job with nslab partial slabs of `elems` elements
// (fixed-order reduce).  One lane per element (consecutive lanes read consecutive elements of a slab:
// coalesced) for the split-K GEMM jobs; a group of 16 lanes per element for the few-element, many-slab jobs
// (the fused fc3 jobs' 257 x one-partial-per-wave), whose one-lane serial sums were the launch's critical
// path; max_elems counts lanes
inline SPP_HD int dw_red_group(int nslab, int64_t elems) { return nslab >= 64 && elems <= 4096 ? 16 : 1; }

// What plan_dw lays out for a job set of up to two phases (jobs [j0[ph], j0[ph] + nj[ph])).
struct DwPlan {
  size_t need = 0;                // floats of the slab arena (phases run back to back: they share it)
  std::vector<int64_t> slab_off;  // per job: where its slabs start in the arena; -1: one slab, stored directly
  std::vector<int> items;         // per phase at ioff[ph]: [item_job (nitems) | item_split (nitems)]
  int ioff[2] = {0, 0}, nitems[2] = {0, 0}, nlds[2] = {0, 0};
  int nthin[2] = {0, 0};          // trailing items of a phase that run as k_dw_thin
  int64_t max_elems[2] = {1, 1};
};

// Split assignment (written into the jobs: wsplit, split_len, nsplit), slab arena and item table of a job set.
// thin_min_bp > 0: the thin fp32 jobs of a set of at least that many padded samples run as k_dw_thin (their items
// are listed last, counted by nthin); 0: every item that is not an LDS one runs in k_dw, in the order of old.
inline DwPlan plan_dw(std::vector<DwJob>& jobs, const int* j0, const int* nj, int nph, int Bp, int num_cu,
                      int thin_min_bp = 0) {
  DwPlan P;
  // Sample splits: the large (>= 128x128 padded) GEMMs of a phase share ~one
  // workgroup per CU in proportion to their MACs; the small, HBM-bound ones
  // take 2048-sample items.
  auto is_big = [](const DwJob& j) {
    return (int64_t)round_up(j.N, 32) * round_up(j.K0 + j.K1, 32) >= 128 * 128;
  };
  // 256 x 256 fp32 jobs run as their own launch (k_dw_big); the other large jobs share k_dw's launch
  // (small batches -- vanilla SAC's B = 100, PPO minibatches -- keep one launch: k_dw's register tiles)
  // (bf16 sets: the 256 x 256 jobs whose A and X rows are both bf16 run as k_dw_big16, in 64-sample steps)
  auto lds_big = [Bp](const DwJob& j) {
    return Bp >= 8192 && j.N == 256 && j.K0 == 256 && j.K1 == 0 &&
           (!j.bf16 || (SPP_DW_BIG16 && j.a_bf && j.x_bf && Bp % 64 == 0));
  };
  // thin jobs (k_dw_thin): fp32, two sample parts per item, one side a single 32-block (the other at most 256)
  auto thin_ok = [Bp, thin_min_bp](const DwJob& j) {
    const int n32 = (int)round_up(j.N, 32), k32 = (int)round_up(j.K0 + j.K1, 32);
    return thin_min_bp > 0 && Bp >= thin_min_bp && !j.bf16 && !j.fused && j.wsplit == 2 &&
           ((n32 == 32 && k32 <= 256) || (k32 == 32 && n32 <= 256));
  };
  auto assign_splits = [&](int first, int count) {
    double big[2] = {0.0, 0.0};  // MACs of the large jobs per launch
    for (int i = first; i < first + count; ++i)
      if (!jobs[i].fused && is_big(jobs[i]))
        big[lds_big(jobs[i]) ? 0 : 1] += (double)round_up(jobs[i].N, 32) * round_up(jobs[i].K0 + jobs[i].K1, 32);
    for (int i = first; i < first + count; ++i) {
      DwJob& j = jobs[i];
      if (j.fused) continue;  // nsplit = the phase kernel's waves, set by the caller
      const double pm = (double)round_up(j.N, 32) * round_up(j.K0 + j.K1, 32);
      // outputs that fit one 128x128 wave quadrant: the 4 waves split each item's samples
      const bool thin_n = j.N <= 128, thin_k = j.K0 + j.K1 <= 128;
      j.wsplit = thin_n && thin_k ? 4 : (thin_n != thin_k ? 2 : 1);
      // large jobs: ~one workgroup per CU over their launch, in proportion to their MACs; small jobs:
      // >= 2048 samples per item, and at most ~256 slabs (the fixed-order reduce is serial over slabs)
      int ns = is_big(j) ? (int)std::lround(num_cu * pm / big[lds_big(j) ? 0 : 1])
                         : std::min(cdiv(Bp, 2048), std::max(1, 256 / j.wsplit));
      // small batches (PPO minibatches of 512): at least 4 items, so each wave of an item takes one
      // 32-sample unit instead of a serial chain over the whole batch
      if (!is_big(j)) ns = std::max(ns, std::min(cdiv(Bp, 32 * j.wsplit), 4));
      ns = std::max(1, std::min(ns, std::max(1, Bp / 32)));
      j.split_len = (int)round_up(cdiv(Bp, ns), lds_big(j) && j.bf16 ? 64 : 32 * j.wsplit);
      j.nsplit = cdiv(Bp, j.split_len);
    }
  };
  for (int ph = 0; ph < nph; ++ph) assign_splits(j0[ph], nj[ph]);
  // slabs: phases run back to back on one stream -> they share one arena
  P.slab_off.assign(jobs.size(), -1);
  for (int ph = 0; ph < nph; ++ph) {
    size_t off = 0;
    for (int j = j0[ph]; j < j0[ph] + nj[ph]; ++j) {
      if (jobs[j].nsplit * jobs[j].wsplit > 1) {
        P.slab_off[j] = (int64_t)off;
        off += (size_t)jobs[j].nsplit * jobs[j].wsplit * jobs[j].slab_stride;
      }
    }
    P.need = std::max(P.need, off);
  }
  for (int ph = 0; ph < nph; ++ph) {
    std::vector<int> jj, ss;
    // large-GEMM items first (they set the phase's critical path): the 256 x 256 fp32 jobs (k_dw_big,
    // LDS-DMA operands), then the other large ones, then the small ones (k_dw), then those of the small ones
    // that k_dw_thin takes (one contiguous run at the end: k_dw's items stay contiguous too)
    P.nlds[ph] = P.nthin[ph] = 0;
    for (int pass = 0; pass < 4; ++pass)
      for (int j = j0[ph]; j < j0[ph] + nj[ph]; ++j) {
        const int cls = lds_big(jobs[j]) ? 0 : (is_big(jobs[j]) ? 1 : (thin_ok(jobs[j]) ? 3 : 2));
        if (cls != pass || jobs[j].fused) continue;
        for (int sp = 0; sp < jobs[j].nsplit; ++sp) {
          jj.push_back(j - j0[ph]);
          ss.push_back(sp);
          if (pass == 0) ++P.nlds[ph];
          if (pass == 3) ++P.nthin[ph];
        }
      }
    P.max_elems[ph] = 1;
    for (int j = j0[ph]; j < j0[ph] + nj[ph]; ++j) {
      const int64_t el = (int64_t)jobs[j].N * (jobs[j].K0 + jobs[j].K1) + jobs[j].N;
      P.max_elems[ph] = std::max<int64_t>(P.max_elems[ph], el * dw_red_group(jobs[j].nsplit * jobs[j].wsplit, el));
    }
    P.ioff[ph] = (int)P.items.size();
    P.nitems[ph] = (int)jj.size();
    P.items.insert(P.items.end(), jj.begin(), jj.end());
    P.items.insert(P.items.end(), ss.begin(), ss.end());
  }
  return P;
}

}  // namespace spp
