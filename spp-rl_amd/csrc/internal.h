// Internal job descriptors shared between kernels and the host API.
#pragma once
#include "common.h"
#include "dw_plan.h"  // DwJob, dw_red_group
#include "mlp.h"

namespace spp {

// dw.hip (own translation unit, ks_dw.hip): the split-K weight-gradient launch + fixed-order reduce
// over nitems work items of jobs[0, njobs); item_job / item_split index the job table; the first
// nlds items are 256 x 256 jobs staged through LDS (k_dw_big; bf16 sets: k_dw_big16, bf16 A and X rows), the
// rest run in k_dw; bf16: the set's jobs are bf16 MFMA jobs (DwJob::bf16); big_waves: 8 runs the fp32 256 x 256
// items as k_dw_big8 (two waves per SIMD), anything else as k_dw_big (bf16 sets: always k_dw_big16).  The last
// nthin items (fp32 sets only: plan_dw's thin jobs) run as k_dw_thin.
void launch_dw_kernels(const DwJob* jobs, const int* item_job, const int* item_split, int nitems, int nlds, int nthin,
                       int njobs, int64_t max_elems, bool bf16, int big_waves, hipStream_t st);
// (dw_red_group, dw_plan.h: the lanes k_dw_reduce gives one output element; max_elems counts lanes)

// fragment-image pack job: logical L[n][k] of a source matrix S (row stride ld)
//   L[n][k] = trans ? S[k][coff + n] : S[n][coff + k]; source rows >= split come from W2
// image order: ob-major ((ob*NBI + ib)*4 + rq)*64 + lane (dense), or
//              ib-major ((ib*NBO + ob)*4 + rq)*64 + lane (dense_lds)
struct PackJob {
  const float* W;
  const float* W2;
  int split, ld, trans, coff;
  MapDesc out, in;
  int NBO, NBI, ibmajor;
  float4* dst;
  int bf16;  // 1: bf16 image for v_mfma_f32_32x32x16_bf16 (2 fragments of 8 bf16 per block pair, mlp.h)
};

struct AdamJob {
  float* p;
  const float* g;
  float* m;
  float* v;
  float* targ;  // polyak target or null
  int64_t n;
};

}  // namespace spp
