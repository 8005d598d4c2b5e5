// Host side of the C-ABI that the two handle units with networks, api.hip and api_onp.hip, use: the job-set and
// pack-plan types, and the helpers and kernel launches that api.hip defines and api_onp.hip calls, on top of
// host_base.h (the stream cast, the device-array type, the calls into api_replay.hip / api_comm.hip).  Host only
// (device code does not need it).
#pragma once
#include <algorithm>
#include <vector>

#include "host_base.h"
#include "internal.h"
#include "layout.h"
#include "sac_kernels.h"
#include "sgd.hip"      // (templates and constants only: each unit instantiates its own k_mlp_sgd heads;
#include "sgd_mlp.hip"  //  mlp_sgd_buffers and mlp_sgd_max_wg below are sized by their constants)

namespace spp {

struct NetBufs {
  float *p = nullptr, *g = nullptr, *m = nullptr, *v = nullptr;
  int64_t n = 0;
};

// A weight-gradient job set (dw.hip): up to two phases launched separately.
struct DwSet {
  DevArray<float> slab;
  DevArray<DwJob> jobs;
  DevArray<int> items;
  int B = -1;
  int j0[2] = {0, 0}, nj[2] = {0, 0}, ioff[2] = {0, 0}, nitems[2] = {0, 0};
  int nlds[2] = {0, 0};  // leading items of a phase that run as k_dw_big / k_dw_big16 (256 x 256 jobs)
  int nthin[2] = {0, 0};  // trailing items of a phase that run as k_dw_thin (thin fp32 jobs)
  int thin_min_bp = 0;    // padded batch from which the thin jobs run as k_dw_thin; 0: never (SPP_DW_THIN, .._MIN_BP)
  int64_t max_elems[2] = {1, 1};  // reduce lanes per phase: largest [N*K | N] image x its dw_red_group
  bool bf16 = false;              // bf16 MFMA job set (k_dw<true>)
  int big_waves = 4;              // waves of the fp32 256 x 256 items' kernel: 4 k_dw_big, 8 k_dw_big8 (SPP_DW_BIG_WAVES)
  void release() { slab.release(); jobs.release(); items.release(); }
};

// The packed weight images and LDS table segments of one handle (build_packs, onp_packs): M / T record them in
// call order, commit() places the images in one arena in that order and uploads the job table ordered by list.
struct PackPlan {
  struct Image {
    int list;
    PackJob job;
    const float4** slot;  // receives the image's address
  };
  std::vector<Image> images;
  std::vector<TabSeg> tab;
  int toff = 0;  // floats of the LDS table so far
  int bf16 = 0;  // bf16 images (PackJob::bf16)
  // ib = 1: ib-major image for dense_lds (256-input layers)
  void M(int list, const float* W, const float* W2, int split, int ld, int trans, int coff, MapDesc out, MapDesc in,
         int NBO, int NBI, const float4** slot, int ib = 0) {
    images.push_back({list, PackJob{W, W2, split, ld, trans, coff, out, in, NBO, NBI, ib, nullptr, bf16}, slot});
  }
  // LDS table: each vector (or pair v | v2) starts on a 32-float boundary, zero padded to a whole block
  int T(const float* v, int n, const float* v2 = nullptr, int n2 = 0) {
    const int off = toff, tot = (int)round_up(n + n2, 32);
    tab.push_back(TabSeg{v, n, v2 ? n : tot, off, 0});
    if (v2) tab.push_back(TabSeg{v2, n2, tot - n, off + n, 0});
    toff += tot;
    return off;
  }
  // jobs = the lists back to back (call order inside a list), as uploaded to d_pj; list l = [off[l], off[l + 1])
  sppStatus commit(int nlists, DevArray<float4>& pk, DevArray<PackJob>& d_pj, std::vector<PackJob>& jobs, int* off) {
    size_t nf4 = 0;
    for (auto& m : images) nf4 += (size_t)m.job.NBO * m.job.NBI * 4 * 64;
    pk.release();
    SPP_CHECK_HIP(pk.alloc(nf4));
    size_t of = 0;
    for (auto& m : images) {
      m.job.dst = pk.ptr + of;
      *m.slot = m.job.dst;
      of += (size_t)m.job.NBO * m.job.NBI * 4 * 64;
    }
    jobs.clear();
    for (int l = 0; l < nlists; ++l) {
      off[l] = (int)jobs.size();
      for (auto& m : images)
        if (m.list == l) jobs.push_back(m.job);
    }
    off[nlists] = (int)jobs.size();
    d_pj.release();
    SPP_CHECK_HIP(d_pj.alloc(jobs.size()));
    SPP_CHECK_HIP(hipMemcpy(d_pj.ptr, jobs.data(), sizeof(PackJob) * jobs.size(), hipMemcpyHostToDevice));
    return SPP_OK;
  }
};
enum { PJ_ACTOR, PJ_ACM, PJ_TARG, PJ_CRITIC, PJ_LISTS };  // the agent handles' pack-job lists, in d_pj order

inline MapDesc nat(int n) { return MapDesc{MAP_NAT, n, 0, 0, 0}; }
inline MapDesc cat(int n0, int n1) { return MapDesc{MAP_CAT, n0, blocks_of(n0), n1, n0}; }
inline MapDesc pair(int n) { return MapDesc{MAP_PAIR, n, 0, 0, 0}; }

// ---- defined in api.hip (each documented there)
sppStatus finalize_dw(DwSet& D, std::vector<DwJob>& jobs, int nph, int Bp, int B, int num_cu);
DwJob& dw_job(std::vector<DwJob>& jobs, int Bp, const float* A, int N, const float* X0, int K0, const float* X1,
              int K1, float* dW, float* db, int nrow2 = -1, float* dW2 = nullptr, float* db2 = nullptr);
DwJob& layer_dw(std::vector<DwJob>& jobs, int Bp, float* G, const NetLayout& L, int i, const float* A,
                const float* X0, const float* X1 = nullptr, int K1 = 0);
void launch_dw_set(DwSet& D, int ph, hipStream_t st);
extern int g_sgd_spin;  // sppSetSgdSpinLimit
int* sgd_ctr(DevArray<int>& sync);
sppStatus mlp_sgd_buffers(DevArray<float>& slab, DevArray<int>& sync, hipStream_t st);
// launches of optim.hip's kernels, which api.hip compiles, with the grids of api_onp.hip's call sites: k_pack_matrix
// over njobs jobs on gx workgroups each; k_adam on one job of n elements (no polyak target)
void launch_pack_matrix(int gx, int njobs, const PackJob* jobs, hipStream_t st);
void launch_adam_kernel(const AdamJob* job, int64_t n, float neg_step, float bc2s, hipStream_t st);

// co-resident workgroups of the multi-workgroup AcM k_mlp_sgd on this device (0: no instantiation)
template <int IN, int H2, int OUT, int HEAD, int WV = 4>
int mlp_sgd_max_wg(int num_cu) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_mlp_sgd<IN, H2, OUT, HEAD, true, WV>,
                                                   64 * WV, 0) != hipSuccess)
    per_cu = 0;
  return std::min(MlCfg<IN, H2, OUT, HEAD, WV>::MAXG, per_cu * num_cu);
}

}  // namespace spp
