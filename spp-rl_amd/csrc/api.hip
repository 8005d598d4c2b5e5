// libspprl C-ABI implementation: the error state and the off-policy agent handle (SAC / DDPG phases, AcM regression
// and SGD, policy act, debug entries); kernels included below.  The other units: api_replay.hip (replay ring,
// obs statistics, stream utilities), api_comm.hip (RCCL exchange), api_onp.hip (on-policy handle).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/spprl.h"
#include "internal.h"
#include "layout.h"
#include "replay.h"  // ReplayDev (sppAgentStageFromReplay), obs_norm1 (k_stage_post)
#include "sac_kernels.h"
#include "host.h"

#include "optim.hip"
#include "sac.hip"
#include "ddpg.hip"
#include "kset.h"
#ifdef SPP_SINGLE_TU  // profiling / development builds: everything in one TU
#include "ks_dw.hip"
#include "ks_sac_hopper.hip"
#if defined(SPP_WITH_HCHEETAH)  // region-profiling builds of the HalfCheetah AcM SGD: + the HalfCheetah set
#include "ks_sac_hcheetah.hip"
#endif
#if defined(SPP_ONLY_BF16)  // region-profiling builds of the bf16 sets: Hopper fp32 + bf16 only
#define SPP_ONLY_HOPPER
#include "ks_sac_bf16.hip"
#endif
#ifndef SPP_ONLY_HOPPER
#include "ks_sac_hcheetah.hip"
#include "ks_sac_ant.hip"
#include "ks_sac_small.hip"
#include "ks_ddpg.hip"
#include "ks_ddpg_ant.hip"
#include "ks_sac_bf16.hip"
#include "ks_sac_vanilla.hip"
#include "ks_ddpg_vanilla.hip"
#endif
#endif

namespace spp {

static thread_local std::string g_err;
void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}
const char* get_error() { return g_err.c_str(); }

}  // namespace spp

using namespace spp;

extern "C" {

const char* sppGetLastError(void) { return get_error(); }
int sppGetVersion(void) { return 1; }

}  // extern "C"

// ================================================================== agent
namespace spp {

// dims -> kernel instantiation: one translation unit per config family (ks_*.hip),
// compiled in parallel by build.py and linked into libspprl.so.
static bool find_kset(int algo, int ob, int aout, int ac, bool acmc, bool bf16, KernelSet* ks) {
  if (bf16) {
#if !defined(SPP_ONLY_HOPPER) || defined(SPP_ONLY_BF16)
    return algo == SPP_ALGO_SAC_ACM && kset_sac_bf16(ob, aout, ac, acmc, ks);
#else
    return false;
#endif
  }
  if (algo == SPP_ALGO_SAC) {
#ifndef SPP_ONLY_HOPPER
    return kset_sac_vanilla(ob, aout, ac, acmc, ks);
#else
    return false;
#endif
  }
  if (algo == SPP_ALGO_DDPG) {
#ifndef SPP_ONLY_HOPPER
    return kset_ddpg_vanilla(ob, aout, ac, acmc, ks);
#else
    return false;
#endif
  }
  if (algo == SPP_ALGO_SAC_ACM) {
    if (kset_sac_hopper(ob, aout, ac, acmc, ks)) return true;
#if defined(SPP_ONLY_HOPPER) && defined(SPP_WITH_HCHEETAH)
    if (kset_sac_hcheetah(ob, aout, ac, acmc, ks)) return true;
#endif
#ifndef SPP_ONLY_HOPPER  // kernel-development builds: one instantiation, fast compile
    if (kset_sac_hcheetah(ob, aout, ac, acmc, ks)) return true;
    if (kset_sac_ant(ob, aout, ac, acmc, ks)) return true;
    if (kset_sac_small(ob, aout, ac, acmc, ks)) return true;
  } else if (algo == SPP_ALGO_DDPG_ACM) {
    if (kset_ddpg(ob, aout, ac, acmc, ks)) return true;
    if (kset_ddpg_ant(ob, aout, ac, acmc, ks)) return true;
#endif
  }
  return false;
}

}  // namespace spp

struct sppAgent {
  sppAgentConfig cfg{};
  int device = 0, num_cu = 256;
  bool team_ok = true;  // SPP_SAC_TEAM=0: the one-wave phase kernels at every batch (A/B)
  KernelSet ks{};
  NetBufs net[SPP_NET_COUNT];
  NetLayout lay[SPP_NET_COUNT];  // flat format of each net's parameter / gradient buffer (layout.h); empty: no such net
  int cin = 0, Bmax = 0, Bpmax = 0;
  int64_t steps[4] = {0, 0, 0, 0};  // actor, critic, alpha, acm
  const float *lo = nullptr, *hi = nullptr, *mean = nullptr, *std = nullptr;
  double* alpha_state = nullptr;
  float* alpha_f32 = nullptr;
  DevArray<float> limits;  // [aout] actor lim | [ac] acm lim
  // packed images
  DevArray<float4> pk;     // all matrix images
  std::vector<PackJob> pj;  // the pack jobs as in d_pj: lists [actor | acm | targ | critic]
  int o_pj[PJ_LISTS + 1] = {};  // list l = jobs [o_pj[l], o_pj[l + 1])
  bool ddpg = false;
  // vanilla SAC (SPP_ALGO_SAC): the ACM net exists but is never evaluated; vanilla DDPG (SPP_ALGO_DDPG,
  // ddpg && plain): there is no ACM net at all
  bool plain = false;
  DevArray<PackJob> d_pj;
  // LDS constant-table segments (canonical bias / fc3 vectors, read at kernel start)
  std::vector<TabSeg> tab;
  int tab_floats = 0;  // weight part of the table (make_args appends the limit / normaliser segments)
  ActorDev actor{};
  CriticDev critic[2]{}, targ[2]{};
  AcmDev acm{};
  const float4* acm_W1n = nullptr;  // ACM W1 natural input packing (regression)
  // DDPG_AcM
  BAcmDev bacm{};
  ActorDev actor_targ{};
  const float4 *bacm_W1n = nullptr, *bacm_W21n = nullptr;  // natural-input packings (regression)
  BAcmScratch bz{};  // agent-phase BasicAcM activations
  float *RBH = nullptr, *RBH1 = nullptr, *RS21 = nullptr, *RBP1 = nullptr, *RPZ = nullptr, *RPZ21 = nullptr;
  // scratch
  DevArray<float> scratch;
  float *S = nullptr, *S2 = nullptr, *ACT = nullptr, *AENV = nullptr, *R = nullptr, *DN = nullptr, *EPS1 = nullptr,
        *EPS2 = nullptr;
  float *H1[2] = {}, *H2[2] = {}, *D1[2] = {}, *D2[2] = {}, *DQ[2] = {};
  float *AH1 = nullptr, *AH2 = nullptr, *AD1 = nullptr, *AD2 = nullptr, *ADH = nullptr;
  float *Z1 = nullptr, *Z2 = nullptr, *T3 = nullptr, *part = nullptr;
  float *aux = nullptr;  // [4] alpha grad operand (all-reduced in DP)
  float* GAD = nullptr;       // wide-head actor phase: d a_d hand-over [aout][Bp]
  uint64_t* MASK = nullptr;   // and the trunk's ReLU masks [tile][4][64]
  // min-critic split of the one-wave actor phase (sac.hip: AcmScratch; SPP_MINQ_SPLIT=0: the one-kernel phase, A/B)
  bool minq_split = false;
  // stage split of the phase kernels (sac.hip), one bit per cut; SPP_STAGE_SPLIT=0: today's kernels (A/B).
  //   bit 0  k_sac_actor_heads<C, true> -> k_sac_heads_stage, k_sac_actor_trunk_bwd
  //   bit 1  k_sac_actor_phase<C, true> -> k_sac_trunk_fwd<C, true>, k_sac_squash_stage<C, true>, the critics
  //   bit 2  k_sac_critic_phase         -> k_sac_trunk_fwd<C, false>, k_sac_squash_stage<C, false>, the rest
  int stage_split = 0;
  // wave pairs over a tile's two critics (sac.hip), one bit per kernel; SPP_CRITIC_PAIRS=0: the unpaired kernels (A/B).
  //   bit 0  k_sac_critic_phase<C, true>      -> <C, true, true>        (behind stage-split cut 3)
  //   bit 1  k_sac_actor_phase<C, true, true> -> <C, true, true, true>  (behind stage-split cut 2)
  int critic_pairs = 0;
  // register hand-over forms of the actor trunk kernels (sac.hip), one bit per direction; SPP_ACTOR_GEN=0: the staged kernels (A/B).
  //   bit 0  k_sac_trunk_fwd<C, ACT>  -> k_sac_trunk_fwd_gen<C, ACT>     (each behind its stage-split cut, 2 / 3)
  //   bit 1  k_sac_actor_trunk_bwd    -> k_sac_actor_trunk_bwd_gen       (behind stage-split cut 1)
  int actor_gen = 0;
  float *THD = nullptr, *SCA = nullptr, *SLP = nullptr;  // its hand-overs (SacArgs)
  AcmScratch mq{};  // its hand-over buffers (SEL ... DCA)
  // ACM regression scratch
  float *RX = nullptr, *RZ1 = nullptr, *RZ2 = nullptr, *RP1 = nullptr, *RP2 = nullptr, *RP3 = nullptr;
  // weight-gradient job sets: [0] SAC (critic phase, actor phase), [1] ACM regression
  DwSet dws[2];
  DevArray<AdamJob> d_adam;  // [critic1, critic2 | actor | acm]
  int cur_B = -1;            // staged batch size
  float* w3p[2] = {};         // SAC critics' fused fc3 gradient partials (slabs of the reduce-only dW jobs)
  int64_t w3p_stride = 0;
  float* alpha_grad = nullptr;  // bound operand (defaults to internal scratch)
  // multi-workgroup AcM SGD (sppAcmSgd with bs > kMlR): gradient slabs + parameter buffer, {counter, timeout flag}
  DevArray<float> sgd_slab;
  DevArray<int> sgd_sync;
  int sgd_max_wg = -1;  // co-resident k_mlp_sgd workgroups (acm_sgd_max_wg, cached)
  // per-kernel timing (HIP events on the launch stream)
  bool timing = false;
  std::vector<hipEvent_t> tev[5];
  size_t tused[5] = {0, 0, 0, 0, 0};
};

static void tmark(sppAgent* a, int kind, hipStream_t st) {
  if (!a->timing) return;
  auto& v = a->tev[kind];
  if (a->tused[kind] == v.size()) {
    hipEvent_t e;
    hipEventCreate(&e);
    v.push_back(e);
  }
  hipEventRecord(v[a->tused[kind]++], st);
}

// Build all pack jobs (the parameter pointers must be bound).
static sppStatus build_packs(sppAgent* a) {
  const int ob = a->cfg.ob, aout = a->cfg.aout, ac = a->cfg.ac;
  const int ca = a->cfg.acm_critic ? ac : aout;
  const int cin = ob + ca;
  for (int k = 0; k < SPP_NET_COUNT; ++k)  // every net the handle has (sppAgentCreate)
    SPP_REQUIRE(a->lay[k].size() == 0 || a->net[k].p, SPP_E_STATE, "network %d parameters not bound", k);
  PackPlan pp;
  pp.bf16 = a->cfg.mlp_bf16 ? 1 : 0;
  if (!a->ddpg) {
    // ---- actor: fc1 [256][ob], fc2, fc_prob [aout][256], fc_scale
    const float* P = a->net[SPP_NET_ACTOR].p;
    const NetLayout& L = a->lay[SPP_NET_ACTOR];
    const float *W1 = P + L.w(0), *W2 = P + L.w(1), *Wp = P + L.w(kFcProb), *Ws = P + L.w(kFcScale);
    pp.M(PJ_ACTOR, W1, nullptr, 1 << 30, ob, 0, 0, nat(256), nat(ob), 8, blocks_of(ob), &a->actor.W1);
    pp.M(PJ_ACTOR, W2, nullptr, 1 << 30, 256, 0, 0, nat(256), nat(256), 8, 8, &a->actor.W2, 1);
    pp.M(PJ_ACTOR, Wp, Ws, aout, 256, 0, 0, nat(2 * aout), nat(256), blocks_of(2 * aout), 8, &a->actor.Wh, 1);
    pp.M(PJ_ACTOR, W2, nullptr, 1 << 30, 256, 1, 0, nat(256), nat(256), 8, 8, &a->actor.W2T, 1);
    pp.M(PJ_ACTOR, Wp, Ws, aout, 256, 1, 0, nat(256), pair(aout), 8, (aout + 15) / 16, &a->actor.WhT);
    if (a->cfg.mlp_bf16)  // the two-tile bf16 critic phase squashes in the heads' epilogue (sac_bf.h)
      pp.M(PJ_ACTOR, Wp, Ws, aout, 256, 0, 0, pair(aout), nat(256), (aout + 15) / 16, 8, &a->actor.WhP, 1);
    a->actor.tb1 = pp.T(P + L.b(0), 256);
    a->actor.tb2 = pp.T(P + L.b(1), 256);
    a->actor.tbh = pp.T(P + L.b(kFcProb), aout, P + L.b(kFcScale), aout);
  } else {
    // ---- DDPG actor and its target: fc1 [256][ob], fc2, fc3 [aout][256]
    for (int t = 0; t < 2; ++t) {
      const int netid = t == 0 ? SPP_NET_ACTOR : SPP_NET_ACTOR_TARG;
      const float* P = a->net[netid].p;
      const NetLayout& L = a->lay[netid];
      ActorDev& ad = t == 0 ? a->actor : a->actor_targ;
      const int l = t == 0 ? PJ_ACTOR : PJ_TARG;
      const float *W1 = P + L.w(0), *W2 = P + L.w(1), *W3 = P + L.w(2);
      pp.M(l, W1, nullptr, 1 << 30, ob, 0, 0, nat(256), nat(ob), 8, blocks_of(ob), &ad.W1);
      pp.M(l, W2, nullptr, 1 << 30, 256, 0, 0, nat(256), nat(256), 8, 8, &ad.W2, 1);
      pp.M(l, W3, nullptr, 1 << 30, 256, 0, 0, nat(aout), nat(256), blocks_of(aout), 8, &ad.Wh, 1);
      if (t == 0) {
        pp.M(l, W2, nullptr, 1 << 30, 256, 1, 0, nat(256), nat(256), 8, 8, &ad.W2T, 1);
        pp.M(l, W3, nullptr, 1 << 30, 256, 1, 0, nat(256), nat(aout), 8, blocks_of(aout), &ad.WhT);
      }
      ad.tb1 = pp.T(P + L.b(0), 256);
      ad.tb2 = pp.T(P + L.b(1), 256);
      ad.tbh = pp.T(P + L.b(2), aout);
    }
  }
  const int in = 2 * ob, nbi = blocks_of(ob) + blocks_of(aout);
  if (!a->ddpg) {
    // ---- ACM: fc1 [64][2ob], fc2 [32][64], fc3 [ac][32]
    const float* P = a->net[SPP_NET_ACM].p;
    const NetLayout& L = a->lay[SPP_NET_ACM];
    const float *W1 = P + L.w(0), *W2 = P + L.w(1), *W3 = P + L.w(2);
    pp.M(PJ_ACM, W1, nullptr, 1 << 30, in, 0, 0, nat(64), cat(ob, aout), 2, nbi, &a->acm.W1);
    pp.M(PJ_ACM, W2, nullptr, 1 << 30, 64, 0, 0, nat(32), nat(64), 1, 2, &a->acm.W2);
    pp.M(PJ_ACM, W3, nullptr, 1 << 30, 32, 0, 0, nat(ac), nat(32), 1, 1, &a->acm.W3);
    pp.M(PJ_ACM, W3, nullptr, 1 << 30, 32, 1, 0, nat(32), nat(ac), 1, 1, &a->acm.W3T);
    pp.M(PJ_ACM, W2, nullptr, 1 << 30, 64, 1, 0, nat(64), nat(32), 2, 1, &a->acm.W2T);
    pp.M(PJ_ACM, W1, nullptr, 1 << 30, in, 1, ob, nat(aout), nat(64), blocks_of(aout), 2, &a->acm.W1Ta);
    pp.M(PJ_ACM, W1, nullptr, 1 << 30, in, 0, 0, nat(64), nat(in), 2, blocks_of(in), &a->acm_W1n);
    a->acm.tb1 = pp.T(P + L.b(0), 64);
    a->acm.tb2 = pp.T(P + L.b(1), 32);
    a->acm.tb3 = pp.T(P + L.b(2), ac);
  } else if (!a->plain) {
    // ---- BasicAcM: t, t1, fc1 [100][2ob], fc2 [50][100], fc21 [50][2ob], fc3 [ac][50]
    const float* P = a->net[SPP_NET_ACM].p;
    const NetLayout& L = a->lay[SPP_NET_ACM];
    const float *W1 = P + L.w(0), *W2 = P + L.w(1), *W21 = P + L.w(kBacmFc21), *W3 = P + L.w(kBacmFc3);
    BAcmDev& B = a->bacm;
    pp.M(PJ_ACM, W1, nullptr, 1 << 30, in, 0, 0, nat(100), cat(ob, aout), 4, nbi, &B.W1);
    pp.M(PJ_ACM, W21, nullptr, 1 << 30, in, 0, 0, nat(50), cat(ob, aout), 2, nbi, &B.W21);
    pp.M(PJ_ACM, W2, nullptr, 1 << 30, 100, 0, 0, nat(50), nat(100), 2, 4, &B.W2);
    pp.M(PJ_ACM, W3, nullptr, 1 << 30, 50, 0, 0, nat(ac), nat(50), 1, 2, &B.W3);
    pp.M(PJ_ACM, W3, nullptr, 1 << 30, 50, 1, 0, nat(50), nat(ac), 2, 1, &B.W3T);
    pp.M(PJ_ACM, W2, nullptr, 1 << 30, 100, 1, 0, nat(100), nat(50), 4, 2, &B.W2T);
    pp.M(PJ_ACM, W1, nullptr, 1 << 30, in, 1, ob, nat(aout), nat(100), blocks_of(aout), 4, &B.W1Ta);
    pp.M(PJ_ACM, W21, nullptr, 1 << 30, in, 1, ob, nat(aout), nat(50), blocks_of(aout), 2, &B.W21Ta);
    pp.M(PJ_ACM, W1, nullptr, 1 << 30, in, 0, 0, nat(100), nat(in), 4, blocks_of(in), &a->bacm_W1n);
    pp.M(PJ_ACM, W21, nullptr, 1 << 30, in, 0, 0, nat(50), nat(in), 2, blocks_of(in), &a->bacm_W21n);
    B.tb1 = pp.T(P + L.b(0), 100);
    B.tb21 = pp.T(P + L.b(kBacmFc21), 50);
    B.tb2 = pp.T(P + L.b(1), 50);
    B.tb3 = pp.T(P + L.b(kBacmFc3), ac);
    B.t = P + kBacmT;
    B.t1 = P + kBacmT1;
  }
  // ---- critics and targets: fc1 [256][cin], fc2, fc3 [1][256]
  for (int t = 0; t < 4; ++t) {
    if (a->ddpg && (t == 1 || t == 3)) continue;  // DDPG: one critic and its target
    const int netid = t < 2 ? SPP_NET_CRITIC1 + t : SPP_NET_CRITIC1_TARG + (t - 2);
    CriticDev& cd = t < 2 ? a->critic[t] : a->targ[t - 2];
    const float* P = a->net[netid].p;
    const NetLayout& L = a->lay[netid];
    const float *W1 = P + L.w(0), *W2 = P + L.w(1);
    const int fl = t < 2 ? PJ_CRITIC : PJ_TARG;
    pp.M(fl, W1, nullptr, 1 << 30, cin, 0, 0, nat(256), cat(ob, ca), 8, blocks_of(ob) + blocks_of(ca), &cd.W1);
    pp.M(fl, W2, nullptr, 1 << 30, 256, 0, 0, nat(256), nat(256), 8, 8, &cd.W2, 1);
    if (t < 2) {
      pp.M(fl, W2, nullptr, 1 << 30, 256, 1, 0, nat(256), nat(256), 8, 8, &cd.W2T, 1);
      pp.M(fl, W1, nullptr, 1 << 30, cin, 1, ob, nat(ca), nat(256), blocks_of(ca), 8, &cd.W1Ta, 1);
    }
    cd.tb1 = pp.T(P + L.b(0), 256);
    cd.tb2 = pp.T(P + L.b(1), 256);
    cd.tw3 = pp.T(P + L.w(2), 256);
    cd.b3 = P + L.b(2);
  }
  // + the per-launch limit / normaliser segments appended by make_args
  a->tab = pp.tab;
  a->tab_floats = pp.toff;
  const int extra = 3 * (int)round_up(aout, 32) + (int)round_up(std::max(ac, 1), 32);
  SPP_REQUIRE(pp.toff + extra <= kTabMax && (int)a->tab.size() + 4 <= kTabSegs, SPP_E_SHAPE,
              "LDS table too large (%d floats, %d segments)", pp.toff + extra, (int)a->tab.size() + 4);
  return pp.commit(PJ_LISTS, a->pk, a->d_pj, a->pj, a->o_pj);
}

// pack job lists [first, last) (adjacent in d_pj)
static void launch_pack(sppAgent* a, int first, int last, hipStream_t st) {
  const int off = a->o_pj[first], n = a->o_pj[last] - off;
  if (n > 0) hipLaunchKernelGGL(k_pack_matrix, dim3(64, n), dim3(256), 0, st, (const PackJob*)(a->d_pj.ptr + off));
}

// ---- shared with api_onp.hip (host.h)
namespace spp {

// Split assignment, slab arena, item table (plan_dw, dw_plan.h) and upload of a job set.
sppStatus finalize_dw(DwSet& D, std::vector<DwJob>& jobs, int nph, int Bp, int B, int num_cu) {
  const DwPlan P = plan_dw(jobs, D.j0, D.nj, nph, Bp, num_cu, D.thin_min_bp);
  if (P.need > D.slab.n) {
    D.slab.release();
    SPP_CHECK_HIP(D.slab.alloc(P.need));
  }
  for (size_t j = 0; j < jobs.size(); ++j)
    if (P.slab_off[j] >= 0) jobs[j].slab = D.slab.ptr + P.slab_off[j];
  for (int ph = 0; ph < nph; ++ph) {
    D.nlds[ph] = P.nlds[ph];
    D.nthin[ph] = P.nthin[ph];
    D.max_elems[ph] = P.max_elems[ph];
    D.ioff[ph] = P.ioff[ph];
    D.nitems[ph] = P.nitems[ph];
  }
  const std::vector<int>& items = P.items;
  D.jobs.release();
  D.items.release();
  SPP_CHECK_HIP(D.jobs.alloc(jobs.size()));
  SPP_CHECK_HIP(D.items.alloc(items.size()));
  SPP_CHECK_HIP(hipMemcpy(D.jobs.ptr, jobs.data(), sizeof(DwJob) * jobs.size(), hipMemcpyHostToDevice));
  SPP_CHECK_HIP(hipMemcpy(D.items.ptr, items.data(), sizeof(int) * items.size(), hipMemcpyHostToDevice));
  D.B = B;
  D.bf16 = !jobs.empty() && jobs[0].bf16;
  for (const DwJob& j : jobs)
    if ((j.bf16 != 0) != D.bf16) return SPP_E_STATE;
  return SPP_OK;
}

// Append a weight-gradient job dW [N][K0 + K1] (+ db) = A [N][Bp] x [X0 | X1]; rows >= nrow2 of it go to
// (dW2, db2).  fp32 operands; build_dw marks the bf16 sets' jobs.
DwJob& dw_job(std::vector<DwJob>& jobs, int Bp, const float* A, int N, const float* X0, int K0, const float* X1,
              int K1, float* dW, float* db, int nrow2, float* dW2, float* db2) {
  DwJob j{};
  j.A = A; j.N = N; j.X0 = X0; j.K0 = K0; j.X1 = X1; j.K1 = K1; j.dW = dW; j.db = db; j.Bp = Bp;
  j.nrow2 = nrow2 < 0 ? N : nrow2;
  j.dW2 = dW2; j.db2 = db2;
  j.slab_stride = round_up((int64_t)N * (K0 + K1) + N, 4);
  jobs.push_back(j);
  return jobs.back();
}
// The job of layer i of a net with gradient buffer G: delta A x the layer's input X0, or [X0 | X1 (K1 rows)]
DwJob& layer_dw(std::vector<DwJob>& jobs, int Bp, float* G, const NetLayout& L, int i, const float* A,
                const float* X0, const float* X1, int K1) {
  return dw_job(jobs, Bp, A, L.rows(i), X0, L.cols(i) - K1, X1, K1, G + L.w(i), G + L.b(i));
}

}  // namespace spp

static int phase_grid(sppAgent* a, int Bp) {
  const int ntiles = Bp / 32;
  return std::max(1, std::min(cdiv(ntiles, kWavesPerWG), a->num_cu));
}
// critic / actor phases: the team kernels (one workgroup per tile; sac_team.h, the vanilla DDPG handles'
// ddpg_team.h) while the tiles fit one per CU; SPP_SAC_TEAM=0 keeps the one-wave kernels at every batch
static bool phase_team(sppAgent* a, int Bp) {
  const bool have = a->ddpg ? a->ks.dcritic_team && a->ks.dactor_team : a->ks.critic_team && a->ks.actor_team;
  return have && a->team_ok && Bp / 32 <= a->num_cu;
}
static int tile_grid(sppAgent* a, int Bp) {
  return phase_team(a, Bp) ? std::max(1, std::min(Bp / 32, a->num_cu)) : phase_grid(a, Bp);
}
// the team critic phase splits each tile's two critics over two workgroups while 2 x tiles fit the CUs
static int sac_critic_grid(sppAgent* a, int Bp) {
  const int nt = std::max(1, Bp / 32);
  return phase_team(a, Bp) && 2 * nt <= a->num_cu ? 2 * nt : tile_grid(a, Bp);
}

// Critic i's jobs: fc1 (delta1 x [s|a]), fc2 (delta2 x h1), fc3 (dq x h2).  fuse3: the critic-phase kernel
// computes fc3 itself and writes one [256 | 1] partial per wave, nsplit of them: a reduce-only job, whose index
// is returned (else -1).
static int critic_dw(sppAgent* a, std::vector<DwJob>& jobs, int Bp, int i, bool fuse3, int nsplit) {
  float* G = a->net[SPP_NET_CRITIC1 + i].g;
  const NetLayout& L = a->lay[SPP_NET_CRITIC1 + i];
  layer_dw(jobs, Bp, G, L, 0, a->D1[i], a->S, a->cfg.acm_critic ? a->AENV : a->ACT, a->cin - a->cfg.ob);
  layer_dw(jobs, Bp, G, L, 1, a->D2[i], a->H1[i]);
  if (!fuse3) {
    layer_dw(jobs, Bp, G, L, 2, a->DQ[i], a->H2[i]);
    return -1;
  }
  DwJob& f = layer_dw(jobs, Bp, G, L, 2, nullptr, nullptr);
  f.fused = 1;
  f.nsplit = nsplit;
  f.wsplit = 1;
  return (int)jobs.size() - 1;
}

// (Re)build a weight-gradient job set for batch size B.
//   set 0: the agent update (phase 0 = the critics, phase 1 = actor); set 1: ACM / BasicAcM regression
static sppStatus build_dw(sppAgent* a, int set, int B) {
  const int Bp = (int)round_up(B, 32);
  const int aout = a->cfg.aout;
  std::vector<DwJob> jobs;
  DwSet& D = a->dws[set];
  int nph = 1, fused[2] = {-1, -1};
  if (set == 0) {
    // critic phase.  fc3 is fused on the SAC sets (bf16 sets with SPP_BF16_FUSE3 = 0: the critic phase stores
    // h2 (bf16) and dq; fc3 is a k_dw job) and on the DDPG sets with ob <= 32 (k_ddpg_critic_phase's kFuse3)
    const bool team = phase_team(a, Bp);
    const bool fuse3 = a->ddpg ? a->cfg.ob <= 32 : (!a->cfg.mlp_bf16 || SPP_BF16_FUSE3);
    const int nsplit = a->ddpg ? tile_grid(a, Bp) * (team ? kTeamDCritic : kWavesPerWG)
                               : sac_critic_grid(a, Bp) * (team ? kTeamCritic : kWavesPerWG);
    for (int i = 0; i < (a->ddpg ? 1 : 2); ++i) fused[i] = critic_dw(a, jobs, Bp, i, fuse3, nsplit);
    D.j0[0] = 0;
    D.nj[0] = (int)jobs.size();
    // actor phase: fc1 (delta1 x s), fc2 (delta2 x h1), head (dhead x h2): DDPG's fc3, SAC's [mu | log-std] pair
    float* G = a->net[SPP_NET_ACTOR].g;
    const NetLayout& L = a->lay[SPP_NET_ACTOR];
    layer_dw(jobs, Bp, G, L, 0, a->AD1, a->S);
    layer_dw(jobs, Bp, G, L, 1, a->AD2, a->AH1);
    if (a->ddpg)
      layer_dw(jobs, Bp, G, L, 2, a->ADH, a->AH2);
    else
      dw_job(jobs, Bp, a->ADH, 2 * aout, a->AH2, L.cols(kFcProb), nullptr, 0, G + L.w(kFcProb), G + L.b(kFcProb), aout,
             G + L.w(kFcScale), G + L.b(kFcScale));
    D.j0[1] = D.nj[0];
    D.nj[1] = (int)jobs.size() - D.nj[0];
    nph = 2;
  } else {
    float* G = a->net[SPP_NET_ACM].g;
    const NetLayout& L = a->lay[SPP_NET_ACM];
    if (a->ddpg) {
      SPP_REQUIRE(!a->plain, SPP_E_STATE, "vanilla DDPG has no ACM to regress");
      // BasicAcM regression (acm.py:246-258): fc1, fc2, fc21 (grad of its output = t * dz), fc3;
      // t / t1 come from the per-tile partials (k_finalize_bacm)
      layer_dw(jobs, Bp, G, L, 0, a->RBP1, a->RX);
      layer_dw(jobs, Bp, G, L, 1, a->RPZ, a->RBH);
      layer_dw(jobs, Bp, G, L, kBacmFc21, a->RPZ21, a->RX);
      layer_dw(jobs, Bp, G, L, kBacmFc3, a->RP3, a->RBH1);
    } else {
      layer_dw(jobs, Bp, G, L, 0, a->RP1, a->RX);
      layer_dw(jobs, Bp, G, L, 1, a->RP2, a->RZ1);
      layer_dw(jobs, Bp, G, L, 2, a->RP3, a->RZ2);
    }
    D.j0[0] = 0;
    D.nj[0] = (int)jobs.size();
  }
  if (a->cfg.mlp_bf16) {
    // bf16 SAC kernel sets write these operand arrays as bf16 (op_st, sac.hip); an X1 segment is always
    // staged fp32 input, like a fp32 X0
    std::vector<const float*> b16;
    if (!a->ddpg && set == 0)
      b16 = {a->H1[0], a->H1[1], a->H2[0], a->H2[1], a->D1[0], a->D1[1], a->D2[0], a->D2[1],
             a->AH1, a->AH2, a->AD1, a->AD2};
    auto is16 = [&](const float* p) { return p && std::find(b16.begin(), b16.end(), p) != b16.end(); };
    for (DwJob& j : jobs) {
      j.bf16 = 1;
      j.a_bf = is16(j.A) ? 1 : 0;
      j.x_bf = is16(j.X0) ? 1 : 0;
    }
  }
  const sppStatus s = finalize_dw(D, jobs, nph, Bp, B, a->num_cu);
  if (set == 0) {  // the critics' fused fc3 partials (DDPG: one critic)
    for (int i = 0; i < 2; ++i) {
      const int f = fused[a->ddpg ? 0 : i];
      a->w3p[i] = f >= 0 ? jobs[f].slab : nullptr;
    }
    a->w3p_stride = fused[0] >= 0 ? jobs[fused[0]].slab_stride : 0;
  }
  return s;
}

namespace spp {

void launch_dw_set(DwSet& D, int ph, hipStream_t st) {
  const int* ij = D.items.ptr + D.ioff[ph];
  const int* is = ij + D.nitems[ph];
  const DwJob* jobs = D.jobs.ptr + D.j0[ph];
  launch_dw_kernels(jobs, ij, is, D.nitems[ph], D.nlds[ph], D.nthin[ph], D.nj[ph], D.max_elems[ph], D.bf16,
                    D.big_waves, st);
}

// polls before a k_mlp_sgd arrival wait times out (0: the kernel's default); test hook sppSetSgdSpinLimit
int g_sgd_spin = 0;

// slabs [2][kMlMaxWG][kMlSlabMax] + the parameter buffer [kSgdPubReps][kMlSlabMax] + {arrival counter, timeout flag}
// sync: [0] unused, [1] the sticky timeout flag, [kSgdShardStride (1 + k)] arrival counter shard k (sgd.hip)
constexpr int kSgdSyncInts = kSgdShardStride * (1 + kSgdShards);
int* sgd_ctr(DevArray<int>& sync) { return sync.ptr + kSgdShardStride; }
sppStatus mlp_sgd_buffers(DevArray<float>& slab, DevArray<int>& sync, hipStream_t st) {
  if (!slab.ptr) {
    SPP_CHECK_HIP(slab.alloc((size_t)(2 * kMlMaxWG + kSgdPubReps) * kMlSlabMax));  // slabs, published replicas
    SPP_CHECK_HIP(sync.alloc(kSgdSyncInts));
    SPP_CHECK_HIP(hipMemsetAsync(sync.ptr, 0, kSgdSyncInts * sizeof(int), st));
  }
  // the arrival counter shards (the flag is sticky)
  SPP_CHECK_HIP(hipMemsetAsync(sgd_ctr(sync), 0, kSgdShards * kSgdShardStride * sizeof(int), st));
  return SPP_OK;
}

// optim.hip's kernels for api_onp.hip
void launch_pack_matrix(int gx, int njobs, const PackJob* jobs, hipStream_t st) {
  hipLaunchKernelGGL(k_pack_matrix, dim3(gx, njobs), dim3(256), 0, st, jobs);
}
void launch_adam_kernel(const AdamJob* job, int64_t n, float neg_step, float bc2s, hipStream_t st) {
  hipLaunchKernelGGL(k_adam, dim3(std::max(1, std::min(cdiv(n, 1024), 1024)), 1), dim3(256), 0, st, job, neg_step,
                     bc2s, 0.f);
}

}  // namespace spp

static void launch_dw(sppAgent* a, int set, int ph, hipStream_t st) { launch_dw_set(a->dws[set], ph, st); }

// Adam job table [critic1, critic2 (+polyak targets) | actor | acm]; pointers only.
// DDPG_AcM: [critic (+polyak) | - | actor (+polyak of the target actor, ddpg.py:273-284) | acm].
static sppStatus build_adam(sppAgent* a) {
  AdamJob jobs[4] = {};
  for (int i = 0; i < (a->ddpg ? 1 : 2); ++i) {
    NetBufs& n = a->net[SPP_NET_CRITIC1 + i];
    jobs[i] = AdamJob{n.p, n.g, n.m, n.v, a->net[SPP_NET_CRITIC1_TARG + i].p, n.n};
  }
  NetBufs& na = a->net[SPP_NET_ACTOR];
  jobs[2] = AdamJob{na.p, na.g, na.m, na.v, a->ddpg ? a->net[SPP_NET_ACTOR_TARG].p : nullptr, na.n};
  NetBufs& nm = a->net[SPP_NET_ACM];
  jobs[3] = AdamJob{nm.p, nm.g, nm.m, nm.v, nullptr, nm.n};
  if (!a->d_adam.ptr) SPP_CHECK_HIP(a->d_adam.alloc(4));
  SPP_CHECK_HIP(hipMemcpy(a->d_adam.ptr, jobs, sizeof(jobs), hipMemcpyHostToDevice));
  return SPP_OK;
}

static void launch_adam(sppAgent* a, int first, int count, int64_t n, int64_t step, float lr, float tau,
                        hipStream_t st) {
  const double bc1 = 1.0 - std::pow(0.9, (double)step), bc2s = std::sqrt(1.0 - std::pow(0.999, (double)step));
  hipLaunchKernelGGL(k_adam, dim3(std::max(1, std::min(cdiv(n, 256 * 4), 1024)), count), dim3(256), 0, st,
                     (const AdamJob*)(a->d_adam.ptr + first), (float)(-(lr / bc1)), (float)bc2s, tau);
}

// Workgroups per CU of the stage kernels' grids (their LDS use lets three share a CU)
constexpr int kStageWGPerCU = 3;
constexpr int kStageSplitAll = 7;
constexpr int kStageSplitDefault = kStageSplitAll;
constexpr int kActorGenDefault = 3;  // both bits cleared the bench rule
constexpr int kCriticPairsDefault = 1;  // bit 1 measured inside the run-to-run range: off unless asked for
constexpr int kDwBigWavesDefault = 8;
// The padded batch from which a job set's thin fp32 weight gradients run as k_dw_thin (dw.hip), 0: never.
// SPP_DW_THIN=0 turns the kernel off (every such item then runs in k_dw, as before it existed; the results are the
// same bit for bit; the default is on: DESIGN.md §8, round 16).  SPP_DW_THIN_MIN_BP moves the threshold (default 8192, the LDS kernels' boundary): it exists for
// the tests, which reach parts of one or no step with it.  Read when a job set's owner is made.
static int dw_thin_min_bp() {
  const char* t = getenv("SPP_DW_THIN");
  if (t && atoi(t) == 0) return 0;
  const char* m = getenv("SPP_DW_THIN_MIN_BP");
  const int v = m ? atoi(m) : 8192;
  return v >= 32 ? v : 32;
}
static int stage_grid(sppAgent* a, int Bp) {
  return std::max(1, std::min(cdiv(Bp / 32, kWavesPerWG), kStageWGPerCU * a->num_cu));
}

static SacArgs make_args(sppAgent* a, int B) {
  SacArgs p{};
  p.B = B;
  p.Bp = (int)round_up(B, 32);
  p.inv_B = 1.f / (float)B;
  p.S = a->S; p.S2 = a->S2; p.ACT = a->ACT; p.AENV = a->AENV; p.R = a->R; p.DN = a->DN;
  p.EPS1 = a->EPS1; p.EPS2 = a->EPS2;
  p.min_max = a->cfg.min_max_denormalize;
  p.lo = a->lo; p.hi = a->hi; p.mean = a->mean; p.std = a->std;
  p.actor_lim = a->limits.ptr;
  p.acm_lim = a->limits.ptr + a->cfg.aout;
  p.gamma = a->cfg.gamma;
  p.custom_loss = a->cfg.custom_loss;
  p.norm_closs = a->cfg.norm_closs;
  p.alpha = a->alpha_f32;
  p.actor = a->actor;
  for (int i = 0; i < 2; ++i) {
    p.critic[i] = a->critic[i];
    p.targ[i] = a->targ[i];
    p.H1[i] = a->H1[i]; p.H2[i] = a->H2[i]; p.D1[i] = a->D1[i]; p.D2[i] = a->D2[i]; p.DQ[i] = a->DQ[i];
    p.W3P[i] = a->w3p[i];
  }
  p.w3p_stride = a->w3p_stride;
  p.acm = a->acm;
  p.bacm = a->bacm;
  p.actor_targ = a->actor_targ;
  p.AH1 = a->AH1; p.AH2 = a->AH2; p.AD1 = a->AD1; p.AD2 = a->AD2; p.ADH = a->ADH;
  p.part = a->part;
  p.THD = a->THD; p.SCA = a->SCA; p.SLP = a->SLP;
  p.nseg = (int)a->tab.size();
  for (int i = 0; i < p.nseg; ++i) p.seg[i] = a->tab[i];
  // limits and normaliser vectors (read per output slot by the squash / head epilogues: LDS
  // instead of a global round trip each); unbound vectors read as zeros
  int off = a->tab_floats;
  auto X = [&](const float* v, int n) {
    const int o = off, np = (int)round_up(std::max(n, 1), 32);
    p.seg[p.nseg++] = TabSeg{v ? v : a->limits.ptr, v ? n : 0, np, o, 0};
    off += np;
    return o;
  };
  const int aout = a->cfg.aout;
  p.t_lim = X(a->limits.ptr, aout);
  p.t_alim = X(a->limits.ptr + aout, a->cfg.ac);
  p.t_n0 = X(p.min_max ? a->lo : a->mean, aout);
  p.t_n1 = X(p.min_max ? a->hi : a->std, aout);
  return p;
}

// The stage kernels' argument block: their LDS table holds only the segments they read, packed from offset 0:
// the ACM's three bias vectors and the limit / normaliser vectors (the other networks' bias / fc3 offsets of
// the block are not read by them).
static SacArgs stage_args(const sppAgent* a, const SacArgs& full) {
  SacArgs p = full;
  const int n0 = (int)a->tab.size();
  p.nseg = 0;
  int off = 0;
  auto keep = [&](int i) {
    TabSeg g = full.seg[i];
    g.off = off;
    p.seg[p.nseg++] = g;
    off += g.npad;
    return g.off;
  };
  for (int i = 0; i < n0; ++i) {
    if (full.seg[i].off == full.acm.tb1) p.acm.tb1 = keep(i);
    else if (full.seg[i].off == full.acm.tb2) p.acm.tb2 = keep(i);
    else if (full.seg[i].off == full.acm.tb3) p.acm.tb3 = keep(i);
  }
  p.t_lim = keep(n0); p.t_alim = keep(n0 + 1); p.t_n0 = keep(n0 + 2); p.t_n1 = keep(n0 + 3);
  return p;
}

static sppStatus check_ready(sppAgent* a) {
  SPP_REQUIRE(a->ddpg || (a->alpha_state && a->alpha_f32), SPP_E_STATE, "alpha not bound");
  SPP_REQUIRE(a->cfg.min_max_denormalize ? (a->lo && a->hi) : (a->mean && a->std), SPP_E_STATE,
              "normalizer not bound");
  SPP_REQUIRE(a->limits.ptr, SPP_E_STATE, "limits not set");
  if (!a->pk.ptr) {
    sppStatus s = build_packs(a);
    if (s) return s;
    if ((s = build_adam(a))) return s;
    a->dws[0].B = a->dws[1].B = -1;
  }
  return SPP_OK;
}

extern "C" {

sppStatus sppAgentCreate(sppAgentHandle* out, const sppAgentConfig* cfg, int device) {
  SPP_REQUIRE(out && cfg, SPP_E_INVALID_ARG, "null arg");
  SPP_REQUIRE(cfg->algo == SPP_ALGO_SAC_ACM || cfg->algo == SPP_ALGO_DDPG_ACM || cfg->algo == SPP_ALGO_SAC ||
                  cfg->algo == SPP_ALGO_DDPG,
              SPP_E_INVALID_ARG, "unsupported algo %d", cfg->algo);
  SPP_REQUIRE(cfg->algo != SPP_ALGO_SAC || (cfg->acm_critic == 0 && cfg->aout == cfg->ac && cfg->custom_loss == 0.f),
              SPP_E_INVALID_ARG, "vanilla SAC: the actor emits the env action (aout == ac), no ACM critic / loss");
  SPP_REQUIRE(cfg->algo != SPP_ALGO_DDPG || (cfg->acm_critic == 0 && cfg->aout == cfg->ac && cfg->custom_loss == 0.f),
              SPP_E_INVALID_ARG, "vanilla DDPG: the actor emits the env action (aout == ac), no ACM critic / loss");
  SPP_REQUIRE(cfg->algo != SPP_ALGO_DDPG || cfg->mlp_bf16 == 0, SPP_E_INVALID_ARG, "vanilla DDPG: fp32 only");
  SPP_REQUIRE(cfg->max_batch > 0, SPP_E_INVALID_ARG, "max_batch must be > 0");
  KernelSet ks;
  SPP_REQUIRE(find_kset(cfg->algo, cfg->ob, cfg->aout, cfg->ac, cfg->acm_critic != 0, cfg->mlp_bf16 != 0, &ks),
              SPP_E_SHAPE, "no kernel instantiation for algo %d (ob=%d, aout=%d, ac=%d, bf16=%d)", cfg->algo, cfg->ob,
              cfg->aout, cfg->ac, cfg->mlp_bf16);
  SPP_CHECK_HIP(hipSetDevice(device));
  auto a = std::make_unique<sppAgent>();
  a->cfg = *cfg;
  a->device = device;
  a->ks = ks;
  hipDeviceProp_t prop;
  SPP_CHECK_HIP(hipGetDeviceProperties(&prop, device));
  a->num_cu = prop.multiProcessorCount;
  {
    const char* t = getenv("SPP_SAC_TEAM");
    a->team_ok = !(t && t[0] == '0');
    const char* m = getenv("SPP_MINQ_SPLIT");
    a->minq_split = ks.actor_fwd && ks.actor_minq && ks.actor_bwd && !(m && m[0] == '0');
    const char* g = getenv("SPP_STAGE_SPLIT");
    const int want = g ? atoi(g) : kStageSplitDefault;
    const bool tab_fits = 128 + 3 * round_up(std::max(cfg->aout, 1), 32) + round_up(std::max(cfg->ac, 1), 32) <= kStageTab;
    const bool have = ks.heads_stage && ks.trunk_bwd && ks.trunk_fwd_a && ks.squash_a && ks.critics_a &&
                      ks.trunk_fwd_c && ks.squash_c && ks.critic_rest;
    if (a->minq_split && have && tab_fits) a->stage_split = want & kStageSplitAll;
    const char* cp = getenv("SPP_CRITIC_PAIRS");
    const int wantp = cp ? atoi(cp) : kCriticPairsDefault;
    if ((a->stage_split & 4) && ks.critic_rest_pair) a->critic_pairs |= wantp & 1;
    if ((a->stage_split & 2) && ks.critics_a_pair) a->critic_pairs |= wantp & 2;
    // SAC_AcM handles (the vanilla handles train at team-kernel batch sizes)
    const char* ag = getenv("SPP_ACTOR_GEN");
    const int wantg = ag ? atoi(ag) : kActorGenDefault;
    const bool acm = cfg->algo == SPP_ALGO_SAC_ACM;
    if (acm && (a->stage_split & 6) && ks.trunk_fwd_a_gen && ks.trunk_fwd_c_gen) a->actor_gen |= wantg & 1;
    if (acm && (a->stage_split & 1) && ks.trunk_bwd_gen) a->actor_gen |= wantg & 2;
    // waves of the fp32 256 x 256 weight-gradient kernel (dw.hip): 8 = k_dw_big8, 4 = k_dw_big; the bf16 sets'
    // k_dw_big16 has 4
    const char* bw = getenv("SPP_DW_BIG_WAVES");
    const int wantw = bw ? atoi(bw) : kDwBigWavesDefault;
    for (DwSet& D : a->dws) D.big_waves = wantw == 8 && !cfg->mlp_bf16 ? 8 : 4;
    for (DwSet& D : a->dws) D.thin_min_bp = dw_thin_min_bp();
  }
  const int ob = cfg->ob, aout = cfg->aout, ac = cfg->ac;
  a->cin = ob + (cfg->acm_critic ? ac : aout);
  a->ddpg = cfg->algo == SPP_ALGO_DDPG_ACM || cfg->algo == SPP_ALGO_DDPG;
  a->plain = cfg->algo == SPP_ALGO_SAC || cfg->algo == SPP_ALGO_DDPG;
  const bool dd = a->ddpg;
  a->lay[SPP_NET_ACTOR] = dd ? ddpg_actor_layout(ob, aout) : sac_actor_layout(ob, aout);
  if (dd) a->lay[SPP_NET_ACTOR_TARG] = a->lay[SPP_NET_ACTOR];
  a->lay[SPP_NET_CRITIC1] = a->lay[SPP_NET_CRITIC1_TARG] = critic_layout(a->cin);
  if (!dd) a->lay[SPP_NET_CRITIC2] = a->lay[SPP_NET_CRITIC2_TARG] = critic_layout(a->cin);
  if (!dd) a->lay[SPP_NET_ACM] = acm_layout(2 * ob, ac);
  else if (!a->plain) a->lay[SPP_NET_ACM] = bacm_layout(2 * ob, ac);
  a->Bmax = cfg->max_batch;
  const int64_t Bp = round_up(cfg->max_batch, 32);
  SPP_REQUIRE((int64_t)Bp * 256 * 4 < ((int64_t)1 << 31), SPP_E_SHAPE, "max_batch %d too large (31-bit buffer offsets)",
              cfg->max_batch);
  a->Bpmax = (int)Bp;
  const int64_t ntiles = Bp / 32;
  // scratch arena
  const int64_t per = Bp;
  int64_t total = 0;
  auto take = [&](int64_t rows) { int64_t o = total; total += rows * per; return o; };
  const int64_t oS = take(ob), oS2 = take(ob), oACT = take(aout), oAENV = take(ac), oR = take(1), oDN = take(1),
                oE1 = take(aout), oE2 = take(aout);
  int64_t oH1[2] = {}, oH2[2] = {}, oD1[2] = {}, oD2[2] = {}, oDQ[2] = {};
  for (int i = 0; i < (dd ? 1 : 2); ++i) {
    oH1[i] = take(256); oH2[i] = take(256); oD1[i] = take(256); oD2[i] = take(256); oDQ[i] = take(1);
  }
  const int64_t oAH1 = take(256), oAH2 = take(256), oAD1 = take(256), oAD2 = take(256), oADH = take(2 * aout);
  // ACM activations kept for its backward: AcM z1 [64], z2 [32], t3 [ac]; BasicAcM h [128], h1 [64], r3 [ac]
  const int64_t oZ1 = take(dd ? 128 : 64), oZ2 = take(dd ? 64 : 32), oT3 = take(ac);
  const int64_t oRX = take(2 * ob), oRZ1 = take(dd ? 128 : 64), oRZ2 = take(dd ? 64 : 32), oRP1 = take(dd ? 128 : 64),
                oRP2 = take(dd ? 64 : 32), oRP3 = take(ac);
  const int64_t oRS21 = dd ? take(64) : 0, oRPZ21 = dd ? take(64) : 0;
  // wide-head actor phase hand-over: d a_d [aout][Bp], ReLU masks (4 x u64 per lane = 16 floats per sample)
  const int64_t oGAD = take(aout), oMASK = take(16);
  // min-critic split hand-over (AcmScratch): selectors (1 B per sample), both critics' masks (128 B per sample),
  // per-tile counts | list offsets | list lengths (ntiles + 2 ntiles + 2 words <= Bp), the two lists, and
  // d q_i / d (critic action input) [CA][Bp] per critic
  const bool mq = a->minq_split;
  const int64_t ca = a->cin - ob;
  const int64_t oSEL = mq ? take(1) : 0, oCM = mq ? take(32) : 0, oCNT = mq ? take(1) : 0, oLIST = mq ? take(2) : 0,
                oDCA = mq ? take(2 * ca) : 0;
  // stage split hand-overs: target heads, the critics' action input, log pi
  const bool ss = a->stage_split != 0;
  const int64_t oTHD = ss ? take(2 * aout) : 0, oSCA = ss ? take(ca) : 0, oSLP = ss ? take(1) : 0;
  const int64_t oPart = total;
  total += ntiles * kBParts + 64;
  const int64_t oAux = total;
  total += 16;
  hipError_t e = a->scratch.alloc(total);
  if (e != hipSuccess) {
    set_error("scratch alloc %.2f GB: %s", total * 4.0 / 1e9, hipGetErrorString(e));
    return SPP_E_OOM;
  }
  SPP_CHECK_HIP(hipMemset(a->scratch.ptr, 0, sizeof(float) * total));
  float* b = a->scratch.ptr;
  a->S = b + oS; a->S2 = b + oS2; a->ACT = b + oACT; a->AENV = b + oAENV; a->R = b + oR; a->DN = b + oDN;
  a->EPS1 = b + oE1; a->EPS2 = b + oE2;
  for (int i = 0; i < 2; ++i) {
    a->H1[i] = b + oH1[i]; a->H2[i] = b + oH2[i]; a->D1[i] = b + oD1[i]; a->D2[i] = b + oD2[i]; a->DQ[i] = b + oDQ[i];
  }
  a->AH1 = b + oAH1; a->AH2 = b + oAH2; a->AD1 = b + oAD1; a->AD2 = b + oAD2; a->ADH = b + oADH;
  a->Z1 = b + oZ1; a->Z2 = b + oZ2; a->T3 = b + oT3;
  a->GAD = b + oGAD;
  a->MASK = reinterpret_cast<uint64_t*>(b + oMASK);
  if (mq) {
    AcmScratch& q = a->mq;
    q.Z1 = a->Z1; q.Z2 = a->Z2; q.T3 = a->T3; q.GAD = a->GAD; q.MASK = a->MASK;
    q.SEL = reinterpret_cast<uint8_t*>(b + oSEL);
    q.CM = reinterpret_cast<uint64_t*>(b + oCM);
    q.CNT = reinterpret_cast<uint32_t*>(b + oCNT);
    q.OFF = q.CNT + ntiles;
    q.NG = reinterpret_cast<int*>(q.OFF + 2 * ntiles);
    q.LIST[0] = reinterpret_cast<int*>(b + oLIST);
    q.LIST[1] = q.LIST[0] + Bp;
    q.DCA[0] = b + oDCA;
    q.DCA[1] = q.DCA[0] + ca * Bp;
  }
  if (ss) {
    a->THD = b + oTHD; a->SCA = b + oSCA; a->SLP = b + oSLP;
  }
  a->RX = b + oRX; a->RZ1 = b + oRZ1; a->RZ2 = b + oRZ2; a->RP1 = b + oRP1; a->RP2 = b + oRP2; a->RP3 = b + oRP3;
  if (dd) {
    a->bz = BAcmScratch{a->Z1, a->Z2, a->T3};
    a->RBH = a->RZ1; a->RBH1 = a->RZ2; a->RBP1 = a->RP1; a->RPZ = a->RP2;
    a->RS21 = b + oRS21; a->RPZ21 = b + oRPZ21;
  }
  a->part = b + oPart;
  a->aux = b + oAux;
  SPP_CHECK_HIP(a->limits.alloc(aout + ac));
  *out = a.release();
  return SPP_OK;
}

sppStatus sppAgentDestroy(sppAgentHandle a) {
  if (!a) return SPP_OK;
  hipSetDevice(a->device);
  hipDeviceSynchronize();
  a->limits.release(); a->pk.release(); a->d_pj.release();
  for (auto& v : a->tev)
    for (auto e : v) hipEventDestroy(e);
  a->scratch.release(); a->d_adam.release();
  for (auto& D : a->dws) D.release();
  delete a;
  return SPP_OK;
}

sppStatus sppAgentNetSize(sppAgentHandle a, int net, int64_t* n) {
  SPP_REQUIRE(a && n && net >= 0 && net < SPP_NET_COUNT, SPP_E_INVALID_ARG, "bad net id");
  *n = a->lay[net].size();
  return SPP_OK;
}

sppStatus sppAgentBindNet(sppAgentHandle a, int net, float* p, float* g, float* m, float* v) {
  SPP_REQUIRE(a && net >= 0 && net < SPP_NET_COUNT && p, SPP_E_INVALID_ARG, "bind: bad args");
  const bool trainable = net == SPP_NET_ACTOR || net == SPP_NET_CRITIC1 || net == SPP_NET_CRITIC2 || net == SPP_NET_ACM;
  SPP_REQUIRE(!trainable || (g && m && v), SPP_E_INVALID_ARG, "bind: trainable net %d needs grad/m/v", net);
  const bool changed = a->net[net].p != p || a->net[net].g != g;
  a->net[net] = NetBufs{p, g, m, v, a->lay[net].size()};
  if (changed) {  // pack tables and gradient jobs hold these pointers
    a->pk.release();
    a->pj.clear();
    a->tab.clear();
  }
  return SPP_OK;
}

sppStatus sppAgentSetLimits(sppAgentHandle a, const float* actor_lim, const float* acm_lim) {
  SPP_REQUIRE(a && actor_lim && acm_lim, SPP_E_INVALID_ARG, "null");
  SPP_CHECK_HIP(hipMemcpy(a->limits.ptr, actor_lim, sizeof(float) * a->cfg.aout, hipMemcpyHostToDevice));
  SPP_CHECK_HIP(hipMemcpy(a->limits.ptr + a->cfg.aout, acm_lim, sizeof(float) * a->cfg.ac, hipMemcpyHostToDevice));
  return SPP_OK;
}

sppStatus sppAgentBindNormalizer(sppAgentHandle a, const float* lo, const float* hi, const float* mean,
                                 const float* std) {
  SPP_REQUIRE(a, SPP_E_INVALID_ARG, "null");
  a->lo = lo; a->hi = hi; a->mean = mean; a->std = std;
  return SPP_OK;
}

sppStatus sppAgentBindAlpha(sppAgentHandle a, double* st, float* af) {
  SPP_REQUIRE(a && st && af, SPP_E_INVALID_ARG, "null");
  a->alpha_state = st;
  a->alpha_f32 = af;
  return SPP_OK;
}

sppStatus sppAgentSetLr(sppAgentHandle a, float actor_lr, float critic_lr, float alpha_lr, float acm_lr) {
  SPP_REQUIRE(a, SPP_E_INVALID_ARG, "null handle");
  if (actor_lr >= 0.f) a->cfg.actor_lr = actor_lr;
  if (critic_lr >= 0.f) a->cfg.critic_lr = critic_lr;
  if (alpha_lr >= 0.f) a->cfg.alpha_lr = alpha_lr;
  if (acm_lr >= 0.f) a->cfg.acm_lr = acm_lr;
  return SPP_OK;
}
sppStatus sppAgentSetSteps(sppAgentHandle a, int64_t s0, int64_t s1, int64_t s2, int64_t s3) {
  SPP_REQUIRE(a, SPP_E_INVALID_ARG, "null");
  a->steps[0] = s0; a->steps[1] = s1; a->steps[2] = s2; a->steps[3] = s3;
  return SPP_OK;
}
sppStatus sppAgentGetSteps(sppAgentHandle a, int64_t* s) {
  SPP_REQUIRE(a && s, SPP_E_INVALID_ARG, "null");
  for (int i = 0; i < 4; ++i) s[i] = a->steps[i];
  return SPP_OK;
}

static sppStatus stage(sppAgentHandle a, const sppBatch* bt, const float* e1, const float* e2, hipStream_t st) {
  SPP_REQUIRE(bt && bt->B > 0 && bt->B <= a->Bmax, SPP_E_SHAPE, "batch B=%d outside (0, max_batch=%d]",
              bt ? bt->B : -1, a->Bmax);
  SPP_REQUIRE(bt->obs && bt->next_obs && bt->reward && bt->done && bt->acm_action, SPP_E_INVALID_ARG,
              "batch: null field");
  SPP_REQUIRE(a->cfg.acm_critic || bt->action, SPP_E_INVALID_ARG, "batch.action required without acm_critic");
  StageArgs s{};
  s.B = bt->B; s.Bp = (int)round_up(bt->B, 32); s.ob = a->cfg.ob; s.aout = a->cfg.aout; s.ac = a->cfg.ac;
  s.obs = bt->obs; s.next_obs = bt->next_obs; s.act = bt->action; s.rew = bt->reward; s.acm = bt->acm_action;
  s.done = bt->done; s.eps1 = e1; s.eps2 = e2;
  s.S = a->S; s.S2 = a->S2; s.ACT = a->ACT; s.AENV = a->AENV; s.R = a->R; s.DN = a->DN; s.EPS1 = a->EPS1;
  s.EPS2 = a->EPS2;
  hipLaunchKernelGGL(k_stage_batch, dim3(cdiv(s.Bp, 256)), dim3(256), 0, st, s);
  a->cur_B = bt->B;
  return SPP_OK;
}

static sppStatus critic_grads_staged(sppAgentHandle a, float* losses, hipStream_t st) {
  SPP_REQUIRE(!a->ddpg, SPP_E_STATE, "not a SAC_AcM agent");
  const int B = a->cur_B;
  SPP_REQUIRE(B > 0, SPP_E_STATE, "no staged batch");
  sppStatus s = check_ready(a);
  if (s) return s;
  if (a->dws[0].B != B) {
    s = build_dw(a, 0, B);
    if (s) return s;
  }
  // pack actor, ACM, targets, critics (current weights)
  launch_pack(a, PJ_ACTOR, PJ_LISTS, st);
  SacArgs p = make_args(a, B);
  const int grid = sac_critic_grid(a, p.Bp);
  tmark(a, 0, st);
  const bool team = phase_team(a, p.Bp);
  if (!team && (a->stage_split & 4)) {
    // stage split: the target actor's trunk; the squash and the ACM forward; both target critics and the critics
    hipLaunchKernelGGL((a->actor_gen & 1) ? a->ks.trunk_fwd_c_gen : a->ks.trunk_fwd_c, dim3(tile_grid(a, p.Bp)), dim3(256), 0, st, p, a->mq);
    hipLaunchKernelGGL(a->ks.squash_c, dim3(stage_grid(a, p.Bp)), dim3(256), 0, st, stage_args(a, p), a->mq);
    hipLaunchKernelGGL((a->critic_pairs & 1) ? a->ks.critic_rest_pair : a->ks.critic_rest, dim3(grid), dim3(256), 0, st, p);
  } else {
    hipLaunchKernelGGL(team ? a->ks.critic_team : a->ks.critic, dim3(grid), dim3(team ? 64 * kTeamCritic : 256), 0, st, p);
  }
  tmark(a, 0, st);
  SPP_CHECK_HIP(hipGetLastError());
  tmark(a, 2, st);
  launch_dw(a, 0, 0, st);
  tmark(a, 2, st);
  hipLaunchKernelGGL(k_finalize_critic, dim3(1), dim3(kFinThreads), 0, st, (const float*)a->part, p.Bp / 32, B, losses);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppSacAcmCriticGrads(sppAgentHandle a, const sppBatch* bt, const float* eps_next, float* losses,
                               void* stream) {
  SPP_REQUIRE(a, SPP_E_INVALID_ARG, "null");
  if (bt) {
    sppStatus s = stage(a, bt, eps_next, nullptr, S(stream));
    if (s) return s;
  } else if (eps_next) {
    const int Bp = (int)round_up(a->cur_B, 32);
    SPP_REQUIRE(a->cur_B > 0, SPP_E_STATE, "no staged batch");
    hipLaunchKernelGGL(k_eps_copy_fm, dim3(cdiv((int64_t)a->cfg.aout * Bp, 256)), dim3(256), 0, S(stream), eps_next,
                       a->EPS1, a->cfg.aout, a->cur_B, Bp);
  }
  return critic_grads_staged(a, losses, S(stream));
}

sppStatus sppSacAcmCriticApply(sppAgentHandle a, void* stream) {
  SPP_REQUIRE(a && a->d_adam.ptr, SPP_E_STATE, "agent not ready");
  a->steps[1] += 1;
  tmark(a, 3, S(stream));
  launch_adam(a, 0, 2, a->net[SPP_NET_CRITIC1].n, a->steps[1], a->cfg.critic_lr, a->cfg.tau, S(stream));
  tmark(a, 3, S(stream));
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

static sppStatus actor_grads(sppAgentHandle a, float* losses, hipStream_t st) {
  SPP_REQUIRE(!a->ddpg, SPP_E_STATE, "not a SAC_AcM agent");
  const int B = a->cur_B;
  SPP_REQUIRE(B > 0, SPP_E_STATE, "no staged batch");
  // repack the updated critics
  launch_pack(a, PJ_CRITIC, PJ_LISTS, st);
  SacArgs p = make_args(a, B);
  AcmScratch z{a->Z1, a->Z2, a->T3, a->GAD, a->MASK};
  const int grid = tile_grid(a, p.Bp);
  tmark(a, 1, st);
  const bool team = phase_team(a, p.Bp);
  if (!team && a->minq_split) {
    // min-critic split: forward to q = min(Q1, Q2); the two lists of samples by chosen critic; that critic's
    // backward over the regrouped samples; everything behind it in the original order (sac.hip)
    z = a->mq;
    if (a->stage_split & 2) {
      hipLaunchKernelGGL((a->actor_gen & 1) ? a->ks.trunk_fwd_a_gen : a->ks.trunk_fwd_a, dim3(grid), dim3(256), 0, st, p, z);
      hipLaunchKernelGGL(a->ks.squash_a, dim3(stage_grid(a, p.Bp)), dim3(256), 0, st, stage_args(a, p), z);
      hipLaunchKernelGGL((a->critic_pairs & 2) ? a->ks.critics_a_pair : a->ks.critics_a, dim3(grid), dim3(256), 0, st, p, z);
    } else {
      hipLaunchKernelGGL(a->ks.actor_fwd, dim3(grid), dim3(256), 0, st, p, z);
    }
    hipLaunchKernelGGL(k_minq_scan, dim3(1), dim3(kMinqScanThreads), 0, st, (const uint32_t*)z.CNT, z.OFF, z.NG, p.Bp / 32);
    hipLaunchKernelGGL(k_minq_scatter, dim3(cdiv(p.Bp, 256)), dim3(256), 0, st, (const uint8_t*)z.SEL,
                       (const uint32_t*)z.OFF, z.LIST[0], z.LIST[1], p.Bp);
    hipLaunchKernelGGL(a->ks.actor_minq, dim3(grid), dim3(256), 0, st, p, z);
    if (a->stage_split & 1) {
      hipLaunchKernelGGL(a->ks.heads_stage, dim3(stage_grid(a, p.Bp)), dim3(256), 0, st, stage_args(a, p), z);
      hipLaunchKernelGGL((a->actor_gen & 2) ? a->ks.trunk_bwd_gen : a->ks.trunk_bwd, dim3(grid), dim3(256), 0, st, p, z);
    } else {
      hipLaunchKernelGGL(a->ks.actor_bwd, dim3(grid), dim3(256), 0, st, p, z);
    }
  } else {
    hipLaunchKernelGGL(team ? a->ks.actor_team : a->ks.actor, dim3(grid), dim3(team ? 64 * kTeamActor : 256), 0, st, p, z);
    if (a->ks.actor_heads) hipLaunchKernelGGL(a->ks.actor_heads, dim3(grid), dim3(256), 0, st, p, z);
  }
  tmark(a, 1, st);
  SPP_CHECK_HIP(hipGetLastError());
  tmark(a, 2, st);
  launch_dw(a, 0, 1, st);
  tmark(a, 2, st);
  hipLaunchKernelGGL(k_actor_partials, dim3(1), dim3(kFinThreads), 0, st, (const float*)a->part, p.Bp / 32, B, a->cfg.aout,
                     a->cfg.custom_loss, (double)a->cfg.target_entropy, a->alpha_grad ? a->alpha_grad : a->aux,
                     losses);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppSacAcmActorGrads(sppAgentHandle a, const float* eps_cur, float* losses, void* stream) {
  SPP_REQUIRE(a, SPP_E_INVALID_ARG, "null");
  const int B = a->cur_B;
  SPP_REQUIRE(B > 0, SPP_E_STATE, "no staged batch");
  const int Bp = (int)round_up(B, 32);
  if (eps_cur)
    hipLaunchKernelGGL(k_eps_copy_fm, dim3(cdiv((int64_t)a->cfg.aout * Bp, 256)), dim3(256), 0, S(stream), eps_cur,
                       a->EPS2, a->cfg.aout, B, Bp);
  return actor_grads(a, losses, S(stream));
}

sppStatus sppAgentStageSplit(sppAgentHandle a, int* bits_out) {
  SPP_REQUIRE(a && bits_out, SPP_E_INVALID_ARG, "null");
  *bits_out = a->stage_split;
  return SPP_OK;
}

sppStatus sppAgentCriticPairs(sppAgentHandle a, int* bits_out) {
  SPP_REQUIRE(a && bits_out, SPP_E_INVALID_ARG, "null");
  *bits_out = a->critic_pairs;
  return SPP_OK;
}

sppStatus sppAgentActorGen(sppAgentHandle a, int* bits_out) {
  SPP_REQUIRE(a && bits_out, SPP_E_INVALID_ARG, "null");
  *bits_out = a->actor_gen;
  return SPP_OK;
}

sppStatus sppAgentDwBigWaves(sppAgentHandle a, int* waves_out) {
  SPP_REQUIRE(a && waves_out, SPP_E_INVALID_ARG, "null");
  *waves_out = a->dws[0].big_waves;
  return SPP_OK;
}

sppStatus sppAgentDwThin(sppAgentHandle a, int* items_out) {
  SPP_REQUIRE(a && items_out, SPP_E_INVALID_ARG, "null");
  *items_out = 0;
  for (const DwSet& D : a->dws)
    if (D.B >= 0) *items_out += D.nthin[0] + D.nthin[1];
  return SPP_OK;
}

sppStatus sppAgentBindAlphaGrad(sppAgentHandle a, float* g) {
  SPP_REQUIRE(a, SPP_E_INVALID_ARG, "null");
  a->alpha_grad = g;
  return SPP_OK;
}

sppStatus sppSacAcmDrawEps(sppAgentHandle a, uint64_t seed, uint64_t counter, void* stream) {
  SPP_REQUIRE(a && a->cur_B > 0, SPP_E_STATE, "no staged batch");
  const int B = a->cur_B, Bp = (int)round_up(B, 32);
  SPP_REQUIRE((int64_t)a->cfg.aout * Bp < ((int64_t)1 << 31), SPP_E_SHAPE, "draw_eps: aout * Bp >= 2^31");
  const int64_t quads = (int64_t)a->cfg.aout * Bp / 4;
  // EPS1 (counter 2c) and EPS2 (2c + 1) in one launch (grid.y)
  hipLaunchKernelGGL(k_eps_fm, dim3(cdiv(quads, 256), 2), dim3(256), 0, S(stream), a->EPS1, a->cfg.aout, B, Bp, seed,
                     2 * counter, a->EPS2, 2 * counter + 1);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppAgentReadEps(sppAgentHandle a, int which, float* out, void* stream) {
  SPP_REQUIRE(a && out && (which == 0 || which == 1), SPP_E_INVALID_ARG, "read_eps: bad args");
  SPP_REQUIRE(a->cur_B > 0, SPP_E_STATE, "no staged batch");
  const int B = a->cur_B, Bp = (int)round_up(B, 32);
  hipLaunchKernelGGL(k_eps_read_fm, dim3(cdiv((int64_t)a->cfg.aout * B, 256)), dim3(256), 0, S(stream),
                     (const float*)(which ? a->EPS2 : a->EPS1), out, a->cfg.aout, B, Bp);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

// The packed weight images that hold parameters of `net` (test access, see sppAgentUnpackImage).
static std::vector<PackJob> images_of(sppAgent* a, int net) {
  std::vector<PackJob> out;
  const NetBufs& nb = a->net[net];
  if (!nb.p) return out;
  for (const PackJob& j : a->pj)
    if (j.W >= nb.p && j.W < nb.p + nb.n) out.push_back(j);
  return out;
}

sppStatus sppAgentImageCount(sppAgentHandle a, int net, int* n) {
  SPP_REQUIRE(a && n && net >= 0 && net < SPP_NET_COUNT, SPP_E_INVALID_ARG, "image_count: bad args");
  *n = (int)images_of(a, net).size();
  return SPP_OK;
}

sppStatus sppAgentUnpackImage(sppAgentHandle a, int net, int i, float* out, void* stream) {
  SPP_REQUIRE(a && out && net >= 0 && net < SPP_NET_COUNT, SPP_E_INVALID_ARG, "unpack_image: bad args");
  const std::vector<PackJob> js = images_of(a, net);
  SPP_REQUIRE(i >= 0 && i < (int)js.size(), SPP_E_INVALID_ARG, "unpack_image: image %d of %d", i, (int)js.size());
  hipLaunchKernelGGL(k_unpack_matrix, dim3(64), dim3(256), 0, S(stream), js[i], (const float*)a->net[net].p, out);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppAgentSetTiming(sppAgentHandle a, int enable) {
  SPP_REQUIRE(a, SPP_E_INVALID_ARG, "null");
  a->timing = enable != 0;
  return SPP_OK;
}

sppStatus sppAgentGetTiming(sppAgentHandle a, double* ms, int64_t* cnt) {
  SPP_REQUIRE(a && ms && cnt, SPP_E_INVALID_ARG, "null");
  for (int k = 0; k < 5; ++k) {
    double t = 0.0;
    for (size_t i = 0; i + 1 < a->tused[k]; i += 2) {
      SPP_CHECK_HIP(hipEventSynchronize(a->tev[k][i + 1]));
      float e = 0.f;
      SPP_CHECK_HIP(hipEventElapsedTime(&e, a->tev[k][i], a->tev[k][i + 1]));
      t += e;
    }
    ms[k] = t;
    cnt[k] = (int64_t)(a->tused[k] / 2);
    a->tused[k] = 0;
  }
  return SPP_OK;
}

static sppStatus actor_apply(sppAgentHandle a, float* losses, hipStream_t st) {
  a->steps[0] += 1;
  a->steps[2] += 1;
  tmark(a, 3, st);
  launch_adam(a, 2, 1, a->net[SPP_NET_ACTOR].n, a->steps[0], a->cfg.actor_lr, 0.f, st);
  tmark(a, 3, st);
  hipLaunchKernelGGL(k_alpha_step, dim3(1), dim3(64), 0, st, (const float*)(a->alpha_grad ? a->alpha_grad : a->aux),
                     (double)a->cfg.alpha_lr, a->steps[2], a->alpha_state, a->alpha_f32, losses);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppSacAcmActorApply(sppAgentHandle a, float* losses, void* stream) {
  SPP_REQUIRE(a, SPP_E_INVALID_ARG, "null");
  return actor_apply(a, losses, S(stream));
}

sppStatus sppSacAcmUpdate(sppAgentHandle a, const sppBatch* bt, const float* eps_next, const float* eps_cur,
                          float* losses, void* stream) {
  SPP_REQUIRE(a && !a->ddpg, SPP_E_STATE, "not a SAC_AcM agent");
  SPP_REQUIRE(a && eps_next && eps_cur, SPP_E_INVALID_ARG, "eps required (use sppSacAcmUpdateStaged for device draws)");
  hipStream_t st = S(stream);
  sppStatus s = stage(a, bt, eps_next, eps_cur, st);
  if (s) return s;
  if ((s = critic_grads_staged(a, losses, st))) return s;
  if ((s = sppSacAcmCriticApply(a, stream))) return s;
  if ((s = actor_grads(a, losses, st))) return s;
  return actor_apply(a, losses, st);
}

// ------------------------------------------------------------------ DDPG_AcM (ddpg_acm.py:147-201)
sppStatus sppDdpgAcmCriticGrads(sppAgentHandle a, const sppBatch* bt, float* losses, void* stream) {
  SPP_REQUIRE(a && a->ddpg, SPP_E_STATE, "not a DDPG_AcM agent");
  hipStream_t st = S(stream);
  sppStatus s;
  if (bt && (s = stage(a, bt, nullptr, nullptr, st))) return s;
  const int B = a->cur_B;
  SPP_REQUIRE(B > 0, SPP_E_STATE, "no staged batch");
  if ((s = check_ready(a))) return s;
  if (a->dws[0].B != B && (s = build_dw(a, 0, B))) return s;
  launch_pack(a, PJ_ACTOR, PJ_LISTS, st);
  SacArgs p = make_args(a, B);
  tmark(a, 0, st);
  const bool team = phase_team(a, p.Bp);
  hipLaunchKernelGGL(team ? a->ks.dcritic_team : a->ks.dcritic, dim3(tile_grid(a, p.Bp)),
                     dim3(team ? 64 * kTeamDCritic : 256), 0, st, p, a->bz);
  tmark(a, 0, st);
  SPP_CHECK_HIP(hipGetLastError());
  tmark(a, 2, st);
  launch_dw(a, 0, 0, st);
  tmark(a, 2, st);
  hipLaunchKernelGGL(k_finalize_ddpg_critic, dim3(1), dim3(kFinThreads), 0, st, (const float*)a->part, p.Bp / 32, B, losses);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppDdpgAcmCriticApply(sppAgentHandle a, void* stream) {
  SPP_REQUIRE(a && a->ddpg && a->d_adam.ptr, SPP_E_STATE, "DDPG_AcM agent not ready");
  a->steps[1] += 1;
  tmark(a, 3, S(stream));
  launch_adam(a, 0, 1, a->net[SPP_NET_CRITIC1].n, a->steps[1], a->cfg.critic_lr, a->cfg.tau, S(stream));
  tmark(a, 3, S(stream));
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppDdpgAcmActorGrads(sppAgentHandle a, float* losses, void* stream) {
  SPP_REQUIRE(a && a->ddpg && a->cur_B > 0, SPP_E_STATE, "DDPG_AcM agent: no staged batch");
  hipStream_t st = S(stream);
  const int B = a->cur_B;
  launch_pack(a, PJ_CRITIC, PJ_LISTS, st);  // the updated critic
  SacArgs p = make_args(a, B);
  tmark(a, 1, st);
  const bool team = phase_team(a, p.Bp);
  hipLaunchKernelGGL(team ? a->ks.dactor_team : a->ks.dactor, dim3(tile_grid(a, p.Bp)),
                     dim3(team ? 64 * kTeamDActor : 256), 0, st, p, a->bz);
  tmark(a, 1, st);
  SPP_CHECK_HIP(hipGetLastError());
  tmark(a, 2, st);
  launch_dw(a, 0, 1, st);
  tmark(a, 2, st);
  hipLaunchKernelGGL(k_finalize_ddpg_actor, dim3(1), dim3(kFinThreads), 0, st, (const float*)a->part, p.Bp / 32, B,
                     a->cfg.aout, a->cfg.custom_loss, losses);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

// actor Adam step, then polyak of the critic target (already fused into the critic
// step: the critic does not change afterwards) and of the actor target (ddpg.py:273-284)
sppStatus sppDdpgAcmActorApply(sppAgentHandle a, void* stream) {
  SPP_REQUIRE(a && a->ddpg && a->d_adam.ptr, SPP_E_STATE, "DDPG_AcM agent not ready");
  a->steps[0] += 1;
  tmark(a, 3, S(stream));
  launch_adam(a, 2, 1, a->net[SPP_NET_ACTOR].n, a->steps[0], a->cfg.actor_lr, a->cfg.tau, S(stream));
  tmark(a, 3, S(stream));
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppDdpgAcmUpdate(sppAgentHandle a, const sppBatch* bt, float* losses, void* stream) {
  sppStatus s;
  if ((s = sppDdpgAcmCriticGrads(a, bt, losses, stream))) return s;
  if ((s = sppDdpgAcmCriticApply(a, stream))) return s;
  if ((s = sppDdpgAcmActorGrads(a, losses, stream))) return s;
  return sppDdpgAcmActorApply(a, stream);
}

sppStatus sppAgentStageFromReplay(sppAgentHandle a, sppReplayHandle r, const int64_t* idx, int B, void* stream) {
  SPP_REQUIRE(a && r && idx && B > 0 && B <= a->Bmax, SPP_E_INVALID_ARG, "stage_from_replay: bad args");
  const ReplayDev& d = replay_dev(r);
  SPP_REQUIRE(d.ob == a->cfg.ob && d.ac == a->cfg.ac && d.aout == a->cfg.aout, SPP_E_SHAPE, "dims differ");
  launch_replay_stage(d, idx, B, (int)round_up(B, 32), a->S, a->S2, a->cfg.acm_critic ? nullptr : a->ACT, a->AENV,
                      a->R, a->DN, S(stream));
  SPP_CHECK_HIP(hipGetLastError());
  a->cur_B = B;
  return SPP_OK;
}

sppStatus sppAgentStagePost(sppAgentHandle a, int normalize, int act_from_next_obs, void* stream) {
  SPP_REQUIRE(a && a->cur_B > 0, SPP_E_STATE, "stage_post: no staged batch");
  if (!normalize && !act_from_next_obs) return SPP_OK;
  SPP_REQUIRE(!act_from_next_obs || (!a->cfg.acm_critic && a->cfg.aout == a->cfg.ob && a->ACT), SPP_E_INVALID_ARG,
              "stage_post: action = next_obs needs a critic on (obs, actor output) with aout == ob");
  SPP_REQUIRE(normalize >= 0 && normalize <= 2, SPP_E_INVALID_ARG, "stage_post: normalize %d", normalize);
  const int mm = normalize == 2 ? 0 : a->cfg.min_max_denormalize;  // 2: z-score whatever the agent's mode
  SPP_REQUIRE(!normalize || (mm ? (a->lo && a->hi) : (a->mean && a->std)), SPP_E_STATE,
              "stage_post: normalizer not bound");
  const int B = a->cur_B, Bp = (int)round_up(B, 32), ob = a->cfg.ob;
  hipLaunchKernelGGL(k_stage_post, dim3(cdiv((int64_t)ob * B, 256)), dim3(256), 0, S(stream), a->S, a->S2, a->ACT, ob,
                     B, Bp, a->lo, a->hi, a->mean, a->std, mm, normalize != 0, act_from_next_obs);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppSacAcmUpdateStaged(sppAgentHandle a, uint64_t seed, uint64_t counter, float* losses, void* stream) {
  SPP_REQUIRE(a && a->cur_B > 0, SPP_E_STATE, "no staged batch");
  hipStream_t st = S(stream);
  sppStatus s = sppSacAcmDrawEps(a, seed, counter, stream);
  if (s) return s;
  if ((s = critic_grads_staged(a, losses, st))) return s;
  if ((s = sppSacAcmCriticApply(a, stream))) return s;
  if ((s = actor_grads(a, losses, st))) return s;
  return actor_apply(a, losses, st);
}

sppStatus sppAcmRegressGrads(sppAgentHandle a, const float* x, const float* y, int B, float* loss, void* stream) {
  SPP_REQUIRE(a && x && y && B > 0 && B <= a->Bmax, SPP_E_INVALID_ARG, "acm step: bad args (B=%d, max %d)", B,
              a->Bmax);
  SPP_REQUIRE(!(a->ddpg && a->plain), SPP_E_STATE, "vanilla DDPG has no ACM to regress");
  hipStream_t st = S(stream);
  sppStatus s = check_ready(a);
  if (s) return s;
  if (a->dws[1].B != B) {
    if ((s = build_dw(a, 1, B))) return s;
  }
  launch_pack(a, PJ_ACM, PJ_TARG, st);
  SacArgs p = make_args(a, B);
  if (a->ddpg) {  // BasicAcM: natural-input fc1 / fc21 packings
    p.bacm.W1 = a->bacm_W1n;
    p.bacm.W21 = a->bacm_W21n;
    BAcmRegArgs g{};
    g.B = B; g.Bp = (int)round_up(B, 32); g.x = x; g.y = y;
    g.XT = a->RX; g.H = a->RBH; g.H1 = a->RBH1; g.S21 = a->RS21; g.P1 = a->RBP1; g.PZ = a->RPZ; g.PZ21 = a->RPZ21;
    g.P3 = a->RP3; g.part = a->part;
    tmark(a, 4, st);
    hipLaunchKernelGGL(a->ks.dreg, dim3(phase_grid(a, g.Bp)), dim3(256), 0, st, p, g);
    SPP_CHECK_HIP(hipGetLastError());
    launch_dw(a, 1, 0, st);
    tmark(a, 4, st);
    hipLaunchKernelGGL(k_finalize_bacm, dim3(1), dim3(256), 0, st, (const float*)a->part, g.Bp / 32, kBParts, B,
                       a->cfg.ac, a->net[SPP_NET_ACM].g, loss);
    SPP_CHECK_HIP(hipGetLastError());
    return SPP_OK;
  }
  p.acm.W1 = a->acm_W1n;
  AcmRegArgs g{};
  g.B = B; g.Bp = (int)round_up(B, 32); g.x = x; g.y = y;
  g.XT = a->RX; g.Z1 = a->RZ1; g.Z2 = a->RZ2; g.P1 = a->RP1; g.P2 = a->RP2; g.P3 = a->RP3; g.part = a->part;
  tmark(a, 4, st);
  hipLaunchKernelGGL(a->ks.acmreg, dim3(phase_grid(a, g.Bp)), dim3(256), 0, st, p, g);
  SPP_CHECK_HIP(hipGetLastError());
  launch_dw(a, 1, 0, st);
  tmark(a, 4, st);
  hipLaunchKernelGGL(k_finalize_acm, dim3(1), dim3(256), 0, st, (const float*)a->part, g.Bp / 32, B, a->cfg.ac, loss);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppAcmRegressApply(sppAgentHandle a, void* stream) {
  SPP_REQUIRE(a && a->d_adam.ptr, SPP_E_STATE, "agent not ready");
  SPP_REQUIRE(!(a->ddpg && a->plain), SPP_E_STATE, "vanilla DDPG has no ACM to regress");
  a->steps[3] += 1;
  launch_adam(a, 3, 1, a->net[SPP_NET_ACM].n, a->steps[3], a->cfg.acm_lr, 0.f, S(stream));
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

// waves per workgroup of the multi-workgroup AcM regression kernel (HEAD 0, bs > 64).  8 = two waves per SIMD,
// up to 128 rows per workgroup, at least 2 workgroups (its LDS has no room for the single-workgroup form's
// canonical gradient staging).  Measured round 5 (1049-row PPO ACM steps, profiles/r05/ab_acm_wv.txt): 8 waves
// on 9 workgroups 17.3 us per step against 13.4 us for 4 waves on 17: the MFMA work per CU doubles while the
// second wave per SIMD hides less than that, so the default stays 4 (A/B: -DSPP_ACM_WV=8; 2 waves on 33
// workgroups measured 17.0 us too).  bs <= 64 always runs
// the single-workgroup 4-wave form.
#ifndef SPP_ACM_WV
#define SPP_ACM_WV 4
#endif
constexpr int kAcmWV = SPP_ACM_WV, kAcmR = 16 * kAcmWV;
// Passes of kAcmR rows per workgroup and step (sppSetAcmSgdPasses; 0: one): P passes put a step on
// ceil(bs / (P kAcmR)) workgroups (k_mlp_sgd's MP form).
static int g_acm_passes = 0;
static int acm_passes(int bs) {
  const int P = std::max(1, g_acm_passes);
  return bs <= kMlR || cdiv(bs, kAcmR) < 2 * P ? 1 : P;  // (>= 2 workgroups after the split)
}
static int acm_sgd_nwg(int bs) { return bs <= kMlR ? 1 : std::max(2, cdiv(bs, kAcmR * acm_passes(bs))); }
static int acm_sgd_max_wg(sppAgentHandle a, int ob, int ac) {
  if (a->sgd_max_wg >= 0) return a->sgd_max_wg;
  int n = 0;
  if (ob == 11 && ac == 3) n = mlp_sgd_max_wg<22, 32, 3, 0, kAcmWV>(a->num_cu);
  else if (ob == 17 && ac == 6) n = mlp_sgd_max_wg<34, 32, 6, 0, kAcmWV>(a->num_cu);
  else if (ob == 3 && ac == 1) n = mlp_sgd_max_wg<6, 32, 1, 0, kAcmWV>(a->num_cu);
  a->sgd_max_wg = n;
  return n;
}

int sppAcmSgdWorkgroups(sppAgentHandle a, int bs) { return (a && !a->ddpg && bs > 0) ? acm_sgd_nwg(bs) : 0; }

sppStatus sppSetAcmSgdPasses(int passes) {
  SPP_REQUIRE(passes >= 0 && passes <= 16, SPP_E_INVALID_ARG, "acm passes %d", passes);
  g_acm_passes = passes;
  return SPP_OK;
}

int sppAcmSgdMaxBatch(sppAgentHandle a) {
  if (!a || a->ddpg) return 0;
  return kAcmR * std::max(1, g_acm_passes) * std::max(1, acm_sgd_max_wg(a, a->cfg.ob, a->cfg.ac));
}

sppStatus sppAcmSgdStatusAsync(sppAgentHandle a, int* timed_out_pinned, void* stream) {
  SPP_REQUIRE(a && timed_out_pinned, SPP_E_INVALID_ARG, "acm_sgd_status_async: null");
  if (a->sgd_sync.ptr)
    SPP_CHECK_HIP(hipMemcpyAsync(timed_out_pinned, a->sgd_sync.ptr + 1, sizeof(int), hipMemcpyDeviceToHost, S(stream)));
  else
    *timed_out_pinned = 0;
  return SPP_OK;
}

// nsteps sequential steps: bs rows each, the last one bs_last (<= bs) rows
static sppStatus acm_sgd_run(sppAgentHandle a, const float* x, const float* y, int nsteps, int bs, int bs_last,
                             float* loss_sum, void* stream) {
  SPP_REQUIRE(a && x && y && loss_sum && nsteps >= 0 && bs > 0 && bs_last > 0 && bs_last <= bs, SPP_E_INVALID_ARG,
              "acm_sgd: bad args");
  SPP_REQUIRE(!a->ddpg, SPP_E_INVALID_ARG, "acm_sgd: the persistent kernel is for the AcM (SAC_AcM / PPO_AcM handles)");
  SPP_REQUIRE(bs <= kAcmR * kMlMaxWG, SPP_E_SHAPE, "acm_sgd: batch %d > %d", bs, kAcmR * kMlMaxWG);
  sppStatus s = check_ready(a);
  if (s) return s;
  if (nsteps == 0) return SPP_OK;
  const NetBufs& n = a->net[SPP_NET_ACM];
  SPP_REQUIRE(n.p && n.m && n.v, SPP_E_STATE, "acm_sgd: ACM buffers not bound");
  MlpSgdArgs g{};
  g.x = x; g.y = y; g.nsteps = nsteps; g.bs = bs; g.bsl = bs; g.bs_last = bs_last;
  g.params = n.p; g.m = n.m; g.v = n.v; g.lr = a->cfg.acm_lr; g.step0 = a->steps[3];
  g.lim = a->limits.ptr + a->cfg.aout; g.loss_sum = loss_sum; g.spin = g_sgd_spin;
  const int ob = a->cfg.ob, ac = a->cfg.ac;
  hipStream_t st = S(stream);
  // <= kAcmR rows per workgroup (sgd_mlp.hip); the per-step arrival barriers need every workgroup resident at once
  const int nwg = acm_sgd_nwg(bs);
  SPP_REQUIRE(nwg <= acm_sgd_max_wg(a, ob, ac), SPP_E_SHAPE, "acm_sgd: batch %d needs %d co-resident workgroups > %d",
              bs, nwg, acm_sgd_max_wg(a, ob, ac));
  if (nwg > 1) {
    g.bsl = cdiv(bs, nwg);
    s = mlp_sgd_buffers(a->sgd_slab, a->sgd_sync, st);
    if (s) return s;
    g.slab = a->sgd_slab.ptr;
    g.pbuf = a->sgd_slab.ptr + (size_t)2 * kMlMaxWG * kMlSlabMax;
    g.ctr = sgd_ctr(a->sgd_sync);
    g.err = a->sgd_sync.ptr + 1;
  }
  const bool mw = nwg > 1, mp = mw && g.bsl > kAcmR;
#define SPP_SGD_LAUNCH(IN_, AC_)                                                                              \
  if (mp) hipLaunchKernelGGL((k_mlp_sgd<IN_, 32, AC_, 0, true, kAcmWV, true>), dim3(nwg), dim3(64 * kAcmWV), 0, st, g); \
  else if (mw) hipLaunchKernelGGL((k_mlp_sgd<IN_, 32, AC_, 0, true, kAcmWV>), dim3(nwg), dim3(64 * kAcmWV), 0, st, g); \
  else hipLaunchKernelGGL((k_mlp_sgd<IN_, 32, AC_, 0, false>), dim3(1), dim3(kMlTH), 0, st, g)
  if (ob == 11 && ac == 3) SPP_SGD_LAUNCH(22, 3);
  else if (ob == 17 && ac == 6) SPP_SGD_LAUNCH(34, 6);
  else if (ob == 3 && ac == 1) SPP_SGD_LAUNCH(6, 1);
  else SPP_REQUIRE(false, SPP_E_SHAPE, "acm_sgd: no instantiation for ob=%d ac=%d", ob, ac);
#undef SPP_SGD_LAUNCH
  a->steps[3] += nsteps;
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppAcmSgd(sppAgentHandle a, const float* x, const float* y, int nsteps, int bs, float* loss_sum,
                    void* stream) {
  return acm_sgd_run(a, x, y, nsteps, bs, bs, loss_sum, stream);
}

sppStatus sppAcmSgdEpoch(sppAgentHandle a, const float* x, const float* y, int nrows, int bs, float* loss_sum,
                         void* stream) {
  SPP_REQUIRE(nrows >= 0 && bs > 0, SPP_E_INVALID_ARG, "acm_sgd_epoch: bad args");
  if (nrows == 0) return SPP_OK;
  const int nsteps = cdiv(nrows, bs);
  return acm_sgd_run(a, x, y, nsteps, bs, nrows - (nsteps - 1) * bs, loss_sum, stream);
}

sppStatus sppAcmSgdStatus(sppAgentHandle a, int* timed_out) {
  SPP_REQUIRE(a && timed_out, SPP_E_INVALID_ARG, "acm_sgd_status: null");
  *timed_out = 0;
  if (a->sgd_sync.ptr) SPP_CHECK_HIP(hipMemcpy(timed_out, a->sgd_sync.ptr + 1, sizeof(int), hipMemcpyDeviceToHost));
  return SPP_OK;
}

sppStatus sppAcmRegressStep(sppAgentHandle a, const float* x, const float* y, int B, float* loss, void* stream) {
  sppStatus s = sppAcmRegressGrads(a, x, y, B, loss, stream);
  if (s) return s;
  return sppAcmRegressApply(a, stream);
}

sppStatus sppPolicyAct(sppAgentHandle a, const float* obs, int E, const float* eps, const float* noise,
                       float act_noise, int mode, int denorm_out, float* target_out, float* env_out, void* stream) {
  SPP_REQUIRE(a && obs && E > 0 && target_out && env_out, SPP_E_INVALID_ARG, "policy_act: bad args");
  SPP_REQUIRE(mode >= 0 && mode <= 3, SPP_E_INVALID_ARG, "mode");
  SPP_REQUIRE((mode != 0 && mode != 3) || eps, SPP_E_INVALID_ARG, "modes 0 / 3 need eps");
  SPP_REQUIRE(mode != 3 || !a->ddpg, SPP_E_INVALID_ARG, "mode 3 (caller action) is a SAC_AcM-handle (AcM) mode");
  hipStream_t st = S(stream);
  sppStatus s = check_ready(a);
  if (s) return s;
  launch_pack(a, PJ_ACTOR, PJ_TARG, st);
  SacArgs p = make_args(a, 32);
  ActArgs g{E, mode, denorm_out, act_noise, obs, eps, noise, target_out, env_out, a->plain ? 1 : 0};
  const int grid = std::max(1, std::min(cdiv(cdiv(E, 32), kWavesPerWG), a->num_cu));
  if (a->ddpg && a->plain && a->ks.dact_team && a->team_ok && cdiv(E, 32) <= a->num_cu)  // one tile per CU
    hipLaunchKernelGGL(a->ks.dact_team, dim3(cdiv(E, 32)), dim3(64 * kTeamDAct), 0, st, p, g, a->bz);
  else if (a->ddpg)
    hipLaunchKernelGGL(a->ks.dact, dim3(grid), dim3(256), 0, st, p, g, a->bz);
  else if (a->plain && a->ks.act_team && a->team_ok && cdiv(E, 32) <= a->num_cu)  // one tile per CU (sac_team.h)
    hipLaunchKernelGGL(a->ks.act_team, dim3(cdiv(E, 32)), dim3(64 * kTeamCritic), 0, st, p, g);
  else
    hipLaunchKernelGGL(a->ks.act, dim3(grid), dim3(256), 0, st, p, g);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppDebugDense(const float* x, const float* W, const float* b, float* y, int B, int K, int N, int act,
                        void* stream) {
  SPP_REQUIRE(x && W && y && B > 0 && K > 0 && K <= 256 && N > 0 && N <= 256, SPP_E_INVALID_ARG, "debug dense: bad");
  SPP_REQUIRE(K <= 224 || K == 256, SPP_E_INVALID_ARG, "debug dense: K in (224, 256) not supported");
  hipStream_t st = S(stream);
  const int NBI = blocks_of(K), NBO = blocks_of(N);
  const int ibm = NBI == 8 ? 1 : 0;
  float4* wf;
  PackJob* dj;
  SPP_CHECK_HIP(hipMalloc(&wf, sizeof(float4) * NBO * NBI * 256));
  SPP_CHECK_HIP(hipMalloc(&dj, sizeof(PackJob)));
  PackJob pj{W, nullptr, 1 << 30, K, 0, 0, nat(N), nat(K), NBO, NBI, ibm, wf};
  SPP_CHECK_HIP(hipMemcpy(dj, &pj, sizeof(pj), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_pack_matrix, dim3(16, 1), dim3(256), 0, st, (const PackJob*)dj);
  const dim3 grid(cdiv(B, 32));
  const int kq = regs_valid(K, 0) / 4;  // quads of block 0 that carry units
  if (NBI == 1 && kq < 4) {
    switch (kq) {
#define SPP_DD(n) case n: hipLaunchKernelGGL((k_debug_dense<1, 1, n>), grid, dim3(64), 0, st, (const float4*)wf, b, x, y, B, K, N, act); break;
      SPP_DD(1) SPP_DD(2) SPP_DD(3)
#undef SPP_DD
    }
  } else if (NBI < 8) {
    switch (NBI) {
#define SPP_DD(n) case n: hipLaunchKernelGGL((k_debug_dense<n, 1>), grid, dim3(64), 0, st, (const float4*)wf, b, x, y, B, K, N, act); break;
      SPP_DD(1) SPP_DD(2) SPP_DD(3) SPP_DD(4) SPP_DD(5) SPP_DD(6) SPP_DD(7)
#undef SPP_DD
    }
  } else {
    switch (NBO) {
#define SPP_DD(n) case n: hipLaunchKernelGGL((k_debug_dense<8, n>), grid, dim3(64), 0, st, (const float4*)wf, b, x, y, B, K, N, act); break;
      SPP_DD(1) SPP_DD(2) SPP_DD(3) SPP_DD(4) SPP_DD(5) SPP_DD(6) SPP_DD(7) SPP_DD(8)
#undef SPP_DD
    }
  }
  SPP_CHECK_HIP(hipGetLastError());
  SPP_CHECK_HIP(hipStreamSynchronize(st));
  hipFree(wf); hipFree(dj);
  return SPP_OK;
}

// One phase of weight-gradient jobs through dw_job, finalize_dw and launch_dw_set: what the agents run (spprl.h).
sppStatus sppDebugDwSet(sppDwJobDesc* descs, int njobs, int B, int num_cu, int big_waves, void* stream) {
  SPP_REQUIRE(descs && njobs > 0 && njobs <= 64 && B > 0 && B <= (1 << 30) && num_cu > 0 && num_cu <= 4096 &&
                  (big_waves == 4 || big_waves == 8),
              SPP_E_INVALID_ARG, "debug dw: njobs %d B %d num_cu %d big_waves %d", njobs, B, num_cu, big_waves);
  const int Bp = (int)round_up(B, 32);
  auto al16 = [](const void* p) { return ((size_t)p & 15) == 0; };
  std::vector<DwJob> jobs;
  for (int i = 0; i < njobs; ++i) {
    const sppDwJobDesc& d = descs[i];
    SPP_REQUIRE(d.N > 0 && d.N <= 256 && d.K0 > 0 && d.K1 >= 0 && d.K0 + d.K1 <= 256, SPP_E_INVALID_ARG,
                "debug dw: job %d N %d K0 %d K1 %d", i, d.N, d.K0, d.K1);
    SPP_REQUIRE(d.nrow2 >= 1 && d.nrow2 <= d.N && d.dW && (d.nrow2 == d.N || (d.dW2 && (!d.db || d.db2))),
                SPP_E_INVALID_ARG, "debug dw: job %d nrow2 %d of %d rows, or an output is null", i, d.nrow2, d.N);
    SPP_REQUIRE((d.bf16 != 0) == (descs[0].bf16 != 0) && (d.bf16 || (!d.a_bf && !d.x_bf)), SPP_E_INVALID_ARG,
                "debug dw: job %d bf16 %d a_bf %d x_bf %d (job 0: bf16 %d)", i, d.bf16, d.a_bf, d.x_bf, descs[0].bf16);
    if (d.fused)
      SPP_REQUIRE(d.nsplit >= 2 && d.nsplit <= (1 << 20) && d.slabs, SPP_E_INVALID_ARG,
                  "debug dw: fused job %d nsplit %d, or slabs null", i, d.nsplit);
    else
      SPP_REQUIRE(d.A && d.X0 && (d.K1 == 0 || d.X1) && al16(d.A) && al16(d.X0) && al16(d.X1), SPP_E_INVALID_ARG,
                  "debug dw: job %d operand null or not 16-byte aligned", i);
    DwJob& j = dw_job(jobs, Bp, (const float*)d.A, d.N, (const float*)d.X0, d.K0, (const float*)d.X1, d.K1, d.dW, d.db,
                      d.nrow2, d.dW2, d.db2);
    j.bf16 = d.bf16 ? 1 : 0;
    j.a_bf = d.a_bf ? 1 : 0;
    j.x_bf = d.x_bf ? 1 : 0;
    if (d.fused) {
      j.fused = 1;
      j.nsplit = d.nsplit;
      j.wsplit = 1;
    }
  }
  hipStream_t st = S(stream);
  DwSet D;
  struct Release {
    DwSet& D;
    ~Release() { D.release(); }
  } release{D};
  D.j0[0] = 0;
  D.nj[0] = njobs;
  D.big_waves = big_waves;
  D.thin_min_bp = dw_thin_min_bp();
  const sppStatus s = finalize_dw(D, jobs, 1, Bp, B, num_cu);
  if (s) return s;
  {  // which jobs' items run in k_dw_thin: the table's last nthin items
    std::vector<int> it(D.nitems[0]);  // item_job
    SPP_CHECK_HIP(hipMemcpy(it.data(), D.items.ptr + D.ioff[0], sizeof(int) * it.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < njobs; ++i) descs[i].thin = 0;
    for (int k = D.nitems[0] - D.nthin[0]; k < D.nitems[0]; ++k) descs[it[k]].thin = 1;
  }
  if (D.slab.n) SPP_CHECK_HIP(hipMemsetAsync(D.slab.ptr, 0xff, sizeof(float) * D.slab.n, st));  // NaN
  for (int i = 0; i < njobs; ++i) {
    descs[i].split_len = jobs[i].split_len;
    descs[i].wsplit = jobs[i].wsplit;
    if (!jobs[i].fused) descs[i].nsplit = jobs[i].nsplit;
    else
      SPP_CHECK_HIP(hipMemcpyAsync(jobs[i].slab, descs[i].slabs, sizeof(float) * jobs[i].nsplit * jobs[i].slab_stride,
                                   hipMemcpyDeviceToDevice, st));
  }
  launch_dw_set(D, 0, st);
  SPP_CHECK_HIP(hipGetLastError());
  SPP_CHECK_HIP(hipStreamSynchronize(st));
  return SPP_OK;
}

// In-place average of one exchange bucket over the communicator (ncclSum, then x 1/world: the same
// arithmetic as spprl.dp.make_allreduce), stream-ordered between *Grads and *Apply.  The bucket's buffers are
// listed here; the exchange itself is api_comm.hip's (comm_allreduce_mean).
sppStatus sppAllReduceGrads(sppAgentHandle h, int bucket, int world, void* rccl_comm, void* stream) {
  SPP_REQUIRE(h && rccl_comm && world > 0 && bucket >= SPP_BUCKET_CRITIC && bucket <= SPP_BUCKET_ALL,
              SPP_E_INVALID_ARG, "allreduce grads: bucket %d world %d", bucket, world);
  SPP_REQUIRE(comm_loaded(), SPP_E_RCCL, "librccl.so.1 not loadable");
  std::vector<std::pair<float*, int64_t>> bufs;
  auto add = [&](int net) {
    if (h->net[net].g && h->lay[net].size() > 0) bufs.push_back({h->net[net].g, h->lay[net].size()});
  };
  const bool all = bucket == SPP_BUCKET_ALL;
  if (all || bucket == SPP_BUCKET_CRITIC) {
    add(SPP_NET_CRITIC1);
    if (!h->ddpg) add(SPP_NET_CRITIC2);
  }
  if (all || bucket == SPP_BUCKET_ACTOR) {
    add(SPP_NET_ACTOR);
    if (!h->ddpg) bufs.push_back({h->alpha_grad, 1});
  }
  if ((all || bucket == SPP_BUCKET_ACM) && !h->plain) add(SPP_NET_ACM);
  SPP_REQUIRE(!bufs.empty(), SPP_E_STATE, "allreduce grads: no gradient buffer bound for bucket %d", bucket);
  return comm_allreduce_mean(bufs, world, rccl_comm, S(stream));
}

}  // extern "C"

extern "C" sppStatus sppDebugReadProf(unsigned long long* out64, int reset) {
#ifdef SPP_PROF
  SPP_REQUIRE(out64, SPP_E_INVALID_ARG, "null");
  SPP_CHECK_HIP(hipDeviceSynchronize());
  SPP_CHECK_HIP(hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_tprof), sizeof(unsigned long long) * 64));
  if (reset) {
    unsigned long long z[64] = {};
    SPP_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_tprof), z, sizeof(z)));
  }
  return SPP_OK;
#else
  (void)out64;
  (void)reset;
  set_error("region profiling is only compiled into profiling builds (build.py --prof)");
  return SPP_E_STATE;
#endif
}

#ifdef SPP_SINGLE_TU  // (the profiling build is one translation unit: g_tprof, mlp.h)
#include "api_comm.hip"
#include "api_onp.hip"
#include "api_replay.hip"
#endif
