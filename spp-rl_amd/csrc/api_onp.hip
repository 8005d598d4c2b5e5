// libspprl C-ABI, the on-policy unit: the on-policy handle (A2C / PPO nets) with its persistent epoch / critic
// launches, and the free-standing on-policy stream utilities (GAE, clip loss, advantage norms).  Compiles ppo.hip, the
// onp*.hip kernels and the PPO actor / critic (HEAD 1 / 2) instantiations of k_mlp_sgd; the off-policy agent is api.hip's.
#include <algorithm>
#include <memory>
#include <vector>

#include "host.h"
#include "replay.h"

#include "ppo.hip"
#include "onp.hip"
#include "onp_a2c.hip"
#include "onp_rollout.hip"

using namespace spp;

// ================================================================== on-policy (A2C / PPO) nets
namespace spp {
struct OnpKernels {
  void (*value)(OnpArgs);
  void (*critic)(OnpArgs);
  void (*actor)(OnpArgs);
  void (*act)(OnpArgs);
  void (*rollout)(OnpRolloutArgs);
  void (*td_adv)(OnpA2cArgs);  // (null: no A2C instantiation for these dims)
  void (*pg_actor)(OnpA2cArgs);
};
template <int OB, int AOUT>
OnpKernels make_onp() {
  using C = OCfg<OB, AOUT>;
  OnpKernels k{k_onp_value<C>, k_onp_critic_grad<C>, k_onp_actor_grad<C>, k_onp_act<C>, k_onp_rollout_act<OB, AOUT>,
               nullptr, nullptr};
  if constexpr (OB != 3) {  // A2C / A2C_AcM: the HalfCheetah and Hopper pairs
    k.td_adv = k_onp_td_adv<C>;
    k.pg_actor = k_onp_pg_actor_grad<C>;
  }
  return k;
}
static bool find_onp(int ob, int aout, OnpKernels* k) {
  if (ob == 17 && aout == 17) { *k = make_onp<17, 17>(); return true; }  // SPP-PPO HalfCheetah
  if (ob == 11 && aout == 11) { *k = make_onp<11, 11>(); return true; }  // Hopper
  if (ob == 17 && aout == 6) { *k = make_onp<17, 6>(); return true; }    // vanilla PPO HalfCheetah
  if (ob == 11 && aout == 3) { *k = make_onp<11, 3>(); return true; }    // vanilla PPO Hopper
  if (ob == 3 && aout == 1) { *k = make_onp<3, 1>(); return true; }      // Pendulum (tests)
  return false;
}
}  // namespace spp

struct sppOnPolicy {
  sppOnPolicyConfig cfg{};
  int device = 0, num_cu = 256;
  OnpKernels ks{};
  NetBufs net[2];  // 0 actor, 1 critic
  NetLayout lay[2];
  int64_t steps[2] = {0, 0};
  DevArray<float> lim;
  DevArray<float4> pk;
  DevArray<PackJob> d_pj;
  int o_pj[3] = {};  // pack jobs in d_pj: the actor's [o_pj[0], o_pj[1]), the critic's [o_pj[1], o_pj[2])
  OnpNet actor{}, critic{};
  std::vector<TabSeg> tab;
  DevArray<float> scratch;
  float *XT = nullptr, *H1 = nullptr, *H2 = nullptr, *D1 = nullptr, *D2 = nullptr, *D3 = nullptr, *part = nullptr;
  int Bpmax = 0, pstride = 0;
  DwSet dw[2];  // 0 critic, 1 actor
  DevArray<AdamJob> d_adam;
  // persistent PPO actor epochs (sppOnpActorEpoch, sgd_mlp.hip HEAD 1): slabs + parameter buffer, {counter, flag}
  DevArray<float> sgd_slab;
  DevArray<int> sgd_sync;
  int sgd_max_wg = -1;
  int crit_max_wg = -1;  // co-resident persistent-critic workgroups (onp_critic_max_wg, cached)
  int wg_reserve = 0;    // CUs left to a persistent launch on another stream (sppOnpReserveWorkgroups)
};

static sppStatus onp_packs(sppOnPolicy* o) {
  const int ob = o->cfg.ob, aout = o->cfg.aout;
  SPP_REQUIRE(o->net[0].p && o->net[1].p, SPP_E_STATE, "on-policy nets not bound");
  PackPlan pp;
  {  // actor (list 0): log_scale, fc1, fc2, fc3
    const float* P = o->net[0].p;
    const NetLayout& L = o->lay[0];
    const float *W1 = P + L.w(0), *W2 = P + L.w(1), *W3 = P + L.w(2);
    pp.M(0, W1, nullptr, 1 << 30, ob, 0, 0, nat(64), nat(ob), 2, blocks_of(ob), &o->actor.W1);
    pp.M(0, W2, nullptr, 1 << 30, 64, 0, 0, nat(64), nat(64), 2, 2, &o->actor.W2);
    pp.M(0, W3, nullptr, 1 << 30, 64, 0, 0, nat(aout), nat(64), blocks_of(aout), 2, &o->actor.W3);
    pp.M(0, W3, nullptr, 1 << 30, 64, 1, 0, nat(64), nat(aout), 2, blocks_of(aout), &o->actor.W3T);
    pp.M(0, W2, nullptr, 1 << 30, 64, 1, 0, nat(64), nat(64), 2, 2, &o->actor.W2T);
    o->actor.tb1 = pp.T(P + L.b(0), 64);
    o->actor.tb2 = pp.T(P + L.b(1), 64);
    o->actor.tb3 = pp.T(P + L.b(2), aout);
  }
  {  // critic (list 1): fc1, fc2, fc3
    const float* P = o->net[1].p;
    const NetLayout& L = o->lay[1];
    const float *W1 = P + L.w(0), *W2 = P + L.w(1);
    pp.M(1, W1, nullptr, 1 << 30, ob, 0, 0, nat(64), nat(ob), 2, blocks_of(ob), &o->critic.W1);
    pp.M(1, W2, nullptr, 1 << 30, 64, 0, 0, nat(64), nat(64), 2, 2, &o->critic.W2);
    pp.M(1, W2, nullptr, 1 << 30, 64, 1, 0, nat(64), nat(64), 2, 2, &o->critic.W2T);
    o->critic.tb1 = pp.T(P + L.b(0), 64);
    o->critic.tb2 = pp.T(P + L.b(1), 64);
    o->critic.tb3 = pp.T(P + L.w(2), 64);
    o->critic.b3 = P + L.b(2);
  }
  o->tab = pp.tab;
  SPP_REQUIRE(pp.toff <= 1024 && o->tab.size() <= 8, SPP_E_SHAPE, "on-policy LDS table too large");
  std::vector<PackJob> jobs;
  sppStatus s = pp.commit(2, o->pk, o->d_pj, jobs, o->o_pj);
  if (s) return s;
  AdamJob aj[2] = {AdamJob{o->net[0].p, o->net[0].g, o->net[0].m, o->net[0].v, nullptr, o->net[0].n},
                   AdamJob{o->net[1].p, o->net[1].g, o->net[1].m, o->net[1].v, nullptr, o->net[1].n}};
  if (!o->d_adam.ptr) SPP_CHECK_HIP(o->d_adam.alloc(2));
  SPP_CHECK_HIP(hipMemcpy(o->d_adam.ptr, aj, sizeof(aj), hipMemcpyHostToDevice));
  o->dw[0].B = o->dw[1].B = -1;
  return SPP_OK;
}

// job set 0: the critic's (net 1), 1: the actor's (net 0); fc1 (delta1 x x), fc2 (delta2 x h1), fc3 (delta3 x h2)
static sppStatus onp_dw(sppOnPolicy* o, int which, int N) {
  const int Bp = (int)round_up(N, 32), net = which == 0 ? 1 : 0;
  std::vector<DwJob> jobs;
  float* G = o->net[net].g;
  const NetLayout& L = o->lay[net];
  layer_dw(jobs, Bp, G, L, 0, o->D1, o->XT);
  layer_dw(jobs, Bp, G, L, 1, o->D2, o->H1);
  layer_dw(jobs, Bp, G, L, 2, o->D3, o->H2);
  DwSet& D = o->dw[which];
  D.j0[0] = 0;
  D.nj[0] = (int)jobs.size();
  return finalize_dw(D, jobs, 1, Bp, N, o->num_cu);
}

static OnpArgs onp_args(sppOnPolicy* o, int N) {
  OnpArgs p{};
  p.N = N;
  p.Np = (int)round_up(N, 32);
  p.actor = o->actor;
  p.critic = o->critic;
  p.log_scale = o->net[0].p;
  p.lim = o->lim.ptr;
  p.eps_clip = o->cfg.ppo_epsilon;
  p.XT = o->XT; p.H1 = o->H1; p.H2 = o->H2; p.D1 = o->D1; p.D2 = o->D2; p.D3 = o->D3;
  p.part = o->part;
  p.pstride = o->pstride;
  p.nseg = (int)o->tab.size();
  for (int i = 0; i < p.nseg; ++i) p.seg[i] = o->tab[i];
  return p;
}

// net 0: repack the actor's weight images (the params may have changed since the last call), 1: the
// critic's; the other network's images are not touched.
static sppStatus onp_ready(sppOnPolicy* o, int N, hipStream_t st, int net) {
  SPP_REQUIRE(N > 0 && N <= o->cfg.max_batch, SPP_E_SHAPE, "batch %d outside (0, max_batch=%d]", N, o->cfg.max_batch);
  SPP_REQUIRE(o->lim.ptr, SPP_E_STATE, "actor limits not set");
  if (!o->pk.ptr) {
    sppStatus s = onp_packs(o);
    if (s) return s;
  }
  const PackJob* pj = (const PackJob*)o->d_pj.ptr + o->o_pj[net];
  launch_pack_matrix(16, o->o_pj[net + 1] - o->o_pj[net], pj, st);
  return SPP_OK;
}

static int onp_grid(sppOnPolicy* o, int N) {
  return std::max(1, std::min(cdiv(cdiv(N, 32), 4), o->num_cu * 2));
}

extern "C" {

sppStatus sppOnpCreate(sppOnPolicyHandle* out, const sppOnPolicyConfig* cfg, int device) {
  SPP_REQUIRE(out && cfg && cfg->max_batch > 0, SPP_E_INVALID_ARG, "on-policy create: bad args");
  OnpKernels k;
  SPP_REQUIRE(find_onp(cfg->ob, cfg->aout, &k), SPP_E_SHAPE, "no on-policy instantiation for (ob=%d, aout=%d)", cfg->ob,
              cfg->aout);
  SPP_CHECK_HIP(hipSetDevice(device));
  auto o = std::make_unique<sppOnPolicy>();
  o->cfg = *cfg;
  o->device = device;
  o->ks = k;
  hipDeviceProp_t prop;
  SPP_CHECK_HIP(hipGetDeviceProperties(&prop, device));
  o->num_cu = prop.multiProcessorCount;
  o->lay[0] = onp_actor_layout(cfg->ob, cfg->aout);
  o->lay[1] = onp_critic_layout(cfg->ob);
  const int64_t Bp = round_up(cfg->max_batch, 32);
  o->Bpmax = (int)Bp;
  o->pstride = (int)round_up(3 + cfg->aout, 4);
  const int64_t rows = cfg->ob + 64 + 64 + 64 + 64 + std::max(cfg->aout, 1);
  const int64_t total = rows * Bp + (Bp / 32) * o->pstride + 64;
  hipError_t e = o->scratch.alloc(total);
  if (e != hipSuccess) {
    set_error("on-policy scratch alloc: %s", hipGetErrorString(e));
    return SPP_E_OOM;
  }
  SPP_CHECK_HIP(hipMemset(o->scratch.ptr, 0, sizeof(float) * total));
  float* b = o->scratch.ptr;
  o->XT = b; b += cfg->ob * Bp;
  o->H1 = b; b += 64 * Bp;
  o->H2 = b; b += 64 * Bp;
  o->D1 = b; b += 64 * Bp;
  o->D2 = b; b += 64 * Bp;
  o->D3 = b; b += std::max(cfg->aout, 1) * Bp;
  o->part = b;
  *out = o.release();
  return SPP_OK;
}

sppStatus sppOnpDestroy(sppOnPolicyHandle o) {
  if (!o) return SPP_OK;
  hipSetDevice(o->device);
  hipDeviceSynchronize();
  o->lim.release(); o->pk.release(); o->d_pj.release(); o->scratch.release(); o->d_adam.release();
  o->sgd_slab.release(); o->sgd_sync.release();
  for (auto& D : o->dw) D.release();
  delete o;
  return SPP_OK;
}

sppStatus sppOnpNetSize(sppOnPolicyHandle o, int net, int64_t* n) {
  SPP_REQUIRE(o && n && (net == 0 || net == 1), SPP_E_INVALID_ARG, "bad net id");
  *n = o->lay[net].size();
  return SPP_OK;
}

sppStatus sppOnpBindNet(sppOnPolicyHandle o, int net, float* p, float* g, float* m, float* v) {
  SPP_REQUIRE(o && (net == 0 || net == 1) && p && g && m && v, SPP_E_INVALID_ARG, "on-policy bind: bad args");
  o->net[net] = NetBufs{p, g, m, v, o->lay[net].size()};
  o->pk.release();
  return SPP_OK;
}

sppStatus sppOnpSetLimits(sppOnPolicyHandle o, const float* lim_host) {
  SPP_REQUIRE(o && lim_host, SPP_E_INVALID_ARG, "null");
  if (!o->lim.ptr) SPP_CHECK_HIP(o->lim.alloc(o->cfg.aout));
  SPP_CHECK_HIP(hipMemcpy(o->lim.ptr, lim_host, sizeof(float) * o->cfg.aout, hipMemcpyHostToDevice));
  return SPP_OK;
}

sppStatus sppOnpValue(sppOnPolicyHandle o, const float* x, int N, float* v, void* stream) {
  SPP_REQUIRE(o && x && v, SPP_E_INVALID_ARG, "value: null");
  hipStream_t st = S(stream);
  sppStatus s = onp_ready(o, N, st, 1);
  if (s) return s;
  OnpArgs p = onp_args(o, N);
  p.X = x;
  p.V = v;
  hipLaunchKernelGGL(o->ks.value, dim3(onp_grid(o, N)), dim3(256), 0, st, p);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppOnpCriticGrads(sppOnPolicyHandle o, const float* x, const float* q, int N, float* loss, void* stream) {
  SPP_REQUIRE(o && x && q, SPP_E_INVALID_ARG, "critic grads: null");
  hipStream_t st = S(stream);
  sppStatus s = onp_ready(o, N, st, 1);
  if (s) return s;
  if (o->dw[0].B != N && (s = onp_dw(o, 0, N))) return s;
  OnpArgs p = onp_args(o, N);
  p.X = x;
  p.Q = q;
  hipLaunchKernelGGL(o->ks.critic, dim3(onp_grid(o, N)), dim3(256), 0, st, p);
  SPP_CHECK_HIP(hipGetLastError());
  launch_dw_set(o->dw[0], 0, st);
  hipLaunchKernelGGL(k_onp_finish_critic, dim3(1), dim3(256), 0, st, (const float*)o->part, p.Np / 32, o->pstride, N,
                     loss);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppOnpCriticApply(sppOnPolicyHandle o, void* stream) {
  SPP_REQUIRE(o && o->d_adam.ptr, SPP_E_STATE, "on-policy handle not ready");
  o->steps[1] += 1;
  const double bc1 = 1.0 - std::pow(0.9, (double)o->steps[1]), bc2s = std::sqrt(1.0 - std::pow(0.999, (double)o->steps[1]));
  launch_adam_kernel((const AdamJob*)(o->d_adam.ptr + 1), o->net[1].n, (float)(-(o->cfg.critic_lr / bc1)),
                     (float)bc2s, S(stream));
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppOnpActorGrads(sppOnPolicyHandle o, const float* x, const float* act, const float* lp_old,
                           const float* adv, const float* next_obs, int N, float* out4, void* stream) {
  SPP_REQUIRE(o && x && act && lp_old && adv && out4, SPP_E_INVALID_ARG, "actor grads: null");
  hipStream_t st = S(stream);
  sppStatus s = onp_ready(o, N, st, 0);
  if (s) return s;
  if (o->dw[1].B != N && (s = onp_dw(o, 1, N))) return s;
  OnpArgs p = onp_args(o, N);
  p.X = x; p.ACT = act; p.LP_OLD = lp_old; p.ADV = adv; p.NXT = next_obs;
  hipLaunchKernelGGL(o->ks.actor, dim3(onp_grid(o, N)), dim3(256), 0, st, p);
  SPP_CHECK_HIP(hipGetLastError());
  launch_dw_set(o->dw[1], 0, st);
  hipLaunchKernelGGL(k_onp_finish_actor, dim3(1), dim3(256), 0, st, (const float*)o->part, p.Np / 32, o->pstride, N,
                     o->cfg.aout, o->cfg.entropy_coef, (const float*)o->net[0].p, o->net[0].g, out4);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppOnpActorApply(sppOnPolicyHandle o, void* stream) {
  SPP_REQUIRE(o && o->d_adam.ptr, SPP_E_STATE, "on-policy handle not ready");
  o->steps[0] += 1;
  const double bc1 = 1.0 - std::pow(0.9, (double)o->steps[0]), bc2s = std::sqrt(1.0 - std::pow(0.999, (double)o->steps[0]));
  launch_adam_kernel((const AdamJob*)o->d_adam.ptr, o->net[0].n, (float)(-(o->cfg.actor_lr / bc1)), (float)bc2s,
                     S(stream));
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppOnpTdAdvantage(sppOnPolicyHandle o, const float* x, const float* x_next, const float* rew,
                            const float* done, int N, float gamma, float* q_out, float* adv_out, float* moments2,
                            void* stream) {
  SPP_REQUIRE(o && x && x_next && rew && done && adv_out, SPP_E_INVALID_ARG, "td advantage: null");
  SPP_REQUIRE(o->ks.td_adv, SPP_E_SHAPE, "no A2C instantiation for (ob=%d, aout=%d)", o->cfg.ob, o->cfg.aout);
  hipStream_t st = S(stream);
  sppStatus s = onp_ready(o, N, st, 1);
  if (s) return s;
  OnpA2cArgs a{};
  a.o = onp_args(o, N);
  a.o.X = x;
  a.XN = x_next; a.REW = rew; a.DONE = done; a.gamma = gamma; a.Q_OUT = q_out; a.ADV_OUT = adv_out;
  hipLaunchKernelGGL(o->ks.td_adv, dim3(onp_grid(o, N)), dim3(256), 0, st, a);
  SPP_CHECK_HIP(hipGetLastError());
  if (moments2) {
    hipLaunchKernelGGL(k_onp_td_moments, dim3(1), dim3(256), 0, st, (const float*)o->part, a.o.Np / 32, o->pstride, N,
                       moments2);
    SPP_CHECK_HIP(hipGetLastError());
  }
  return SPP_OK;
}

sppStatus sppOnpPgActorGrads(sppOnPolicyHandle o, const float* x, const float* act, const float* adv,
                             const float* moments2, const float* dist_act, const float* next_obs, int N, float* out4,
                             void* stream) {
  SPP_REQUIRE(o && x && act && adv && out4, SPP_E_INVALID_ARG, "pg actor grads: null");
  SPP_REQUIRE(o->ks.pg_actor, SPP_E_SHAPE, "no A2C instantiation for (ob=%d, aout=%d)", o->cfg.ob, o->cfg.aout);
  hipStream_t st = S(stream);
  sppStatus s = onp_ready(o, N, st, 0);
  if (s) return s;
  if (o->dw[1].B != N && (s = onp_dw(o, 1, N))) return s;
  OnpA2cArgs a{};
  a.o = onp_args(o, N);
  a.o.X = x; a.o.ACT = act; a.o.ADV = adv; a.o.NXT = next_obs;
  a.MOM = moments2; a.DIST_ACT = dist_act;
  hipLaunchKernelGGL(o->ks.pg_actor, dim3(onp_grid(o, N)), dim3(256), 0, st, a);
  SPP_CHECK_HIP(hipGetLastError());
  launch_dw_set(o->dw[1], 0, st);
  hipLaunchKernelGGL(k_onp_finish_actor, dim3(1), dim3(256), 0, st, (const float*)o->part, a.o.Np / 32, o->pstride, N,
                     o->cfg.aout, 0.f, (const float*)o->net[0].p, o->net[0].g, out4);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

// co-resident workgroups of the multi-workgroup PPO actor epoch kernel (0: no instantiation for these dims)
static int onp_epoch_max_wg(sppOnPolicy* o) {
  if (o->sgd_max_wg >= 0) return o->sgd_max_wg;
  const int ob = o->cfg.ob, aout = o->cfg.aout;
  int n = 0;
  if (ob == 17 && aout == 17) n = mlp_sgd_max_wg<17, 64, 17, 1>(o->num_cu);
  else if (ob == 11 && aout == 11) n = mlp_sgd_max_wg<11, 64, 11, 1>(o->num_cu);
  else if (ob == 17 && aout == 6) n = mlp_sgd_max_wg<17, 64, 6, 1>(o->num_cu);  // vanilla PPO: aout = ac
  else if (ob == 11 && aout == 3) n = mlp_sgd_max_wg<11, 64, 3, 1>(o->num_cu);
  o->sgd_max_wg = n;
  return n;
}

// slots of a kernel with `full` co-resident workgroups on the device that the reserved CUs take away: each
// reserved CU held a whole workgroup of the concurrent launch (k_mlp_sgd's LDS, > 80 KB for every
// instantiation, fits one per CU), so it removes this kernel's per-CU occupancy, not one slot
static int onp_reserved_slots(sppOnPolicy* o, int full) {
  return o->wg_reserve * std::max(1, cdiv(full, std::max(1, o->num_cu)));
}

int sppOnpActorEpochMaxBatch(sppOnPolicyHandle o) {
  if (!o) return 0;
  const int n = onp_epoch_max_wg(o) - onp_reserved_slots(o, onp_epoch_max_wg(o));
  return n > 0 ? kMlR * n : 0;
}

sppStatus sppOnpActorEpoch(sppOnPolicyHandle o, const float* x, const float* act, const float* lp_old, const float* adv,
                           const float* next_obs, const int64_t* idx, int nrows, int bs, float* out4, void* stream) {
  SPP_REQUIRE(o && x && act && lp_old && adv && idx && out4 && nrows >= 0 && bs > 0, SPP_E_INVALID_ARG,
              "actor epoch: bad args");
  const int nsteps = cdiv(nrows, bs);
  SPP_REQUIRE(o->net[0].p && o->net[0].m && o->net[0].v && o->lim.ptr, SPP_E_STATE, "actor epoch: actor not bound");
  const int nwg = cdiv(bs, kMlR), maxwg = onp_epoch_max_wg(o) - onp_reserved_slots(o, onp_epoch_max_wg(o));
  SPP_REQUIRE(maxwg > 0, SPP_E_SHAPE, "actor epoch: no instantiation for ob=%d aout=%d", o->cfg.ob, o->cfg.aout);
  SPP_REQUIRE(nwg <= maxwg, SPP_E_SHAPE, "actor epoch: batch %d needs %d co-resident workgroups > %d", bs, nwg, maxwg);
  if (nsteps == 0) return SPP_OK;
  hipStream_t st = S(stream);
  MlpSgdArgs g{};
  g.x = x; g.y = act; g.nxt = next_obs ? next_obs : act; g.lp_old = lp_old; g.adv = adv; g.idx = idx;
  g.nsteps = nsteps; g.bs = bs; g.bsl = bs; g.bs_last = nrows - (nsteps - 1) * bs;
  const NetBufs& n = o->net[0];
  g.params = n.p; g.m = n.m; g.v = n.v; g.lr = o->cfg.actor_lr; g.step0 = o->steps[0];
  g.lim = o->lim.ptr; g.eps_clip = o->cfg.ppo_epsilon; g.ent_coef = o->cfg.entropy_coef; g.out = out4;
  g.spin = g_sgd_spin;
  if (nwg > 1) {
    g.bsl = cdiv(bs, nwg);
    sppStatus s = mlp_sgd_buffers(o->sgd_slab, o->sgd_sync, st);
    if (s) return s;
    g.slab = o->sgd_slab.ptr;
    g.pbuf = o->sgd_slab.ptr + (size_t)2 * kMlMaxWG * kMlSlabMax;
    g.ctr = sgd_ctr(o->sgd_sync);
    g.err = o->sgd_sync.ptr + 1;
  }
  const bool mw = nwg > 1;
#define SPP_EPOCH_LAUNCH(OB_, OUT_)                                                                     \
  if (mw) hipLaunchKernelGGL((k_mlp_sgd<OB_, 64, OUT_, 1, true>), dim3(nwg), dim3(kMlTH), 0, st, g);     \
  else hipLaunchKernelGGL((k_mlp_sgd<OB_, 64, OUT_, 1, false>), dim3(1), dim3(kMlTH), 0, st, g)
  // (maxwg > 0 above: one of onp_epoch_max_wg's four pairs)
  if (o->cfg.ob == 17 && o->cfg.aout == 17) SPP_EPOCH_LAUNCH(17, 17);
  else if (o->cfg.ob == 11 && o->cfg.aout == 11) SPP_EPOCH_LAUNCH(11, 11);
  else if (o->cfg.ob == 17) SPP_EPOCH_LAUNCH(17, 6);
  else SPP_EPOCH_LAUNCH(11, 3);
#undef SPP_EPOCH_LAUNCH
  o->steps[0] += nsteps;
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

// persistent critic steps (HEAD 2): co-resident workgroups, passes of 64 rows per workgroup and step
constexpr int kCriticMaxPasses = 64;  // (the data-parallel PPO union batch: world x 32,768 rows)
// slots the critic grid always leaves free (a concurrent ACM grid of up to 64 workgroups: PPO_AcM), so that
// its row partition -- and with it the gradient's summation order -- is the same with or without one
constexpr int kCriticSideSlots = 64;

static int onp_critic_max_wg(sppOnPolicy* o) {
  if (o->crit_max_wg >= 0) return o->crit_max_wg;
  const int ob = o->cfg.ob;
  int n = 0;
  if (ob == 17) n = mlp_sgd_max_wg<17, 64, 1, 2>(o->num_cu);
  else if (ob == 11) n = mlp_sgd_max_wg<11, 64, 1, 2>(o->num_cu);
  o->crit_max_wg = n;
  return n;
}

static int onp_critic_budget(sppOnPolicy* o) {
  const int full = onp_critic_max_wg(o);
  const int res = onp_reserved_slots(o, full);
  return std::max(0, full > kCriticSideSlots ? full - std::max(res, kCriticSideSlots) : full - res);
}

int sppOnpCriticStepsMaxBatch(sppOnPolicyHandle o) {
  if (!o) return 0;
  const int b = onp_critic_budget(o);
  // one workgroup takes one 64-row pass per step (its single-workgroup form has no passes): batches of more
  // than one tile need >= 2 co-resident workgroups
  return b >= 2 ? kMlR * kCriticMaxPasses * b : (b == 1 ? kMlR : 0);
}

sppStatus sppOnpReserveWorkgroups(sppOnPolicyHandle o, int n) {
  SPP_REQUIRE(o && n >= 0, SPP_E_INVALID_ARG, "reserve workgroups: bad args");
  o->wg_reserve = n;
  return SPP_OK;
}

sppStatus sppOnpCriticSteps(sppOnPolicyHandle o, const float* x, const float* q, int N, int nsteps, float* loss_sum,
                            void* stream) {
  SPP_REQUIRE(o && x && q && loss_sum && N > 0 && nsteps >= 0, SPP_E_INVALID_ARG, "critic steps: bad args");
  SPP_REQUIRE(o->net[1].p && o->net[1].m && o->net[1].v && o->lim.ptr, SPP_E_STATE, "critic steps: critic not bound");
  const int maxwg = onp_critic_budget(o);
  SPP_REQUIRE(maxwg > 0, SPP_E_SHAPE, "critic steps: no instantiation for ob=%d (or every slot reserved)", o->cfg.ob);
  // fewest passes per workgroup the co-resident grid allows, then the fewest workgroups for that many passes;
  // more than one tile always runs the multi-workgroup form (G >= 2: the single-workgroup kernel makes one
  // 64-row pass per step)
  const int tiles = cdiv(N, kMlR);
  SPP_REQUIRE(tiles == 1 || maxwg >= 2, SPP_E_SHAPE, "critic steps: batch %d needs >= 2 co-resident workgroups", N);
  const int passes = tiles == 1 ? 1 : cdiv(tiles, maxwg), nwg = tiles == 1 ? 1 : std::max(2, cdiv(tiles, passes));
  SPP_REQUIRE(passes <= kCriticMaxPasses, SPP_E_SHAPE, "critic steps: batch %d > %d", N, kMlR * kCriticMaxPasses * maxwg);
  if (nsteps == 0) return SPP_OK;
  hipStream_t st = S(stream);
  MlpSgdArgs g{};
  g.x = x; g.y = q; g.nsteps = nsteps; g.bs = N; g.bsl = N; g.bs_last = N;
  const NetBufs& n = o->net[1];
  g.params = n.p; g.m = n.m; g.v = n.v; g.lr = o->cfg.critic_lr; g.step0 = o->steps[1];
  g.lim = o->lim.ptr; g.loss_sum = loss_sum; g.spin = g_sgd_spin;
  if (nwg > 1) {
    g.bsl = cdiv(N, nwg);
    sppStatus s = mlp_sgd_buffers(o->sgd_slab, o->sgd_sync, st);
    if (s) return s;
    g.slab = o->sgd_slab.ptr;
    g.pbuf = o->sgd_slab.ptr + (size_t)2 * kMlMaxWG * kMlSlabMax;
    g.ctr = sgd_ctr(o->sgd_sync);
    g.err = o->sgd_sync.ptr + 1;
  }
  const bool mw = nwg > 1;
#define SPP_CRITIC_LAUNCH(OB_)                                                                        \
  if (mw) hipLaunchKernelGGL((k_mlp_sgd<OB_, 64, 1, 2, true>), dim3(nwg), dim3(kMlTH), 0, st, g);     \
  else hipLaunchKernelGGL((k_mlp_sgd<OB_, 64, 1, 2, false>), dim3(1), dim3(kMlTH), 0, st, g)
  if (o->cfg.ob == 17) SPP_CRITIC_LAUNCH(17);
  else SPP_CRITIC_LAUNCH(11);
#undef SPP_CRITIC_LAUNCH
  o->steps[1] += nsteps;
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppOnpSyncStatusAsync(sppOnPolicyHandle o, int* timed_out_pinned, void* stream) {
  SPP_REQUIRE(o && timed_out_pinned, SPP_E_INVALID_ARG, "onp sync status async: null");
  if (o->sgd_sync.ptr)
    SPP_CHECK_HIP(hipMemcpyAsync(timed_out_pinned, o->sgd_sync.ptr + 1, sizeof(int), hipMemcpyDeviceToHost, S(stream)));
  else
    *timed_out_pinned = 0;
  return SPP_OK;
}

sppStatus sppSetSgdSpinLimit(int polls) {
  g_sgd_spin = polls;  // < 0: every wait gives up at once (sgd_arrive_wait_wt)
  return SPP_OK;
}

sppStatus sppOnpActorEpochStatus(sppOnPolicyHandle o, int* timed_out) {
  SPP_REQUIRE(o && timed_out, SPP_E_INVALID_ARG, "actor epoch status: null");
  *timed_out = 0;
  if (o->sgd_sync.ptr) SPP_CHECK_HIP(hipMemcpy(timed_out, o->sgd_sync.ptr + 1, sizeof(int), hipMemcpyDeviceToHost));
  return SPP_OK;
}

sppStatus sppOnpAct(sppOnPolicyHandle o, const float* x, int N, const float* eps, float* act_out, float* logp_out,
                    void* stream) {
  SPP_REQUIRE(o && x && act_out, SPP_E_INVALID_ARG, "act: null");
  hipStream_t st = S(stream);
  sppStatus s = onp_ready(o, N, st, 0);
  if (s) return s;
  OnpArgs p = onp_args(o, N);
  p.X = x; p.EPS = eps; p.ACT_OUT = act_out; p.LP_OUT = logp_out;
  hipLaunchKernelGGL(o->ks.act, dim3(onp_grid(o, N)), dim3(256), 0, st, p);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppOnpRolloutAct(sppOnPolicyHandle o, const float* obs, int E, const float* mean, const float* std,
                           uint64_t seed, uint64_t offset, int deterministic, float* act_out, float* logp_out,
                           float* norm_obs_out, float* noise_out, void* stream) {
  SPP_REQUIRE(o && obs && act_out && E > 0, SPP_E_INVALID_ARG, "rollout act: bad args");
  SPP_REQUIRE((mean == nullptr) == (std == nullptr), SPP_E_INVALID_ARG, "rollout act: mean and std, or neither");
  SPP_REQUIRE(o->net[0].p && o->lim.ptr, SPP_E_STATE, "rollout act: actor not bound / limits not set");
  OnpRolloutArgs p{};
  p.obs = obs; p.mean = mean; p.std = std; p.P = o->net[0].p; p.lim = o->lim.ptr;
  p.seed = seed; p.offset = offset; p.E = E; p.deterministic = deterministic;
  p.act = act_out; p.lp = logp_out; p.xn = norm_obs_out; p.noise = noise_out;
  hipLaunchKernelGGL(o->ks.rollout, dim3(E), dim3(64), 0, S(stream), p);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppOnpObsStats(const float* start_obs, int64_t n_start, const float* next_obs, int64_t n_next,
                         const float* obs, int64_t n_obs, int ob, double alpha, float* mean, float* std,
                         float* max_obs, float* min_obs, int have_minmax, void* stream) {
  SPP_REQUIRE(ob > 0 && n_start >= 0 && n_next >= 0 && n_obs >= 0 && (start_obs || n_start == 0) &&
                  (next_obs || n_next == 0) && (obs || n_obs == 0),
              SPP_E_INVALID_ARG, "obs stats: bad rows");
  SPP_REQUIRE(mean && std && max_obs && min_obs && alpha >= 0.0 && alpha <= 1.0, SPP_E_INVALID_ARG,
              "obs stats: null statistics or alpha outside [0, 1]");
  if (n_start + n_next == 0 && n_obs == 0) return SPP_OK;
  OnpStatsArgs a{};
  a.start = start_obs; a.next = next_obs; a.obs = obs;
  a.n_start = n_start; a.n_next = n_next; a.n_obs = n_obs;
  a.ob = ob; a.have_minmax = have_minmax; a.alpha = alpha;
  a.mean = mean; a.std = std; a.max_obs = max_obs; a.min_obs = min_obs;
  hipLaunchKernelGGL(k_onp_obs_stats, dim3(ob), dim3(256), 0, S(stream), a);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

// ---------------------------------------------------------------- stream utilities (ppo.hip)
sppStatus sppGaeScan(const float* rew, const float* v, const float* v_next, const uint8_t* done,
                     const uint8_t* end, int64_t T, int64_t E, double gamma, double lam, int mode, float* q_out,
                     float* adv, void* stream) {
  SPP_REQUIRE(T >= 0 && E > 0 && mode >= -1 && mode <= 1, SPP_E_INVALID_ARG, "gae: T=%lld E=%lld mode=%d",
              (long long)T, (long long)E, mode);
  if (T == 0) return SPP_OK;
  SPP_REQUIRE(rew && v && v_next && done && end && adv, SPP_E_INVALID_ARG, "gae: null input");
  if (mode < 0) mode = E >= 64 ? 0 : 1;
  const double disc = lam * gamma;  // python floats: discount = gae_lambda * gamma (ppo.py:136)
  if (mode == 0)
    hipLaunchKernelGGL(k_gae_seq, dim3(cdiv(E, 256)), dim3(256), 0, S(stream), rew, v, v_next, done, end, T, E,
                       (float)gamma, disc, q_out, adv);
  else
    hipLaunchKernelGGL(k_gae_scan, dim3(E), dim3(kScanThreads), 0, S(stream), rew, v, v_next, done, end, T, E,
                       (float)gamma, (float)disc, q_out, adv);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppPpoClipLoss(const float* lp_old, const float* lp_new, const float* adv, int B, float eps, float* grad,
                         float* out2, void* stream) {
  SPP_REQUIRE(lp_old && lp_new && adv && out2 && B > 0, SPP_E_INVALID_ARG, "clip loss: bad args");
  const int nblk = cdiv(B, 256);
  double* part = nullptr;
  SPP_CHECK_HIP(hipMallocAsync((void**)&part, sizeof(double) * 2 * nblk, S(stream)));
  hipLaunchKernelGGL(k_ppo_clip, dim3(nblk), dim3(256), 0, S(stream), lp_old, lp_new, adv, B, eps, grad, part);
  hipLaunchKernelGGL(k_ppo_clip_finish, dim3(1), dim3(256), 0, S(stream), (const double*)part, nblk, B, out2);
  SPP_CHECK_HIP(hipFreeAsync(part, S(stream)));
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppAdvNormalize(const float* adv, int64_t n, float* out, void* stream) {
  SPP_REQUIRE(adv && out && n > 0, SPP_E_INVALID_ARG, "adv normalize: bad args");
  const int nblk = (int)std::min<int64_t>(cdiv(n, 256), 1024);
  double* part = nullptr;
  SPP_CHECK_HIP(hipMallocAsync((void**)&part, sizeof(double) * 2 * nblk, S(stream)));
  hipLaunchKernelGGL(k_adv_moments, dim3(nblk), dim3(256), 0, S(stream), adv, n, part);
  hipLaunchKernelGGL(k_adv_norm, dim3(nblk), dim3(256), 0, S(stream), adv, n, (const double*)part, nblk, out);
  SPP_CHECK_HIP(hipFreeAsync(part, S(stream)));
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppAdvSums(const float* adv, int64_t n, double* sums2, void* stream) {
  SPP_REQUIRE(adv && sums2 && n >= 0, SPP_E_INVALID_ARG, "adv sums: bad args");
  if (n == 0) {
    SPP_CHECK_HIP(hipMemsetAsync(sums2, 0, sizeof(double) * 2, S(stream)));
    return SPP_OK;
  }
  const int nblk = (int)std::min<int64_t>(cdiv(n, 256), 1024);
  double* part = nullptr;
  SPP_CHECK_HIP(hipMallocAsync((void**)&part, sizeof(double) * 2 * nblk, S(stream)));
  hipLaunchKernelGGL(k_adv_moments, dim3(nblk), dim3(256), 0, S(stream), adv, n, part);
  hipLaunchKernelGGL(k_adv_sum2, dim3(1), dim3(64), 0, S(stream), (const double*)part, nblk, sums2);
  SPP_CHECK_HIP(hipFreeAsync(part, S(stream)));
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppAdvNormalizeGlobal(const float* adv, int64_t n_local, const double* sums2, int64_t n_global, float* out,
                                void* stream) {
  SPP_REQUIRE(adv && out && sums2 && n_local >= 0 && n_global > 0, SPP_E_INVALID_ARG, "adv normalize dp: bad args");
  if (n_local == 0) return SPP_OK;
  hipLaunchKernelGGL(k_adv_norm_g, dim3((int)std::min<int64_t>(cdiv(n_local, 256), 1024)), dim3(256), 0, S(stream),
                     adv, n_local, sums2, n_global, out);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

}  // extern "C"
