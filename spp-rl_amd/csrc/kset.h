// Kernel-set table: dims -> phase-kernel instantiations.  Each config family is
// instantiated in its own translation unit (ks_*.hip) so the library builds in
// parallel; api.hip, the agent's unit and the only api unit to include this, only holds the function pointers.
#pragma once
#include "sac.hip"
#include "sac_bf.h"
#include "ddpg.hip"
#include "sac_team.h"
#include "ddpg_team.h"

namespace spp {

struct KernelSet {
  void (*critic)(SacArgs);
  void (*actor)(SacArgs, AcmScratch);
  void (*actor_heads)(SacArgs, AcmScratch);  // wide heads: second kernel of the actor phase
  void (*act)(SacArgs, ActArgs);
  void (*acmreg)(SacArgs, AcmRegArgs);
  // DDPG_AcM
  void (*dcritic)(SacArgs, BAcmScratch);
  void (*dactor)(SacArgs, BAcmScratch);
  void (*dact)(SacArgs, ActArgs, BAcmScratch);
  void (*dreg)(SacArgs, BAcmRegArgs);
  // small-batch (team) forms of the SAC phases: one 4-wave workgroup per 32-sample tile (sac_team.h);
  // null where the shapes have none
  void (*critic_team)(SacArgs);
  void (*actor_team)(SacArgs, AcmScratch);
  void (*act_team)(SacArgs, ActArgs);  // plain handles' rollout action
  // small-batch (team) forms of the DDPG phases and rollout action (ddpg_team.h): vanilla DDPG handles
  void (*dcritic_team)(SacArgs, BAcmScratch);
  void (*dactor_team)(SacArgs, BAcmScratch);
  void (*dact_team)(SacArgs, ActArgs, BAcmScratch);
  // min-critic split of the one-wave SAC actor phase (fp32 sets; sac.hip): forward to q = min(Q1, Q2), the
  // chosen critics' backward over the regrouped samples, and everything behind it; null where there is none
  void (*actor_fwd)(SacArgs, AcmScratch);
  void (*actor_minq)(SacArgs, AcmScratch);
  void (*actor_bwd)(SacArgs, AcmScratch);
  // stage split of actor_bwd (narrow heads; sac.hip): the per-sample stages as a high-occupancy kernel, then the
  // trunk backward; null where there is none
  void (*heads_stage)(SacArgs, AcmScratch);
  void (*trunk_bwd)(SacArgs, AcmScratch);
  // stage split of actor_fwd and of the critic phase: trunk, squash + ACM forward, the rest
  void (*trunk_fwd_a)(SacArgs, AcmScratch);
  void (*squash_a)(SacArgs, AcmScratch);
  void (*critics_a)(SacArgs, AcmScratch);
  void (*trunk_fwd_c)(SacArgs, AcmScratch);
  void (*squash_c)(SacArgs, AcmScratch);
  void (*critic_rest)(SacArgs);
  // wave-pair forms of critics_a and critic_rest (sac.hip): a tile's two critics on two waves
  void (*critics_a_pair)(SacArgs, AcmScratch);
  void (*critic_rest_pair)(SacArgs);
  // register hand-over forms of the three trunk kernels (sac.hip: Fc1Gen / WhTGen under the 256-wide layer; SPP_ACTOR_GEN);
  // null where the set compiles none (Cfg::GEN_AFC1 / GEN_AWHT)
  void (*trunk_fwd_a_gen)(SacArgs, AcmScratch);
  void (*trunk_fwd_c_gen)(SacArgs, AcmScratch);
  void (*trunk_bwd_gen)(SacArgs, AcmScratch);
};

template <int OB, int AOUT, int AC, bool ACMC, bool BF = false>
KernelSet make_kset() {
  using C = Cfg<OB, AOUT, AC, ACMC, BF>;
  void (*heads)(SacArgs, AcmScratch) = nullptr;
  if constexpr (C::NB_PAIR > 2) heads = k_sac_actor_heads<C>;
  void (*critic)(SacArgs) = k_sac_critic_phase<C>;
#if SPP_BF16_TWO_TILES
  if constexpr (C::BF && C::ACMC && !C::F3) critic = k_sac_critic_phase2<C>;  // two tiles per wave (sac_bf.h)
#endif
  KernelSet ks{critic, k_sac_actor_phase<C>, heads, k_policy_act<C>, k_acm_regress<C>,
               nullptr, nullptr, nullptr, nullptr};
  if constexpr (!C::BF) {
    ks.actor_fwd = k_sac_actor_phase<C, true>;
    ks.actor_minq = k_sac_minq_backward<C>;
    ks.actor_bwd = k_sac_actor_heads<C, true>;
    if constexpr (C::NB_PAIR <= 2) {
      ks.heads_stage = k_sac_heads_stage<C>;
      ks.trunk_bwd = k_sac_actor_trunk_bwd<C>;
      ks.trunk_fwd_a = k_sac_trunk_fwd<C, true>;
      ks.squash_a = k_sac_squash_stage<C, true>;
      ks.critics_a = k_sac_actor_phase<C, true, true>;
      ks.trunk_fwd_c = k_sac_trunk_fwd<C, false>;
      ks.squash_c = k_sac_squash_stage<C, false>;
      ks.critic_rest = k_sac_critic_phase<C, true>;
      ks.critics_a_pair = k_sac_actor_phase<C, true, true, true>;
      ks.critic_rest_pair = k_sac_critic_phase<C, true, true>;
      if constexpr (C::GEN_AFC1) {
        ks.trunk_fwd_a_gen = k_sac_trunk_fwd_gen<C, true>;
        ks.trunk_fwd_c_gen = k_sac_trunk_fwd_gen<C, false>;
      }
      if constexpr (C::GEN_AWHT) ks.trunk_bwd_gen = k_sac_actor_trunk_bwd_gen<C>;
    }
  }
  return ks;
}
template <int OB, int AOUT, int AC, bool ACMC>
KernelSet make_dkset() {
  using D = DCfg<OB, AOUT, AC, ACMC>;
  return {nullptr, nullptr, nullptr, nullptr, nullptr,
          k_ddpg_critic_phase<D>, k_ddpg_actor_phase<D>, k_ddpg_policy_act<D>, k_bacm_regress<D>};
}

#define SPP_KSET_CASE(mk, o, a, c)                                     \
  if (ob == o && aout == a && ac == c) {                               \
    *ks = acmc ? mk<o, a, c, true>() : mk<o, a, c, false>();           \
    return true;                                                       \
  }

bool kset_sac_hopper(int ob, int aout, int ac, bool acmc, KernelSet* ks);    // ks_sac_hopper.hip
bool kset_sac_hcheetah(int ob, int aout, int ac, bool acmc, KernelSet* ks);  // ks_sac_hcheetah.hip
bool kset_sac_ant(int ob, int aout, int ac, bool acmc, KernelSet* ks);       // ks_sac_ant.hip
bool kset_sac_small(int ob, int aout, int ac, bool acmc, KernelSet* ks);     // ks_sac_small.hip
bool kset_ddpg(int ob, int aout, int ac, bool acmc, KernelSet* ks);          // ks_ddpg.hip
bool kset_ddpg_ant(int ob, int aout, int ac, bool acmc, KernelSet* ks);      // ks_ddpg_ant.hip
bool kset_sac_bf16(int ob, int aout, int ac, bool acmc, KernelSet* ks);      // ks_sac_bf16.hip
bool kset_sac_vanilla(int ob, int aout, int ac, bool acmc, KernelSet* ks);   // ks_sac_vanilla.hip
bool kset_ddpg_vanilla(int ob, int aout, int ac, bool acmc, KernelSet* ks);  // ks_ddpg_vanilla.hip

}  // namespace spp
