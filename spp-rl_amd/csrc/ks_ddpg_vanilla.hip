// Vanilla DDPG phase kernels (rltoolkit/algorithms/ddpg/ddpg.py, train/vanilla_ddpg_hcheetah.py):
// HalfCheetah-v2 / Walker2d-v2, the actor emits the 6-dim env action, one critic on cat(obs, action).
#ifndef SPP_SINGLE_TU
#define SPP_KSET_TU
#endif
#include "kset.h"

namespace spp {
bool kset_ddpg_vanilla(int ob, int aout, int ac, bool acmc, KernelSet* ks) {
  if (acmc || aout != ac) return false;
  if (ob == 17 && ac == 6) {
    *ks = make_dkset<17, 6, 6, false>();
    using D = DCfg<17, 6, 6, false>;
    ks->dreg = nullptr;  // no BasicAcM on these handles
    ks->dcritic_team = k_ddpg_critic_team<D>;
    ks->dactor_team = k_ddpg_actor_team<D>;
    ks->dact_team = k_ddpg_policy_act_team<D>;
    return true;
  }
  return false;
}
}  // namespace spp
