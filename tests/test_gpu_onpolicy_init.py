"""An on-policy agent's own seeded initial state, bit for bit, against a CPU re-draw: the on-policy twin of
test_gpu_agent_init.py.

The four classes share their constructor's front half (OnPolicyLoop._init_loop) and build their nets after it, so a
base that drew, or a class that built its nets in another order, would shift every parameter and no fixture test --
they all LOAD parameters -- would notice.  Expected values come from spprl.nets alone: one
``torch.Generator().manual_seed(SEED)`` through ``nets.linear_init_``, the actor first (``log_scale`` filled with
-1.34, basic_model.py:18-20, then its layout without ``log_scale``), the critic after it.  The AcM classes' ACM net
is the one a SAC_AcM draws at that seed (test_gpu_agent_init's order table).

Per class: both parameter vectors; the loop's state (n_envs, T, the zeroed episode accounting, no observation yet);
the key order of ``collect_params_dict()`` (rl.py:263-279, + "acm"); the KL counter.  Construction only.

Shapes: Hopper-v2 is (11, 3), the smallest the on-policy kernels are instantiated at; batch_size 10 over 4 envs
takes the ceiling in T = ceil(10 / 4) = 3.
"""
import pytest
import torch

import spprl
from spprl import _lib, nets
from spprl.onpolicy import actor_layout, critic_layout
from test_gpu_agent_init import CASES, NORM_KEYS, SEED

pytestmark = pytest.mark.gpu

OB, AC = 11, 3
# class: (actor output dim, extra keywords, checkpoint keys, kl_div_updates_counter)
ONPOLICY = {
    "PPO": (AC, {}, ["actor", "critic"] + NORM_KEYS, 0),
    "A2C": (AC, {}, ["actor", "critic"] + NORM_KEYS, None),
    "PPO_AcM": (OB, dict(acm_pre_train_samples=64), ["actor", "critic"] + NORM_KEYS + ["acm"], 0),
    "A2C_AcM": (OB, dict(acm_pre_train_samples=64), ["actor", "critic"] + NORM_KEYS + ["acm"], None),
}


@pytest.mark.parametrize("name", sorted(ONPOLICY))
def test_seeded_initial_state(name):
    aout, kw, keys, kl = ONPOLICY[name]
    ag = getattr(spprl, name)(env_name="Hopper-v2", n_envs=4, batch_size=10, seed=SEED, loop_seed=3, device="cuda:0",
                              **kw)
    gen = torch.Generator().manual_seed(SEED)
    a_lay, c_lay = actor_layout(OB, aout), critic_layout(OB)
    actor = torch.empty(nets.numel(a_lay))
    actor[:aout].fill_(-1.34)
    nets.linear_init_(actor[aout:], a_lay[1:], gen)
    critic = nets.linear_init_(torch.empty(nets.numel(c_lay)), c_lay, gen)
    assert ag.nets.layouts == [a_lay, c_lay]
    assert torch.equal(ag.nets.params[0].cpu(), actor)
    assert torch.equal(ag.nets.params[1].cpu(), critic)
    if "acm" in keys:
        gen = torch.Generator().manual_seed(SEED)
        drawn = {net: nets.linear_init_(torch.empty(nets.numel(lay)), lay, gen) for net, lay in CASES["SAC_AcM"][1]}
        assert torch.equal(ag.acm.params[_lib.SPP_NET_ACM].cpu(), drawn[_lib.SPP_NET_ACM])
    assert ag.n_envs == 4 and ag.T == 3
    assert ag._ep_ret.shape == (4,) and ag._ep_ret.dtype == torch.float32 and not ag._ep_ret.any()
    assert ag._ret_sums.shape == (2,) and ag._ret_sums.dtype == torch.float64 and not ag._ret_sums.any()
    assert ag._obs is None
    assert ag.iteration == 0
    assert list(ag.collect_params_dict()) == keys
    assert ag.kl_div_updates_counter == kl and (kl is None) == (ag.kl_div_updates_counter is None)
