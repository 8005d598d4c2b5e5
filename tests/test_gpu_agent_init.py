"""An off-policy agent's own seeded initial state, bit for bit, against a CPU re-draw.

tests/edge_cases.py and tests/bf16_cases.py re-draw parameters "in the library's network order" and LOAD them, so
nothing else would notice a constructor that permuted its draws.  Here the expected values come from spprl.nets alone:
one ``torch.Generator().manual_seed(seed)`` through ``nets.linear_init_`` over the layouts in the order written
below (the targets are drawn too, then overwritten by their sources; skipping them would shift every later net).

Per class: every ``params[net]``; target == source; ``grads`` / ``exp_avg`` / ``exp_avg_sq`` exist for exactly the
trainable nets and are zero; the gradient buckets alias the gradients the way the data-parallel exchange reads them;
the key order of ``collect_params_dict()`` (the reference's: sac.py:287-296, ddpg.py:331-339 + the AcM classes'
"acm").  Construction only: no kernel is launched.

Shapes: ``env_spec=(11, 3, 1.0, 1000)`` for SAC_AcM and DDPG_AcM.  The library instantiates the vanilla algorithms'
kernel sets at (17, 6) alone (csrc/ks_sac_vanilla.hip, ks_ddpg_vanilla.hip), and sppAgentCreate refuses any other
shape, so SAC and DDPG run at ``(17, 6, 1.0, 1000)``: the same assertions on larger nets.
"""
import pytest
import torch

import spprl
from spprl import _lib, nets

pytestmark = pytest.mark.gpu

ACM_SHAPE, VANILLA_SHAPE = (11, 3), (17, 6)
SEED = 20
A, A_T, C1, C2, C1_T, C2_T, ACM = (_lib.SPP_NET_ACTOR, _lib.SPP_NET_ACTOR_TARG, _lib.SPP_NET_CRITIC1,
                                   _lib.SPP_NET_CRITIC2, _lib.SPP_NET_CRITIC1_TARG, _lib.SPP_NET_CRITIC2_TARG,
                                   _lib.SPP_NET_ACM)
NORM_KEYS = ["obs_mean", "obs_std", "min_obs", "max_obs"]


def _sac(shape, aout, acm):
    ob, ac = shape
    cin = ob + aout
    return [(A, nets.sac_actor_layout(ob, aout)), (C1, nets.critic_layout(cin)), (C2, nets.critic_layout(cin)),
            (C1_T, nets.critic_layout(cin)), (C2_T, nets.critic_layout(cin)), (ACM, acm(2 * ob, ac))]


def _ddpg(shape, aout, acm):
    ob, ac = shape
    cin = ob + aout
    order = [(A, nets.ddpg_actor_layout(ob, aout)), (A_T, nets.ddpg_actor_layout(ob, aout)),
             (C1, nets.critic_layout(cin)), (C1_T, nets.critic_layout(cin))]
    return order + ([(ACM, acm(2 * ob, ac))] if acm else [])


# class: (env shape, draw order with layouts, trainable nets, target -> source, checkpoint keys); the AcM actors
# emit an observation (aout = ob), the vanilla ones the env action (aout = ac)
CASES = {
    "SAC_AcM": (ACM_SHAPE, _sac(ACM_SHAPE, ACM_SHAPE[0], nets.acm_layout), {C1, C2, A, ACM}, {C1_T: C1, C2_T: C2},
                ["actor", "critic_1", "critic_2"] + NORM_KEYS + ["acm"]),
    "SAC": (VANILLA_SHAPE, _sac(VANILLA_SHAPE, VANILLA_SHAPE[1], nets.acm_layout), {C1, C2, A, ACM},
            {C1_T: C1, C2_T: C2}, ["actor", "critic_1", "critic_2"] + NORM_KEYS),
    "DDPG_AcM": (ACM_SHAPE, _ddpg(ACM_SHAPE, ACM_SHAPE[0], nets.basic_acm_layout), {C1, A, ACM},
                 {C1_T: C1, A_T: A}, ["actor", "critic"] + NORM_KEYS + ["acm"]),
    "DDPG": (VANILLA_SHAPE, _ddpg(VANILLA_SHAPE, VANILLA_SHAPE[1], None), {C1, A}, {C1_T: C1, A_T: A},
             ["actor", "critic"] + NORM_KEYS),
}


def _same_memory(t, bucket):
    return t.data_ptr() == bucket.data_ptr() and t.numel() == bucket.numel()


@pytest.mark.parametrize("name", sorted(CASES))
def test_seeded_initial_state(name):
    shape, order, trainable, targets, keys = CASES[name]
    ag = getattr(spprl, name)(env_name="custom", env_spec=shape + (1.0, 1000), max_batch=32, buffer_size=64,
                              device="cuda:0", seed=SEED)
    gen = torch.Generator().manual_seed(SEED)
    drawn = {net: nets.linear_init_(torch.empty(nets.numel(lay)), lay, gen) for net, lay in order}
    assert list(ag.layouts) == [net for net, _ in order] and set(ag.params) == set(drawn)
    for net, lay in order:
        assert ag.layouts[net] == lay, net
        assert torch.equal(ag.params[net].cpu(), drawn[targets.get(net, net)]), net
    for targ, src in targets.items():
        assert torch.equal(ag.params[targ], ag.params[src]), (targ, src)
        assert not torch.equal(drawn[targ], drawn[src])  # (the target's own draw differs: the copy is checked)
    for state in (ag.grads, ag.exp_avg, ag.exp_avg_sq):
        assert set(state) == trainable
        for net in trainable:
            assert state[net].shape == ag.params[net].shape and state[net].dtype == torch.float32
            assert not state[net].any(), net
    n = {net: ag.params[net].numel() for net in trainable}
    if name.startswith("SAC"):
        bc, ba, es = ag.bucket_critic, ag.bucket_actor, ag.bucket_critic.element_size()
        assert bc.numel() == n[C1] + n[C2] and ba.numel() == n[A] + 1
        assert ag.grads[C1].data_ptr() == bc.data_ptr() and ag.grads[C1].numel() == n[C1]
        assert ag.grads[C2].data_ptr() == bc.data_ptr() + es * n[C1] and ag.grads[C2].numel() == n[C2]
        assert _same_memory(ag.grads[A], ba[:-1])
        assert _same_memory(ag.alpha_grad, ba[-1:]) and not ag.alpha_grad.any()
        assert _same_memory(ag.grads[ACM], ag.bucket_acm)
    else:
        assert ag.bucket_critic is ag.grads[C1] and ag.bucket_actor is ag.grads[A]
        if name == "DDPG":
            assert ag.bucket_acm is None
        else:
            assert ag.bucket_acm is ag.grads[ACM]
    assert list(ag.collect_params_dict()) == keys
