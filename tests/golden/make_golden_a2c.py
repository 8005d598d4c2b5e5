"""Generator of tests/golden/a2c_vanilla_hcheetah.npz and a2c_acm_hcheetah.npz: the REFERENCE's A2C
(rltoolkit/algorithms/a2c/a2c.py) and A2C_AcM (rltoolkit/acm/on_policy.py) run on the CPU through make_golden.py's
dependency stand-ins, in the build container only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_a2c.py

Seeded networks (weights.fill_params) and hand-filled memories of the three-rollout shape (96 frames, 99
observations).  The stored log-probs are built WITH THEIR GRAPH, per frame, as collect_batch leaves them
(a2c.py:165-166): ``actor.get_actions_dist(buf.normalize(obs_i)).log_prob(act_i)`` BEFORE update_obs_mean_std -- so
the actor's step back-propagates through observations normalised with the rollout's statistics while the critic and
the advantages see the updated ones.

  a2c_vanilla_hcheetah  A2C(env_name="HalfCheetah-v2", obs_norm_alpha=0.95, ...) from running statistics that are no
                        longer the initial zeros and ones (so the update moves them visibly): update_obs_mean_std,
                        update_critic (2 targets x 3 steps, with calculate_advantage), update_actor
  a2c_acm_hcheetah      A2C_AcM(custom_loss=0.5, denormalize_actor_out=True, min_max_denormalize=True,
                        norm_closs=False): update_critic + update_actor on TWO memories in turn; update_actor_acm never
                        zeroes the gradient (on_policy.py:117-124), so the second step applies g1 + g2.
                        norm_closs=True is not recorded: the reference raises there (update_actor_acm passes
                        ``force=True`` to Memory.normalize, which takes no such keyword, memory.py:76).
Only expected outputs are stored; tests rebuild the inputs from the seed.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (installs the stand-ins and puts the reference on sys.path)
import a2c_ref  # noqa: E402
from ppo_ref import GOLDEN_SEED, golden_inputs  # noqa: E402
from rltoolkit.acm.on_policy import A2C_AcM  # noqa: E402
from rltoolkit.algorithms.a2c.a2c import A2C  # noqa: E402
from rltoolkit.buffer import Memory, MemoryAcM  # noqa: E402

# numpy 1.18's float64 percentile weights (see make_golden_ppo.py)
_percentile = np.percentile
np.percentile = lambda a, q, *args, **kw: _percentile(np.asarray(a, np.float64), q, *args, **kw)

HP = dict(gamma=0.99, actor_lr=3e-3, critic_lr=1e-3, critic_num_target_updates=2, num_critic_updates_per_target=3,
          obs_norm_alpha=0.95)


def fill(buf, actor, mem):
    """Frames into a Memory; every frame's log-prob keeps its graph through ``actor`` (a2c.py:165-166)."""
    i, N = 0, len(mem["obs"])
    for s0 in mem["start_obs"]:
        obs = torch.from_numpy(s0[None])
        prev = buf.add_obs(obs)
        while True:
            act = torch.from_numpy(mem["act"][i:i + 1])
            lp = actor.get_actions_dist(buf.normalize(obs)).log_prob(act)
            obs = torch.from_numpy(mem["next_obs"][i:i + 1])
            nxt = buf.add_obs(obs)
            buf.add_timestep(prev, nxt, act, lp, float(mem["rew"][i]), bool(mem["done"][i]), bool(mem["end"][i]))
            prev = nxt
            i += 1
            if mem["end"][i - 1]:
                break
        buf.end_rollout()
    assert i == N == len(buf)
    assert np.array_equal(buf.obs.numpy(), mem["obs"]) and np.array_equal(buf.next_obs.numpy(), mem["next_obs"])
    return buf


def gen_vanilla(seed=GOLDEN_SEED):
    ob, ac = 17, 6
    actor0, critic0, mem = golden_inputs(seed, ob, ac)
    torch.manual_seed(seed)
    a2c = A2C(env_name="HalfCheetah-v2", use_gpu=False, **HP)
    mg.load(a2c.actor, seed * 100)
    mg.load(a2c.critic, seed * 100 + 1)
    assert np.array_equal(mg.flat_params(a2c.actor), actor0) and np.array_equal(mg.flat_params(a2c.critic), critic0)
    # running statistics of an earlier iteration, far enough from this memory's that alpha = 0.95 moves them
    mean0, std0 = a2c_ref.vanilla_start_stats(seed, ob)
    a2c.obs_mean, a2c.obs_std = torch.from_numpy(mean0.copy()), torch.from_numpy(std0.copy())
    buf = fill(Memory(obs_mean=a2c.obs_mean, obs_std=a2c.obs_std, device=a2c.device, alpha=a2c.obs_norm_alpha),
               a2c.actor, mem)
    a2c.buffer = buf
    buf = a2c.update_obs_mean_std(buf)
    out = dict(obs_mean=a2c.obs_mean.numpy(), obs_std=a2c.obs_std.numpy(),
               max_obs=a2c.max_obs.numpy(), min_obs=a2c.min_obs.numpy())
    adv = a2c.update_critic(buf)
    out.update(crit_loss=np.array(a2c.loss["critic"]), crit_post=mg.flat_params(a2c.critic), adv=adv.numpy())
    a2c.update_actor(adv, buf)
    out.update(actor_loss=np.array(a2c.loss["actor"]), actor_post=mg.flat_params(a2c.actor),
               ac_lim=a2c.ac_lim.numpy())
    mg.save("a2c_vanilla_hcheetah.npz", seed=np.array(seed), dims=np.array([ob, ac]),
            **{k: np.array(v) for k, v in HP.items()}, **out)


def gen_acm(seed=a2c_ref.ACM_SEED):
    ob = 17
    actor0, critic0, mems, lo, hi = a2c_ref.acm_inputs(seed, ob)
    torch.manual_seed(seed)
    hp = dict(HP, obs_norm_alpha=None)
    m = A2C_AcM(env_name="HalfCheetah-v2", use_gpu=False, custom_loss=0.5, denormalize_actor_out=True,
                min_max_denormalize=True, norm_closs=False, acm_pre_train_samples=10, acm_val_buffer_size=None, **hp)
    mg.load(m.actor, seed * 100)
    mg.load(m.critic, seed * 100 + 1)
    assert np.array_equal(mg.flat_params(m.actor), actor0) and np.array_equal(mg.flat_params(m.critic), critic0)
    out = {}
    for k, mem in enumerate(mems, 1):
        buf = fill(MemoryAcM(obs_mean=None, obs_std=None, device=m.device, alpha=None, max_obs=torch.from_numpy(hi),
                             min_obs=torch.from_numpy(lo), min_max_denormalize=True), m.actor, mem)
        m.buffer = buf
        adv = m.update_critic(buf)
        m.update_actor(adv, buf)
        out.update({"crit_loss%d" % k: np.array(m.loss["critic"]), "crit_post%d" % k: mg.flat_params(m.critic),
                    "adv%d" % k: adv.numpy(), "actor_post%d" % k: mg.flat_params(m.actor),
                    "losses%d" % k: np.array([m.loss[n] for n in ("actor", "dist", "policy")])})
    mg.save("a2c_acm_hcheetah.npz", seed=np.array(seed), dims=np.array([ob, ob]), custom_loss=np.array(0.5),
            actor_ac_lim=np.asarray(m.actor_ac_lim, np.float32),
            **{k: np.array(v) for k, v in hp.items() if v is not None}, **out)


if __name__ == "__main__":
    gen_vanilla()
    gen_acm()
