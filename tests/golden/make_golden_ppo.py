"""Generator of tests/golden/ppo_vanilla_hcheetah.npz: the REFERENCE's vanilla PPO
(rltoolkit/algorithms/ppo/ppo.py on a2c.py, ``PPO(env_name="HalfCheetah-v2", obs_norm_alpha=0.95,
use_gpu=False)``) run on the CPU through make_golden.py's dependency stand-ins, in the build container only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ppo.py

Seeded networks (weights.fill_params) and a hand-filled ``Memory`` of three rollouts (tests/ppo_ref.py
golden_inputs: 40 frames ended done, 25 ended done, 31 ended by a time limit -- end but not done; 96 frames, 99
observations).  Then the reference's own update_obs_mean_std, update_critic (2 targets x 3 steps, with
calculate_advantage) and update_actor with ppo_batch_size = 96 -- one full-batch minibatch per epoch, so the
DataLoader's shuffle only permutes a mean -- max_ppo_epochs = 4 and a KL threshold between the 2nd and 3rd
epochs' KL (read from a first run without the stop): epochs 0..2 run, the check at i = 3 breaks the loop.
Only expected outputs (and lp_old, which depends on the reference's actor) are stored; tests rebuild the inputs
from the seed.
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
from ppo_ref import GOLDEN_SEED, golden_inputs  # noqa: E402
from rltoolkit.algorithms.ppo import ppo as ppo_mod  # noqa: E402
from rltoolkit.buffer import Memory  # noqa: E402

# One more dependency stand-in, as make_golden.py's ``np.int = int``: the reference pins numpy 1.18, whose
# percentile weights are float64 whatever the data's dtype, so Memory.update_obs_mean_std's percentiles of its
# float32 observations (memory.py:294-295) are interpolated in float64 and then cast by ``.float()``.  numpy >= 2
# casts q to the data's dtype first (0.99 -> float32: the interpolation fraction moves by ~1e-5 relative).
_percentile = np.percentile
np.percentile = lambda a, q, *args, **kw: _percentile(np.asarray(a, np.float64), q, *args, **kw)

HP = dict(gamma=0.99, actor_lr=3e-3, critic_lr=1e-3, critic_num_target_updates=2, num_critic_updates_per_target=3,
          ppo_batch_size=96, entropy_coef=0.01, obs_norm_alpha=0.95)


def gen(seed=GOLDEN_SEED):
    ob, ac = 17, 6
    actor0, critic0, mem = golden_inputs(seed, ob, ac)
    N = len(mem["obs"])

    def run(thr, max_epochs):
        torch.manual_seed(seed)
        ppo = ppo_mod.PPO(env_name="HalfCheetah-v2", use_gpu=False, max_ppo_epochs=max_epochs, kl_div_threshold=thr,
                          **HP)
        mg.load(ppo.actor, seed * 100)
        mg.load(ppo.critic, seed * 100 + 1)
        assert np.array_equal(mg.flat_params(ppo.actor), actor0) and np.array_equal(mg.flat_params(ppo.critic), critic0)
        buf = Memory(obs_mean=ppo.obs_mean, obs_std=ppo.obs_std, device=ppo.device, alpha=ppo.obs_norm_alpha)
        # lp_old: the stored actions' log-probs under the actor on the observations normalised with the statistics
        # in force during the rollout (zeros and ones), off by a seeded noise so the ratios spread around 1
        with torch.no_grad():
            lp_cur = ppo.actor.get_actions_dist(buf.normalize(torch.from_numpy(mem["obs"]))).log_prob(
                torch.from_numpy(mem["act"])).numpy()
        lp_old = (lp_cur + mem["lp_noise"]).astype(np.float32)
        i = 0
        for r, s0 in enumerate(mem["start_obs"]):
            prev = buf.add_obs(torch.from_numpy(s0[None]))
            while True:
                nxt = buf.add_obs(torch.from_numpy(mem["next_obs"][i:i + 1]))
                buf.add_timestep(prev, nxt, torch.from_numpy(mem["act"][i:i + 1]), torch.from_numpy(lp_old[i:i + 1]),
                                 float(mem["rew"][i]), bool(mem["done"][i]), bool(mem["end"][i]))
                prev = nxt
                i += 1
                if mem["end"][i - 1]:
                    break
            buf.end_rollout()
        assert i == N == len(buf) and buf.current_len == N + len(mem["start_obs"])
        assert np.array_equal(buf.obs.numpy(), mem["obs"]) and np.array_equal(buf.next_obs.numpy(), mem["next_obs"])
        ppo.buffer = buf
        buf = ppo.update_obs_mean_std(buf)
        out = dict(obs_mean=ppo.obs_mean.numpy(), obs_std=ppo.obs_std.numpy(), max_obs=ppo.max_obs.numpy(),
                   min_obs=ppo.min_obs.numpy())
        assert (buf.norm_obs.numpy() == 10.0).any()  # the clip is reached
        adv = ppo.update_critic(buf)
        out.update(crit_loss=np.array(ppo.loss["critic"]), crit_post=mg.flat_params(ppo.critic), adv=adv.numpy())
        kls = []
        real = ppo_mod.utils.kl_divergence

        def rec(log_p, log_q):
            kls.append(real(log_p, log_q))
            return kls[-1]

        ppo_mod.utils.kl_divergence = rec
        try:
            ppo.update_actor(adv, buf)
        finally:
            ppo_mod.utils.kl_divergence = real
        out.update(kls=np.array(kls), losses=np.array([ppo.loss[k] for k in ("actor", "entropy", "sum")]),
                   counter=np.array(ppo.kl_div_updates_counter), actor_post=mg.flat_params(ppo.actor), lp_old=lp_old,
                   eps=np.array(ppo.ppo_epsilon), gae_lambda=np.array(ppo.gae_lambda),
                   ac_lim=ppo.ac_lim.numpy(), max_ep_len=np.array(ppo.max_ep_len))
        return out

    kls = run(1e9, 4)["kls"]
    assert len(kls) == 4 and max(kls[:2]) + 2e-3 < kls[2], kls  # a crossing with margin on both sides
    thr = 0.5 * (max(kls[:2]) + kls[2])
    out = run(thr, 4)
    assert len(out["kls"]) == 3 and int(out["counter"]) == 4, (out["kls"], out["counter"])
    print("ppo vanilla: kl per epoch", [round(float(k), 5) for k in kls], "threshold", round(float(thr), 5))
    mg.save("ppo_vanilla_hcheetah.npz", seed=np.array(seed), dims=np.array([ob, ac]), threshold=np.array(thr),
            max_epochs=np.array(4), **{k: np.array(v) for k, v in HP.items()}, **out)


if __name__ == "__main__":
    gen()
