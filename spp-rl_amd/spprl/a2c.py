"""Vanilla A2C: rltoolkit/algorithms/a2c/a2c.py on the MI355X library -- the class every on-policy algorithm of the
reference sits on, and the baseline of the SPP-A2C curves.  ``spprl.PPO``'s loop (rollout act, Memory normaliser,
collect_batch, test, checkpoints: ppo_vanilla.py) with A2C's own update:

  perform_iteration   a2c.py:122-142: collect, update_obs_mean_std, update_critic, calculate_advantage, update_actor
  calculate_advantage a2c.py:227-265: adv = r + gamma (1 - done) V(s') - V(s), one launch with its moments
                      (sppOnpTdAdvantage); SPP_A2C_FUSED_ADV=0 runs two sppOnpValue launches and torch arithmetic
  update_actor        a2c.py:267-286: ONE full-batch Adam step on (-logp * A).mean(), A normalised over the whole
                      batch with std + 1e-8 (not AdvantageDataset's + 1.2e-7), applied inside sppOnpPgActorGrads
  loss                {"actor", "critic"} (a2c.py:91)

Ordering quirk kept: the critic and the advantages see observations normalised with the statistics
updated just before them, but the actor's loss back-propagates through the log-probs stored WHILE ACTING
(a2c.py:165-166, 279-285), i.e. of observations normalised with the statistics in force during the rollout.  The
actor has not changed since the rollout, so recomputing those log-probs on the rollout-normalised observations gives
the same gradient; update(mem) keeps a copy of the statistics before it updates them.
Out of scope: discrete actions (the reference's CartPole default), data parallelism, TensorBoard.
"""
import torch

from . import config
from ._lib import call, ptr, stream_handle
from .onpolicy_loop import refuse_process_group
from .ppo_vanilla import PPO

# PPO.__init__'s loop / environment keywords A2C passes through
_LOOP_KWARGS = ("iterations", "stats_freq", "test_episodes", "return_done", "max_frames", "n_envs", "env", "env_spec",
                "device", "seed", "loop_seed")


class A2C(PPO):
    def __init__(self, env_name="HalfCheetah-v2", gamma=config.GAMMA, actor_lr=3e-3, critic_lr=3e-4,
                 critic_num_target_updates=10, num_critic_updates_per_target=10, normalize_adv=True,
                 obs_norm_alpha=0.99, batch_size=config.BATCH_SIZE, **kw):
        config.refuse_keywords("A2C", kw, config.ACM_ONLY_ON_POLICY, config.PPO_ONLY)
        config.check_kwargs("A2C", {k: v for k, v in kw.items() if k not in _LOOP_KWARGS},
                            {k: v for k, v in config.ON_POLICY_NO_EFFECT_KWARGS.items() if k != "obs_norm_alpha"})
        refuse_process_group("A2C")
        super().__init__(env_name=env_name, gamma=gamma, actor_lr=actor_lr, critic_lr=critic_lr,
                         critic_num_target_updates=critic_num_target_updates,
                         num_critic_updates_per_target=num_critic_updates_per_target, normalize_adv=normalize_adv,
                         obs_norm_alpha=obs_norm_alpha, batch_size=batch_size, **kw)
        self.normalize_adv = bool(normalize_adv)

    kl_div_updates_counter = None  # (PPO's counter: A2C has none)

    def actor_observations(self, raw_obs, rollout_mean, rollout_std):
        """The observations the stored log-probs were taken on: standardize_and_clip with the ROLLOUT's statistics
        (a2c.py:165-166), not the ones update_obs_mean_std has just written."""
        if rollout_mean is None:
            return raw_obs
        out = torch.empty_like(raw_obs)
        call("sppObsNormalize", ptr(raw_obs), raw_obs.shape[0], self.ob_dim, None, None, ptr(rollout_mean),
             ptr(rollout_std), 0, 0, ptr(out), stream_handle())
        self._keep_actor_norm = (raw_obs, rollout_mean, rollout_std)
        return out

    def update(self, mem):
        """a2c.py:137-142 on a memory dict (collect_batch's, or a caller's: PPO.update's keys; ``lp`` and ``end``
        are not read -- the log-probs are recomputed with their graph, the TD advantage needs no episode ends)."""
        _, _, N, mem = self._flatten(mem)
        on = self.obs_norm_alpha is not None  # (the rollout's statistics, before _normalized updates them)
        rollout_mean, rollout_std = (self.obs_mean.clone(), self.obs_std.clone()) if on else (None, None)
        obs, nobs, rew, done = self._normalized(mem, N)
        self.nets.update_critic(obs, nobs, rew, done, advantages=False)  # a2c.py:186-222
        adv, mom = self.nets.td_advantage(obs, nobs, rew, done)  # a2c.py:223, 227-265
        self.last_advantages = adv
        out = self.nets.pg_actor_step(self.actor_observations(mem["obs"], rollout_mean, rollout_std),
                                      self._dev(mem["act"]).reshape(N, self.ac_dim), adv,
                                      mom if self.normalize_adv else None)  # a2c.py:267-286
        self.loss = {"actor": float(out[0].item()), "critic": self.nets.loss["critic"]}
