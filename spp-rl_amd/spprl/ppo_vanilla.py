"""Vanilla PPO: rltoolkit/algorithms/ppo/ppo.py on algorithms/a2c/a2c.py (train/vanilla_ppo_hcheetah.py,
train/vanilla_ppo_hopper.py) on the MI355X library.  The baseline of the SPP-PPO curves: PPO_AcM with the AcM
taken out.  The actor (``OnPolicyNets(ob, ac)``) emits the env action, ``process_action`` is the identity, and
the observations are normalised by the running Memory normaliser (``obs_norm_alpha``), which PPO_AcM never runs.

  collect_batch         a2c.py:144-184: whole episodes until batch_size frames (n_envs = 1), or PPO_AcM's lockstep
                        [T][E] scheme; a time-limit end is ``end`` but not ``done``.  The memory holds RAW obs /
                        next obs and each rollout's first observation; actions and log-probs are the policy's on the
                        observation normalised with the statistics in force during the rollout.
  perform_iteration     a2c.py:122-142: collect, update_obs_mean_std, update_critic, GAE, update_actor.  The
                        reference's ordering quirk is kept: critic and actor train on observations normalised with
                        the statistics updated just before them, lp_old stays the rollout's.
  update_obs_mean_std   buffer/memory.py:283-302 (sppOnpObsStats): mean / unbiased std over every observation of the
                        iteration blended as (1 - alpha) new + alpha old from zeros and ones (rl.py:389-405); max /
                        min_obs the running max / min of the exact 99th / 1st percentile of the frames' obs rows.
  loss                  ppo.py:164-187: actor / entropy / sum are SUMS over all minibatch steps (not divided by the
                        epochs as acm/on_policy.py divides), critic the mean over its steps (a2c.py:217-219).
  checkpoints           rl.py:263-279: actor, critic, obs_mean, obs_std, min_obs, max_obs.

Rollout step: one launch (sppOnpRolloutAct: normalise, draw, actor forward from the canonical parameters, log-prob)
for up to onpolicy.FUSED_ACT_MAX_ROWS envs; SPP_PPO_FUSED_ACT=0 or more envs run sppObsNormalize + sppRandNormal +
sppOnpAct on the same draws.  The actor's minibatch steps run one by one (sppOnpActorGrads / Apply) unless
SPP_PPO_EPOCH_KERNEL=1 selects the one-launch epochs (sppOnpActorEpoch at (17, 6) / (11, 3)): measured, they did not
raise env-steps/s by more than the run-to-run spread at the reference cadence.
train, collect_batch, the per-step bookkeeping, test and save / load are OnPolicyLoop's (onpolicy_loop.py), shared
with PPO_AcM; this class states its act call, what its memory records and its update.
A2C's own update (TD advantage, one policy-gradient step) is spprl.A2C (a2c.py), a subclass of this loop.
Out of scope: discrete actions, data parallelism, TensorBoard.
"""
import os

import numpy as np
import torch

from . import config
from ._lib import call, ptr, stream_handle
from .onpolicy import OnPolicyNets, obs_stats
from .onpolicy_loop import OnPolicyLoop, refuse_process_group
from .ppo import calculate_gae


class PPO(OnPolicyLoop):
    def __init__(self, env_name="HalfCheetah-v2", gamma=config.GAMMA, actor_lr=3e-3, critic_lr=3e-4, epsilon=0.2,
                 gae_lambda=0.95, kl_div_threshold=0.15, max_ppo_epochs=50, ppo_batch_size=1000, entropy_coef=0.0,
                 critic_num_target_updates=10, num_critic_updates_per_target=10, normalize_adv=True,
                 obs_norm_alpha=0.99, batch_size=config.BATCH_SIZE, iterations=config.ITERATIONS,
                 stats_freq=config.STATS_FREQ, test_episodes=None, return_done=None, max_frames=None, n_envs=1,
                 env=None, env_spec=None, device="cuda", seed=None, loop_seed=0, **unused):
        # PPO -> A2C -> RL -> MetaLearner (ppo.py:15-25, a2c.py:17-27, rl.py:116-132, 17-26) take no AcM keyword and
        # no **kwargs at the end of the chain: raised here, before the library is touched
        config.refuse_keywords("PPO", unused, config.ACM_ONLY_ON_POLICY)
        config.check_kwargs("PPO", unused, {k: v for k, v in config.ON_POLICY_NO_EFFECT_KWARGS.items()
                                            if k != "obs_norm_alpha"})  # (taken explicitly and honoured)
        refuse_process_group("PPO")
        if obs_norm_alpha is not None and not 0 <= obs_norm_alpha <= 1:
            raise ValueError("obs_norm_alpha needs to be in <0, 1> range")  # memory.py:142-143
        ac_high, _, Nmax = self._init_loop(env_name, env_spec, device, gamma, gae_lambda, batch_size, iterations,
                                           stats_freq, test_episodes, return_done, max_frames, n_envs, env, loop_seed)
        ob, ac = self.ob_dim, self.ac_dim
        # a2c.py:137 tests the alpha's truth, so 0 switches the reference's update off although its docstring gives
        # 0 the meaning "replace old mean and std" (a2c.py:41-45); here only None is off and 0 replaces
        self.obs_norm_alpha = None if obs_norm_alpha is None else float(obs_norm_alpha)
        self.actor_output_dim = ac
        self.nets = OnPolicyNets(ob, ac, ac_lim=ac_high, actor_lr=actor_lr, critic_lr=critic_lr, ppo_epsilon=epsilon,
                                 entropy_coef=entropy_coef, gamma=gamma, gae_lambda=gae_lambda,
                                 critic_num_target_updates=critic_num_target_updates,
                                 num_critic_updates_per_target=num_critic_updates_per_target,
                                 max_ppo_epochs=max_ppo_epochs, ppo_batch_size=ppo_batch_size,
                                 kl_div_threshold=kl_div_threshold, normalize_adv=normalize_adv,
                                 max_batch=max(Nmax, ppo_batch_size), device=self.device, seed=seed)
        # The one-launch actor epoch (sppOnpActorEpoch at aout != ob) is opt-in here, SPP_PPO_EPOCH_KERNEL=1: at the
        # reference cadence the update is ~5 % of an iteration, and the kernel's gain on it (about 7 against 9 ms per
        # iteration) did not move env-steps/s by more than the run-to-run spread (profiles/r09/)
        if os.environ.get("SPP_PPO_EPOCH_KERNEL", "0") != "1":
            self.nets._epoch_max_bs = 0  # _epoch_kernel_ok: the per-minibatch path
        d = self.device
        # rl.py:389-405: zeros and ones when the normaliser is on, else None
        on = self.obs_norm_alpha is not None
        self.obs_mean = torch.zeros(ob, device=d) if on else None
        self.obs_std = torch.ones(ob, device=d) if on else None
        self.max_obs, self.min_obs = torch.zeros(ob, device=d), torch.zeros(ob, device=d)
        self._have_minmax = False
        self.loss = {"actor": 0.0, "critic": 0.0}  # a2c.py:91
        self._starts = []  # the first observation of every rollout since the last memory (_memory takes them)

    def pre_train(self):
        name = type(self).__name__
        raise AttributeError("vanilla %s has no ACM pre-training (rltoolkit %s defines none)" % (name, name))

    def update_acm(self, *a, **k):
        name = type(self).__name__
        raise AttributeError("vanilla %s has no ACM (rltoolkit %s defines none)" % (name, name))

    update_acm_batches = update_actor_acm = update_acm

    # ---------------------------------------------------------------- normaliser (memory.py:76-88, 283-302)
    def normalize(self, x):
        """standardize_and_clip with the running statistics; obs_norm_alpha None: unchanged (memory.py:84-85)."""
        x = x.contiguous()
        if self.obs_mean is None:
            return x.clone()  # the caller keeps it: never alias the env's double-buffered obs
        out = torch.empty_like(x)
        call("sppObsNormalize", ptr(x), x.numel() // self.ob_dim, self.ob_dim, None, None, ptr(self.obs_mean),
             ptr(self.obs_std), 0, 0, ptr(out), stream_handle())
        self._keep_norm = x
        return out

    def update_obs_mean_std(self, mem):
        """Memory.update_obs_mean_std on the iteration's memory: every observation (each rollout's first + every
        next observation) for mean / std, the frames' obs rows for the percentiles."""
        self._keep_stats = obs_stats(mem["start_obs"], mem["next_obs"], mem["obs"], self.obs_norm_alpha, self.obs_mean,
                                     self.obs_std, self.max_obs, self.min_obs, self._have_minmax)
        self._have_minmax = True

    def process_action(self, action, norm_obs=None):
        return action  # a2c.py:311-323: the policy's action goes to the env as it is

    # ---------------------------------------------------------------- RL.train / perform_iteration
    def perform_iteration(self, sync=True):
        """a2c.py:122-142.  Returns the mean return of the episodes completed (None if none)."""
        self._ret_sums.zero_()
        self.update(self.collect_batch())
        return self._mean_return(sync)

    # ---------------------------------------------------------------- A2C.collect_batch
    def _start(self):
        super()._start()
        self._starts.append(self._obs.clone())

    def _run_on(self):
        self._starts.append(self._obs.clone())  # the envs run on: this segment's first observations

    def _memory(self, flat):
        """Rollout memory, time-major [T][E]: RAW obs and next obs, actions, log-probs, rewards, done, end, and
        start_obs, the first observation of every rollout (of this iteration's segment for envs that run on)."""
        mem = super()._memory(flat)
        starts, self._starts = self._starts, []
        mem["start_obs"] = torch.cat(starts)
        return mem

    def _step(self):
        raw = self._obs.clone()  # (the env's obs buffers alternate: keep this step's)
        self._ctr += 1
        act, lp, _, _ = self.nets.rollout_act(raw, self.obs_mean, self.obs_std, self._key_policy, self._ctr)
        nobs, rew, end, end_dev = self.env.step(self.process_action(act))
        tail, reset = self._account(nobs, rew, end, end_dev)
        if reset:
            self._starts.append(self._obs[torch.as_tensor(np.flatnonzero(end), device=self.device)].clone())
        return (raw, act, lp) + tail

    # ---------------------------------------------------------------- update (statistics, critic, GAE, actor)
    def _dev(self, t):
        return torch.as_tensor(t).to(self.device, torch.float32).contiguous()

    def _flatten(self, mem):
        """(T, E, N = T * E, the memory with obs / next_obs [N][ob] and start_obs [R][ob] on the device)."""
        T, E, ob = mem["T"], mem.get("E", self.n_envs), self.ob_dim
        N = T * E
        return T, E, N, dict(mem, obs=self._dev(mem["obs"]).reshape(N, ob),
                             next_obs=self._dev(mem["next_obs"]).reshape(N, ob),
                             start_obs=self._dev(mem["start_obs"]).reshape(-1, ob))

    def _normalized(self, mem, N):
        """The statistics' update on the flattened memory (a2c.py:137-138), then (obs, next obs) normalised with them
        and (rew, done) [N] on the device."""
        if self.obs_norm_alpha is not None:
            self.update_obs_mean_std(mem)
        obs, nobs = self.normalize(mem["obs"]), self.normalize(mem["next_obs"])  # Memory.norm_obs / norm_next_obs
        return obs, nobs, self._dev(mem["rew"]).reshape(N), self._dev(mem["done"]).reshape(N)

    def update(self, mem):
        """The iteration's update on a memory dict (collect_batch's, or a caller's: obs / next_obs [T][E][ob] RAW,
        act [T][E][ac], lp / rew / done / end [T][E], start_obs [R][ob], T, optionally E)."""
        T, E, N, mem = self._flatten(mem)
        obs, nobs, rew, done = self._normalized(mem, N)
        self.nets.update_critic(obs, nobs, rew, done)  # a2c.py:186-225
        v = self.nets.value(obs).reshape(T, E)
        v_next = self.nets.value(nobs).reshape(T, E)
        _, adv = calculate_gae(rew.reshape(T, E), v, v_next, done.reshape(T, E), self._dev(mem["end"]).reshape(T, E),
                               self.gamma, self.gae_lambda)  # ppo.py:101-150
        self.last_advantages = adv
        self.nets.update_actor(adv.reshape(N), obs, self._dev(mem["act"]).reshape(N, self.ac_dim),
                               self._dev(mem["lp"]).reshape(N))
        self.loss = dict(self.nets.loss_sums, critic=self.nets.loss["critic"])  # ppo.py:164-187: sums, not means

    # ---------------------------------------------------------------- test (a2c.py:325-350)
    def _test_action(self, obs):
        act, _, _, _ = self.nets.rollout_act(obs.clone(), self.obs_mean, self.obs_std, 0, 0, deterministic=True)
        return self.process_action(act)

    # ---------------------------------------------------------------- checkpoints (rl.py:263-279)
    def collect_params_dict(self):
        cpu = lambda t: None if t is None else t.cpu()  # noqa: E731
        return {**self._nets_state(), "obs_mean": cpu(self.obs_mean), "obs_std": cpu(self.obs_std),
                "min_obs": self.min_obs.cpu() if self._have_minmax else None,
                "max_obs": self.max_obs.cpu() if self._have_minmax else None}

    def apply_params_dict(self, d):
        self._load_nets(d)
        dev = lambda t: torch.as_tensor(t, dtype=torch.float32).to(self.device).clone()  # noqa: E731
        if d.get("obs_mean") is not None and d.get("obs_std") is not None:
            self.obs_mean, self.obs_std = dev(d["obs_mean"]), dev(d["obs_std"])
        else:
            self.obs_mean = self.obs_std = None
        self._have_minmax = d.get("min_obs") is not None and d.get("max_obs") is not None
        if self._have_minmax:
            self.min_obs, self.max_obs = dev(d["min_obs"]), dev(d["max_obs"])
