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
A2C's own update (TD advantage, one policy-gradient step) is spprl.A2C (a2c.py), a subclass of this loop.
Out of scope: discrete actions, data parallelism, TensorBoard.
"""
import numpy as np
import torch

from . import config
from ._lib import call, ptr, stream_handle
from .dp import stream_key
from .onpolicy import OnPolicyNets, actor_layout, critic_layout, obs_stats
from .ppo import calculate_gae
from .trainer import StatsLogger, SynthVecEnv


class PPO:
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
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("spprl.PPO is single-process: data parallelism is PPO_AcM's")
        if obs_norm_alpha is not None and not 0 <= obs_norm_alpha <= 1:
            raise ValueError("obs_norm_alpha needs to be in <0, 1> range")  # memory.py:142-143
        ob, ac, ac_high, max_ep = env_spec or config.ENV_SPECS[env_name]
        self.env_name, self.ob_dim, self.ac_dim = env_name, ob, ac
        self.device = torch.device(device)
        self.gamma, self.gae_lambda = gamma, gae_lambda
        self.batch_size, self.iterations, self.stats_freq = int(batch_size), int(iterations), int(stats_freq)
        self.test_episodes, self.return_done, self.max_frames = test_episodes, return_done, max_frames
        # a2c.py:137 tests the alpha's truth, so 0 switches the reference's update off although its docstring gives
        # 0 the meaning "replace old mean and std" (a2c.py:41-45); here only None is off and 0 replaces
        self.obs_norm_alpha = None if obs_norm_alpha is None else float(obs_norm_alpha)
        self.actor_output_dim = ac
        if env is None:
            env = SynthVecEnv(n_envs, ob, ac, max_episode_steps=max_ep, ac_high=ac_high, seed=loop_seed,
                              device=self.device)
        self.env = env
        self.n_envs = E = env.n
        self.T = 1 if E == 1 else max(1, -(-self.batch_size // E))
        Nmax = max(self.T * E, self.batch_size + (max_ep or 1000) if E == 1 else 0)
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
        import os

        if os.environ.get("SPP_PPO_EPOCH_KERNEL", "0") != "1":
            self.nets._epoch_max_bs = 0  # _epoch_kernel_ok: the per-minibatch path
        d = self.device
        # rl.py:389-405: zeros and ones when the normaliser is on, else None
        on = self.obs_norm_alpha is not None
        self.obs_mean = torch.zeros(ob, device=d) if on else None
        self.obs_std = torch.ones(ob, device=d) if on else None
        self.max_obs, self.min_obs = torch.zeros(ob, device=d), torch.zeros(ob, device=d)
        self._have_minmax = False
        self.stats_logger = StatsLogger()
        self.iteration = 0
        self.loop_seed, self._ctr = int(loop_seed), 0
        self._key_policy = stream_key(loop_seed, "policy")
        self.loss = {"actor": 0.0, "critic": 0.0}  # a2c.py:91
        self._ep_ret = torch.zeros(E, device=d)
        self._ret_sums = torch.zeros(2, dtype=torch.float64, device=d)
        self._obs = None
        self._starts = []

    @property
    def kl_div_updates_counter(self):  # ppo.py:91, 192 (epochs + 1 per update_actor)
        return self.nets.kl_div_updates_counter

    @kl_div_updates_counter.setter
    def kl_div_updates_counter(self, v):  # ppo.py:226 resets it after logging
        self.nets.kl_div_updates_counter = int(v)

    def pre_train(self):
        raise AttributeError("vanilla PPO has no ACM pre-training (rltoolkit PPO defines none)")

    def update_acm(self, *a, **k):
        raise AttributeError("vanilla PPO has no ACM (rltoolkit PPO defines none)")

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
    def train(self, iterations=None):
        if iterations:
            self.iterations += iterations
        while self.iteration < self.iterations:
            ret = self.perform_iteration()
            running = self.stats_logger.calc_running_return(ret)
            if self.return_done is not None and running is not None and running >= self.return_done:
                break
            if self.test_episodes and self.iteration % self.stats_freq == 0:
                self.stats_logger.test_return = self.test()
            self.iteration += 1
            if self.max_frames is not None and self.max_frames < self.stats_logger.frames:
                break
        return self.stats_logger.running_return

    def perform_iteration(self, sync=True):
        """a2c.py:122-142.  Returns the mean return of the episodes completed (None if none)."""
        self._ret_sums.zero_()
        self.update(self.collect_batch())
        if not sync:
            return None
        s = self._ret_sums.cpu().numpy()
        return float(s[0] / s[1]) if s[1] > 0 else None

    # ---------------------------------------------------------------- A2C.collect_batch
    def _start(self):
        self._obs = self.env.reset()
        self._starts.append(self._obs.clone())
        self._ep_ret.zero_()
        self._ep_len = np.zeros(self.n_envs, np.int64)

    def collect_batch(self):
        """Rollout memory, time-major [T][E]: RAW obs and next obs, actions, log-probs, rewards, done, end, and
        start_obs, the first observation of every rollout (of this iteration's segment for envs that run on)."""
        E = self.n_envs
        self._starts = []
        if E == 1:  # whole episodes until batch_size frames (a2c.py:155-184)
            flat = []
            while len(flat) < self.batch_size:
                self.stats_logger.rollouts += 1
                self._start()
                end = False
                while not end:
                    step = self._step()
                    end = bool(step[-1])
                    flat.append(step[:-1])
        else:
            if self._obs is None:
                self._start()
                self.stats_logger.rollouts += E
            else:
                self._starts.append(self._obs.clone())  # the envs run on: this segment's first observations
            flat = [self._step()[:-1] for _ in range(self.T)]
        T = len(flat)
        cat = lambda k: torch.stack([f[k] for f in flat])  # noqa: E731
        mem = {"obs": cat(0), "act": cat(1), "lp": cat(2), "rew": cat(3), "done": cat(4), "end": cat(5),
               "next_obs": cat(6), "start_obs": torch.cat(self._starts), "T": T}
        if E > 1:
            mem["end"][-1].fill_(1)  # segment truncation: GAE bootstraps from V(s') (ppo.py:136-148)
        self.stats_logger.frames += T * E
        return mem

    def _step(self):
        E = self.n_envs
        raw = self._obs.clone()  # (the env's obs buffers alternate: keep this step's)
        self._ctr += 1
        act, lp, _, _ = self.nets.rollout_act(raw, self.obs_mean, self.obs_std, self._key_policy, self._ctr)
        nobs, rew, end, end_dev = self.env.step(self.process_action(act))
        # a2c.py:168-171: end = env done; done = False when the episode hit max_ep_len (a time-limit end)
        self._ep_len += 1
        max_ep = getattr(self.env, "_max_episode_steps", None)
        done_h = end & (self._ep_len != max_ep) if max_ep else end.copy()
        self._ep_len[end] = 0
        done = (torch.from_numpy(done_h.astype(np.uint8)).to(self.device) if done_h.any()
                else torch.zeros(E, dtype=torch.uint8, device=self.device))
        any_end = bool(end.any())
        call("sppEpisodeAccum", ptr(rew), ptr(end_dev) if any_end else None, E, ptr(self._ep_ret),
             ptr(self._ret_sums), stream_handle())
        out = (raw, act, lp, rew.clone(), done, end_dev.clone(), nobs.clone(), any_end if E == 1 else False)
        self._obs = nobs
        if any_end and E > 1:
            self.stats_logger.rollouts += int(end.sum())
            self._obs = self.env.reset(end)
            self._starts.append(self._obs[torch.as_tensor(np.flatnonzero(end), device=self.device)].clone())
        return out

    # ---------------------------------------------------------------- update (statistics, critic, GAE, actor)
    def update(self, mem):
        """The iteration's update on a memory dict (collect_batch's, or a caller's: obs / next_obs [T][E][ob] RAW,
        act [T][E][ac], lp / rew / done / end [T][E], start_obs [R][ob], T, optionally E)."""
        T, E, ob = mem["T"], mem.get("E", self.n_envs), self.ob_dim
        N = T * E
        dev = lambda t, dt=torch.float32: torch.as_tensor(t).to(self.device, dt).contiguous()  # noqa: E731
        mem = dict(mem, obs=dev(mem["obs"]).reshape(N, ob), next_obs=dev(mem["next_obs"]).reshape(N, ob),
                   start_obs=dev(mem["start_obs"]).reshape(-1, ob))
        if self.obs_norm_alpha is not None:
            self.update_obs_mean_std(mem)  # a2c.py:137-138
        obs, nobs = self.normalize(mem["obs"]), self.normalize(mem["next_obs"])  # Memory.norm_obs / norm_next_obs
        rew, done = dev(mem["rew"]).reshape(N), dev(mem["done"]).reshape(N)
        self.nets.update_critic(obs, nobs, rew, done)  # a2c.py:186-225
        v = self.nets.value(obs).reshape(T, E)
        v_next = self.nets.value(nobs).reshape(T, E)
        _, adv = calculate_gae(rew.reshape(T, E), v, v_next, done.reshape(T, E), dev(mem["end"]).reshape(T, E),
                               self.gamma, self.gae_lambda)  # ppo.py:101-150
        self.last_advantages = adv
        self.nets.update_actor(adv.reshape(N), obs, dev(mem["act"]).reshape(N, self.ac_dim), dev(mem["lp"]).reshape(N))
        self.loss = dict(self.nets.loss_sums, critic=self.nets.loss["critic"])  # ppo.py:164-187: sums, not means

    # ---------------------------------------------------------------- test (a2c.py:325-350)
    def test(self, episodes=None):
        episodes = episodes or self.test_episodes or 1
        env = self.env.spawn(episodes, seed=self.loop_seed + 99991)
        obs = env.reset()
        ret = torch.zeros(episodes, device=self.device)
        sums = torch.zeros(2, dtype=torch.float64, device=self.device)
        alive = np.ones(episodes, bool)
        while alive.any():
            act, _, _, _ = self.nets.rollout_act(obs.clone(), self.obs_mean, self.obs_std, 0, 0, deterministic=True)
            obs, rew, end, _ = env.step(self.process_action(act))
            m = torch.as_tensor((end & alive).astype(np.uint8), device=self.device)
            call("sppEpisodeAccum", ptr(rew), ptr(m), episodes, ptr(ret), ptr(sums), stream_handle())
            alive &= ~end
            if end.any() and alive.any():
                obs = env.reset(end)
        s = sums.cpu().numpy()
        return float(s[0] / s[1])

    # ---------------------------------------------------------------- checkpoints (rl.py:263-301)
    def collect_params_dict(self):
        from . import nets as _nets

        cpu = lambda t: None if t is None else t.cpu()  # noqa: E731
        return {"actor": _nets.state_dict(self.nets.params[0], actor_layout(self.ob_dim, self.ac_dim)),
                "critic": _nets.state_dict(self.nets.params[1], critic_layout(self.ob_dim)),
                "obs_mean": cpu(self.obs_mean), "obs_std": cpu(self.obs_std),
                "min_obs": self.min_obs.cpu() if self._have_minmax else None,
                "max_obs": self.max_obs.cpu() if self._have_minmax else None}

    def apply_params_dict(self, d):
        from . import nets as _nets

        for i, (k, lay) in enumerate((("actor", actor_layout(self.ob_dim, self.ac_dim)),
                                      ("critic", critic_layout(self.ob_dim)))):
            _nets.load_state(self.nets.params[i], lay, d[k])
        dev = lambda t: torch.as_tensor(t, dtype=torch.float32).to(self.device).clone()  # noqa: E731
        if d.get("obs_mean") is not None and d.get("obs_std") is not None:
            self.obs_mean, self.obs_std = dev(d["obs_mean"]), dev(d["obs_std"])
        else:
            self.obs_mean = self.obs_std = None
        self._have_minmax = d.get("min_obs") is not None and d.get("max_obs") is not None
        if self._have_minmax:
            self.min_obs, self.max_obs = dev(d["min_obs"]), dev(d["max_obs"])

    def save(self, path):  # rl.py:281-292
        from .checkpoint import save_params

        save_params(path, self.collect_params_dict())

    def load(self, path):  # rl.py:294-301
        from .checkpoint import load_params

        self.apply_params_dict(load_params(path))
