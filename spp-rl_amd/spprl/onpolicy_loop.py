"""What the on-policy agents share: rltoolkit's A2C loop (algorithms/a2c/a2c.py on rl.py) around a class's own act and
update.  ``PPO`` (ppo_vanilla.py) and ``PPO_AcM`` (ppo_acm.py) derive from ``OnPolicyLoop``; ``A2C`` and ``A2C_AcM``
change only the update on top of them.

  _init_loop            the env spec, the default SynthVecEnv, n_envs / T, the counters and the episode accounting
  train                 rl.py:192-229
  collect_batch         a2c.py:144-184: whole episodes until batch_size frames (n_envs = 1), or T lockstep steps of E
                        envs that run on across iterations, the last step a truncation (end = 1, done = 0)
  _account              one step's bookkeeping: a time-limit end is ``end`` but not ``done`` (a2c.py:168-171), the
                        episode returns, the resets of a vectorized env
  test                  a2c.py:325-350 over the class's deterministic action
  checkpoints           rl.py:263-301: save / load, the actor / critic entries

A class states what tells it apart by overriding: ``_start`` / ``_run_on`` (what a rollout's first observations
record), ``_step`` (its act call and recorded tuple), ``_memory`` (what joins the stacked memory), ``_test_action``,
``update`` and the rest of its checkpoint.
"""
import numpy as np
import torch
import torch.distributed as dist

from . import config, nets
from ._lib import call, ptr, stream_handle
from .checkpoint import load_params, save_params
from .dp import stream_key
from .trainer import StatsLogger, SynthVecEnv


def refuse_process_group(owner):
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("spprl.%s is single-process: data parallelism is PPO_AcM's" % owner)


class OnPolicyLoop:
    def _init_loop(self, env_name, env_spec, device, gamma, gae_lambda, batch_size, iterations, stats_freq,
                   test_episodes, return_done, max_frames, n_envs, env, loop_seed):
        """The constructor half every class shares.  Returns (ac_high, max_ep, Nmax): the env's action limit and
        episode limit, and the most frames one collect_batch can return."""
        ob, ac, ac_high, max_ep = env_spec or config.ENV_SPECS[env_name]
        self.env_name, self.ob_dim, self.ac_dim = env_name, ob, ac
        self.device = torch.device(device)
        self.gamma, self.gae_lambda = gamma, gae_lambda
        self.batch_size, self.iterations, self.stats_freq = int(batch_size), int(iterations), int(stats_freq)
        self.test_episodes, self.return_done, self.max_frames = test_episodes, return_done, max_frames
        if env is None:
            env = SynthVecEnv(n_envs, ob, ac, max_episode_steps=max_ep, ac_high=ac_high, seed=loop_seed,
                              device=self.device)
        self.env = env
        self.n_envs = E = env.n
        self.T = 1 if E == 1 else max(1, -(-self.batch_size // E))
        self.stats_logger = StatsLogger()
        self.iteration = 0
        self.loop_seed, self._ctr = int(loop_seed), 0
        self._key_policy = stream_key(loop_seed, "policy")
        self._ep_ret = torch.zeros(E, device=self.device)
        self._ret_sums = torch.zeros(2, dtype=torch.float64, device=self.device)
        self._obs = None
        return ac_high, max_ep, max(self.T * E, self.batch_size + (max_ep or 1000) if E == 1 else 0)

    @property
    def kl_div_updates_counter(self):  # ppo.py:91, 192, on_policy.py:216 (epochs + 1 per update_actor(_acm))
        return self.nets.kl_div_updates_counter

    @kl_div_updates_counter.setter
    def kl_div_updates_counter(self, v):  # ppo.py:226 resets it after logging
        self.nets.kl_div_updates_counter = int(v)

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

    def _mean_return(self, sync):
        """perform_iteration's result: the mean return of the episodes completed (None if none, or unsynchronised)."""
        if not sync:
            return None
        s = self._ret_sums.cpu().numpy()
        return float(s[0] / s[1]) if s[1] > 0 else None

    # ---------------------------------------------------------------- A2C.collect_batch
    def _start(self):
        self._obs = self.env.reset()
        self._ep_ret.zero_()
        self._ep_len = np.zeros(self.n_envs, np.int64)

    def _run_on(self):
        """The envs run on from the last iteration: nothing starts, so nothing is recorded."""

    def collect_batch(self):
        """Rollout memory, time-major [T][E] (_memory), of the steps ``_step`` returns."""
        E = self.n_envs
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
                self._run_on()
            flat = [self._step()[:-1] for _ in range(self.T)]
        return self._memory(flat)

    def _memory(self, flat):
        T, E = len(flat), self.n_envs
        cat = lambda k: torch.stack([f[k] for f in flat])  # noqa: E731
        mem = {"obs": cat(0), "act": cat(1), "lp": cat(2), "rew": cat(3), "done": cat(4), "end": cat(5),
               "next_obs": cat(6), "T": T}
        if E > 1:
            mem["end"][-1].fill_(1)  # segment truncation: GAE bootstraps from V(s') (ppo.py:136-148)
        self.stats_logger.frames += T * E
        return mem

    def _account(self, nobs, rew, end, end_dev):
        """The bookkeeping of one env step.  Returns the tail every class's step tuple ends with -- (reward, done,
        end, next obs, whether a 1-env episode ended), copies the env no longer owns -- and whether ended envs of a
        vectorized env were reset (``_obs`` then holds their first observations)."""
        E = self.n_envs
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
        tail = (rew.clone(), done, end_dev.clone(), nobs.clone(), any_end if E == 1 else False)
        self._obs = nobs
        reset = any_end and E > 1
        if reset:
            self.stats_logger.rollouts += int(end.sum())
            self._obs = self.env.reset(end)
        return tail, reset

    # ---------------------------------------------------------------- test (a2c.py:325-350)
    def test(self, episodes=None):
        episodes = episodes or self.test_episodes or 1
        env = self.env.spawn(episodes, seed=self.loop_seed + 99991)
        obs = env.reset()
        ret = torch.zeros(episodes, device=self.device)
        sums = torch.zeros(2, dtype=torch.float64, device=self.device)
        alive = np.ones(episodes, bool)
        while alive.any():
            obs, rew, end, _ = env.step(self._test_action(obs))
            m = torch.as_tensor((end & alive).astype(np.uint8), device=self.device)
            call("sppEpisodeAccum", ptr(rew), ptr(m), episodes, ptr(ret), ptr(sums), stream_handle())
            alive &= ~end
            if end.any() and alive.any():
                obs = env.reset(end)
        s = sums.cpu().numpy()
        return float(s[0] / s[1])

    # ---------------------------------------------------------------- checkpoints (rl.py:263-301)
    def _nets_state(self):
        return {k: nets.state_dict(p, lay) for k, p, lay in zip(("actor", "critic"), self.nets.params,
                                                                self.nets.layouts)}

    def _load_nets(self, d):
        for k, p, lay in zip(("actor", "critic"), self.nets.params, self.nets.layouts):
            nets.load_state(p, lay, d[k])

    def save(self, path):  # rl.py:281-292
        save_params(path, self.collect_params_dict())

    def load(self, path):  # rl.py:294-301
        self.apply_params_dict(load_params(path))
