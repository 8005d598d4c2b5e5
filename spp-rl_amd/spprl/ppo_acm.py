"""PPO_AcM: rltoolkit's SPP-PPO loop on the MI355X library, vectorized over E envs.

Mirrors rltoolkit/acm/on_policy.py (AcMOnPolicyTrainer / A2C_AcM / PPO_AcM) with
A2C (algorithms/a2c/a2c.py) and PPO (algorithms/ppo/ppo.py) underneath:

  collect_batch         a2c.py:144-184 + on_policy.py:32-50 (process_action: denormalise ->
                        AcM -> env), SURVEY.md §8a row a21
  update_critic         a2c.py:186-225 (critic_num_target_updates x num_critic_updates_per_target
                        full-batch steps), row a22
  calculate_gae         ppo.py:117-150 (device scan over [T][E] streams), row a23
  update_actor_acm      on_policy.py:164-216 + advantage_dataset.py:30-42 (clip loss, entropy,
                        custom dist loss on the buffer's (denormalised) actions, KL early stop), row a24
  update_acm(_batches)  acm.py:266-303, 356-372 every acm_update_freq iterations
  update_obs_mean_std   on the ACM ring when denormalize_actor_out (on_policy.py:70-71)
  pre_train             acm.py:234-244

Device pieces: actor / critic = ``OnPolicyNets`` (libspprl sppOnp*), GAE = sppGaeScan, the AcM
(64-32 tanh, basic_model.py:108-132) and its replay ring = the AcM half of an SPP agent handle
(sppPolicyAct mode 3 for the act, sppAcmRegress* for the regression, BufferAcMOffPolicy for the
ring).  Rollout memory is time-major [T][E] on device.

Vectorization: each iteration collects T = ceil(batch_size / E) steps of E lockstep envs
(N = T*E transitions); envs keep running across iterations and the last step of every
iteration is a truncation (end = 1, done = 0), so GAE bootstraps from V(s') there exactly as
the reference does at a time-limit end.  With E = 1 whole episodes are collected until
batch_size frames, as the reference does.  That scheme, train, the per-step bookkeeping, test and
save / load are OnPolicyLoop's (onpolicy_loop.py), shared with vanilla PPO; this class states its act
call, its ring writes, the side stream, the data-parallel paths and its update.
"""
import os

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, config
from ._lib import call, ptr, stream_handle
from .dp import make_allreduce
from .onpolicy import OnPolicyNets
from .onpolicy_loop import OnPolicyLoop
from .ppo import calculate_gae
from .sac_acm import SAC_AcM


class PPO_AcM(OnPolicyLoop):
    def __init__(self, env_name="HalfCheetah-v2", gamma=0.99, actor_lr=3e-4, critic_lr=3e-4, batch_size=2000,
                 ppo_batch_size=512, kl_div_threshold=0.1, max_ppo_epochs=10, entropy_coef=0.0, ppo_epsilon=0.2,
                 gae_lambda=0.95, critic_num_target_updates=10, num_critic_updates_per_target=10, normalize_adv=True,
                 custom_loss=0.1, norm_closs=config.NORM_CLOSS, min_max_denormalize=True, denormalize_actor_out=True,
                 acm_epochs=5, acm_batch_size=64, acm_update_freq=3, acm_lr=3e-4, acm_update_batches=None,
                 acm_pre_train_samples=100_000, acm_pre_train_epochs=5, acm_scheduler_step=config.ACM_SCHEDULER_STEP,
                 acm_scheduler_gamma=config.ACM_SCHEDULER_GAMMA, acm_keep_pretrain=True, acm_ring_size=None,
                 iterations=1001,
                 stats_freq=1, test_episodes=None, return_done=None, max_frames=None, n_envs=1, env=None,
                 env_spec=None, device="cuda", seed=None, loop_seed=0, epsilon=None, obs_norm=False,
                 rehearse_world=None, dp_update=None, comm=None, acm_ob_idx=None, **unused):
        # unknown keywords raise (the reference's MetaLearner takes no **kwargs, rl.py:17-26); `epsilon` is the
        # reference's name of the clip range (PPO.__init__, ppo.py:17), ppo_epsilon this class's older one
        config.check_kwargs("PPO_AcM", unused, config.ON_POLICY_NO_EFFECT_KWARGS)
        # obs_norm only sets ReplayBufferAcM.obs_norm (acm.py:127-139), read by the ring's normalize() and
        # _sample_batch (replay_buffer.py:77-81, 246-249), neither of which the on-policy loop calls: the rollout
        # normalises through its own Memory (a2c.py:165, on_policy.py:107-112) and the ACM trains on raw ring rows
        # (acm.py:273-282, replay_buffer.py:404-430).  Accepted; it changes nothing computed.
        self.obs_norm = bool(obs_norm)
        if epsilon is not None:
            ppo_epsilon = epsilon
        ac_high, max_ep, Nmax = self._init_loop(env_name, env_spec, device, gamma, gae_lambda, batch_size, iterations,
                                                stats_freq, test_episodes, return_done, max_frames, n_envs, env,
                                                loop_seed)
        ob, ac, env, E = self.ob_dim, self.ac_dim, self.env, self.n_envs
        self.custom_loss, self.norm_closs = float(custom_loss), bool(norm_closs)
        self.min_max_denormalize, self.denormalize_actor_out = bool(min_max_denormalize), bool(denormalize_actor_out)
        self.acm_epochs, self.acm_update_freq, self.acm_update_batches = int(acm_epochs), acm_update_freq, \
            acm_update_batches
        self.actor_output_dim = ob
        lim = 1.0 if self.min_max_denormalize else float(config.MAX_ABS_OBS_VALUE)  # acm.py:102-108
        dp_world = dist.get_world_size() if make_allreduce() is not None else 1  # (the union: world x N rows)
        # rehearse_world = W (measurement only, one process): update(mem) runs on this rank's rollout tiled W
        # times -- the shape, and so the per-rank work, of a W-rank job's union batch -- with no collective
        self.rehearse_world = int(rehearse_world or 0)
        dp_world = max(dp_world, self.rehearse_world)
        # data parallel update (dp_update): "shard" -- each rank updates on its own rollout with one gradient
        # all-reduce per critic / actor step (the reference's per-step losses are batch means, so equal shards
        # average to the union's gradient); "union" -- one all-gather of the rollouts per iteration and every rank
        # runs the whole update on the union (no per-step exchange, replicas equal one process on the union)
        self.dp_update =dp_update or os.environ.get("SPP_PPO_DP_UPDATE", "shard")
        if self.dp_update not in ("shard", "union"):
            raise ValueError("dp_update must be 'shard' or 'union', got %r" % (self.dp_update,))
        self.nets = OnPolicyNets(ob, ob, ac_lim=lim, actor_lr=actor_lr, critic_lr=critic_lr, ppo_epsilon=ppo_epsilon,
                                 entropy_coef=entropy_coef, gamma=gamma, gae_lambda=gae_lambda,
                                 critic_num_target_updates=critic_num_target_updates,
                                 num_critic_updates_per_target=num_critic_updates_per_target,
                                 max_ppo_epochs=max_ppo_epochs, ppo_batch_size=ppo_batch_size,
                                 kl_div_threshold=kl_div_threshold, normalize_adv=normalize_adv,
                                 max_batch=max((dp_world if self.dp_update == "union" else 1) * Nmax,
                                               ppo_batch_size),
                                 device=self.device, seed=seed, custom_loss=custom_loss)
        # the AcM and its replay ring (acm.py:127-141: size = pre-train samples * 1.1)
        ring = int(acm_ring_size or acm_pre_train_samples * 1.1)
        self.acm = SAC_AcM(env_name=env_name, env_spec=(ob, ac, ac_high, max_ep), acm_lr=acm_lr, buffer_size=ring,
                           max_batch=max(acm_batch_size, 64), min_max_denormalize=min_max_denormalize,
                           denormalize_actor_out=denormalize_actor_out, device=self.device, seed=seed, env=env,
                           acm_epochs=acm_epochs, acm_batch_size=acm_batch_size, acm_update_freq=1,
                           acm_update_batches=acm_update_batches, acm_pre_train_samples=acm_pre_train_samples,
                           acm_pre_train_epochs=acm_pre_train_epochs, acm_scheduler_step=acm_scheduler_step,
                           acm_scheduler_gamma=acm_scheduler_gamma, acm_keep_pretrain=acm_keep_pretrain,
                           acm_ob_idx=acm_ob_idx, loop_seed=loop_seed + 17)
        self.replay_buffer = self.acm.replay_buffer
        # Data parallel: the ACM ring is REPLICATED (every rank writes every rank's transitions, in rank
        # order, at the end of each iteration: ReplayBufferAcM.add_buffer, replay_buffer.py:284-297), so the
        # ACM epochs (acm.py:266-303) run on identical rings with one permutation stream and need no
        # per-batch collective, and the ring's obs statistics are global without a collective either.
        # Data parallel (self.dp: a process group with more than one rank, or SPP_DP_FORCE=1's one-rank rehearsal):
        # the on-policy batch is REPLICATED too -- one all-gather of the ranks' rollouts per iteration, the union
        # ordered rank-major along the env axis ([T][world * E]) -- and every rank runs update(mem) (critic
        # targets, GAE, the persistent sppOnpCriticSteps / sppOnpActorEpoch launches) on the identical union with
        # one permutation stream: no per-step gradient exchange, replicas bit-identical, and the result is one
        # process's update on the union batch (acm/on_policy.py:72-75, a2c.py:186-225, ppo.py:152-192)
        self.dp = self.nets.allreduce is not None or self.rehearse_world > 1
        self.world = dist.get_world_size() if self.nets.allreduce is not None else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        if self.dp_update == "union":
            self.nets.allreduce = self.nets.allreduce_sum = None  # (the nets see the union: no per-step exchange)
            self.nets.world = self.nets.shards = 1
        else:
            if comm is not None and self.nets.allreduce is not None:  # the per-step exchange on the compute stream
                inv = 1.0 / comm.world

                def allreduce(t):
                    comm.allreduce_sum(t)
                    t.mul_(inv)

                self.nets.allreduce, self.nets.allreduce_sum = allreduce, comm.allreduce_sum
            # the global minibatch ppo_batch_size is split over the ranks (a rehearsal: over rehearse_world)
            self.nets.shards = max(self.world, self.rehearse_world)
        if self.world > 1 and E == 1:
            # one env per rank collects whole episodes: the ranks' ring-write records ("start" per episode)
            # then differ in count and kind, which the rank-major all-gather of _flush_ring cannot carry
            raise ValueError("PPO_AcM data parallel needs n_envs > 1 per rank (vectorized lockstep envs); "
                             "got n_envs = 1 with world = %d" % self.world)
        if self.dp:  # the replicated ring needs no gradient or statistics exchange either
            self.acm.allreduce = self.acm.allreduce_sum = self.acm.host_sum = None
        self.acm._perm_seed = int(seed or 0) * 7919 + 17  # rank-independent epoch permutations
        self._ring_log = []  # this iteration's ring writes (applied by _flush_ring)
        self._prev_all = None  # per rank: the ring slot of each env's last obs
        self.loss = {}

    # ---------------------------------------------------------------- helpers
    def _randn(self, t):
        self._ctr += 1
        call("sppRandNormal", ptr(t), t.numel(), self._key_policy, self._ctr, stream_handle())
        return t

    def normalize(self, x):
        """MemoryAcM.normalize with the ring's statistics (memory.py:76-88)."""
        rb = self.replay_buffer
        if self.min_max_denormalize and not rb._have_minmax:
            return x.clone()  # the caller keeps it: never alias the env's double-buffered obs
        return rb._norm(x, 0)

    def denormalize(self, x):
        return self.replay_buffer._norm(x, 1)

    def process_action(self, action, norm_obs):
        """on_policy.py:32-50: denormalise (if denormalize_actor_out) -> AcM(cat(obs, a)) -> env action."""
        _, env_act = self.acm.act(norm_obs, eps=action, mode=3)
        return env_act

    # ---------------------------------------------------------------- RL.train / perform_iteration
    def pre_train(self):
        """acm.py:234-244.  Data parallel: the random-action samples of every rank go into every rank's
        ring (replicated, as the iteration's writes), then the same epochs run on every rank."""
        if self.world == 1:
            self.acm.pre_train()
            self._obs = None
            return
        acm, E = self.acm, self.n_envs
        obs = self.env.reset()
        self._ring_log.append(("start", obs.clone()))
        act = torch.empty(E, self.ac_dim, device=self.device)
        collected = 0
        while collected < acm.acm_pre_train_samples:  # AcMOffPolicy.collect_samples (off_policy.py:56-87)
            self.env.sample_actions(act)
            nobs, rew, end, end_dev = self.env.step(act)
            mask, robs = None, None
            if end.any():
                obs = self.env.reset(end)
                mask, robs = end.copy(), obs.clone()
            # the buffer's action slot holds the next obs; time-limit ends are kept as done
            self._ring_log.append(("step", nobs.clone(), rew.clone(), end_dev.clone(), end_dev.clone(), act.clone(),
                                   mask, robs))
            collected += E
        self._flush_ring()
        acm.update_acm(epochs=acm.acm_pre_train_epochs, pretrain=True)
        acm.update_obs_stats()
        if not acm.acm_keep_pretrain:
            self.replay_buffer.reset_idx()
        self._obs = None

    def perform_iteration(self, sync=True):
        """on_policy.py:52-75.  Returns the mean return of the episodes completed (None if none).

        update(mem) (critic, GAE, actor) and update_acm touch disjoint networks and data: the ACM trains on
        the ring, already flushed by collect_batch, and nothing in update(mem) reads the ACM.  A single-process
        run therefore enqueues the ACM epochs on a side stream first and runs update(mem) beside them (the
        persistent critic / actor grids leave the ACM grid's workgroup slots free); the obs statistics and the
        next rollout wait for both, as in the reference's order.  The results are the serial order's."""
        self._ret_sums.zero_()
        mem = self.collect_batch()
        if self.dp and self.dp_update == "union":
            mem = self._union(mem)  # every rank's rollout, before the ACM's side stream starts
        acm_now = bool(self.acm_update_freq) and self.iteration % self.acm_update_freq == 0
        side = self._acm_side_stream() if acm_now else None
        if side is not None:
            ready = torch.cuda.Event()
            ready.record()
            side.wait_event(ready)
            self.nets.reserve_workgroups(self.acm.acm_sgd_workgroups())
            with torch.cuda.stream(side):
                self._update_acm()
            done = torch.cuda.Event()
            done.record(side)
            try:
                self.update(mem)
            finally:
                torch.cuda.current_stream().wait_event(done)
                self.nets.reserve_workgroups(0)
        else:
            self.update(mem)
            if acm_now:
                self._update_acm()
        if self.denormalize_actor_out:
            self.acm.update_obs_stats()
        return self._mean_return(sync)

    def _update_acm(self):
        if self.acm_update_batches:
            self.acm.update_acm_batches(self.acm_update_batches)
        else:
            self.acm.update_acm(self.acm_epochs)

    def _acm_side_stream(self):
        """The side stream of the concurrent ACM update, or None: CUDA device, persistent ACM SGD eligible (one
        launch per epoch), and the env var SPP_PPO_ACM_OVERLAP not 0.  Data parallel too: the iteration's
        collectives (the ring flush, the rollout union) are all issued before the side stream starts, and the
        ACM epochs themselves exchange nothing (replicated ring)."""
        if os.environ.get("SPP_PPO_ACM_OVERLAP", "1") == "0" or self.device.type != "cuda":
            return None
        if not self.acm._acm_sgd_ok(self.acm.acm_batch_size):
            return None
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.device)
        return self._side

    # ---------------------------------------------------------------- A2C.collect_batch
    def _start(self):
        super()._start()
        self._ring_log.append(("start", self._obs.clone()))

    # ---------------------------------------------------------------- the ACM ring (add_buffer)
    def _flush_ring(self):
        """Apply the iteration's ring writes (ReplayBufferAcM.add_buffer at the iteration's end,
        replay_buffer.py:284-297): locally, or -- data parallel -- every rank's writes in rank order
        after one all-gather of the iteration's records, so every rank holds the same ring."""
        log, self._ring_log = self._ring_log, []
        if not log:
            return
        E, ob, ac = self.n_envs, self.ob_dim, self.ac_dim
        W = self.world
        R = self.rehearse_world if W == 1 and self.rehearse_world > 1 else 1
        if self._prev_all is None:
            self._prev_all = [None] * max(W, R)
        if W == 1:
            # (a rehearsal of R ranks: the replicated ring takes R ranks' writes per iteration -- this rank's R times)
            blocks = [log] * R
        else:
            F = 2 * ob + ac + 4  # obs | rew | done | end | env action | reset obs | reset mask
            buf = torch.zeros(len(log), E, F, device=self.device)
            for i, rec in enumerate(log):
                if rec[0] == "start":
                    buf[i, :, :ob] = rec[1]
                else:
                    _, nobs, rew, done, end, act, mask, robs = rec
                    buf[i, :, :ob] = nobs
                    buf[i, :, ob] = rew
                    buf[i, :, ob + 1] = done.float()
                    buf[i, :, ob + 2] = end.float()
                    buf[i, :, ob + 3:ob + 3 + ac] = act
                    if mask is not None:
                        buf[i, :, ob + 3 + ac:2 * ob + 3 + ac] = robs
                        buf[i, :, 2 * ob + 3 + ac] = torch.from_numpy(mask.astype(np.float32)).to(self.device)
            allb = torch.empty(W * buf.shape[0], *buf.shape[1:], device=self.device)
            dist.all_gather_into_tensor(allb, buf)  # rank-major along dim 0
            allb = allb.view(W, *buf.shape)
            masks = allb[:, :, :, 2 * ob + 3 + ac].cpu().numpy() > 0.5  # one host copy for every rank's masks
            blocks = []
            for r in range(W):
                recs = []
                for i, rec in enumerate(log):
                    b = allb[r, i]
                    if rec[0] == "start":
                        recs.append(("start", b[:, :ob]))
                    else:
                        m = masks[r, i]
                        recs.append(("step", b[:, :ob], b[:, ob], b[:, ob + 1].to(torch.uint8),
                                     b[:, ob + 2].to(torch.uint8), b[:, ob + 3:ob + 3 + ac],
                                     m if m.any() else None, b[:, ob + 3 + ac:2 * ob + 3 + ac]))
                blocks.append(recs)
        rb = self.replay_buffer
        for r, recs in enumerate(blocks):
            prev = self._prev_all[r]
            for rec in recs:
                if rec[0] == "start":
                    prev = rb.add_obs_batch(rec[1])
                    continue
                _, nobs, rew, done, end, act, mask, robs = rec
                slots = rb.add_obs_batch(nobs)
                rb.add_timestep_batch(prev, slots, nobs, rew, done, end, act)  # ReplayBufferAcM ring
                prev = slots
                if mask is not None:
                    idx = np.flatnonzero(mask)
                    rs = rb.add_obs_batch(robs[torch.as_tensor(idx, device=self.device)])
                    prev = prev.copy()
                    prev[idx] = rs
            self._prev_all[r] = prev

    def _memory(self, flat):
        """Rollout memory, time-major [T][E]: normalised obs, actions, log-probs, rewards, done,
        end, next obs (raw).  The iteration's ring writes are applied first."""
        self._flush_ring()
        return super()._memory(flat)

    def _step(self):
        norm_obs = self.normalize(self._obs)
        eps = self._randn(torch.empty(self.n_envs, self.actor_output_dim, device=self.device))
        act, lp = self.nets.act(norm_obs, eps)
        env_act = self.process_action(act, norm_obs)
        nobs, rew, end, end_dev = self.env.step(env_act)
        tail, reset = self._account(nobs, rew, end, end_dev)
        mask, robs = (end.copy(), self._obs.clone()) if reset else (None, None)
        # ring writes of this step (applied at the iteration's end, _flush_ring)
        self._ring_log.append(("step", tail[3], tail[0], tail[1], tail[2], env_act.clone(), mask, robs))
        return (norm_obs, act, lp) + tail

    # ---------------------------------------------------------------- data parallel: the rollout union
    def _union(self, mem):
        """All-gather the ranks' rollouts [T][E] into the union [T][world * E] (rank-major along the env axis),
        in one collective of one packed tensor: normalised obs | action | log-prob | reward | done | end | next
        obs.  Every rank then holds the same batch."""
        if mem.get("union"):
            return mem
        T, E, ob, W = mem["T"], self.n_envs, self.ob_dim, self.world
        if self.rehearse_world > 1:  # (measurement: a W-rank union's shape from this rank's rollout)
            R = self.rehearse_world
            tile = lambda x: x.repeat(1, R, *([1] * (x.dim() - 2)))  # noqa: E731
            out = {k: tile(mem[k]) for k in ("obs", "act", "lp", "rew", "done", "end", "next_obs")}
            out.update(T=T, E=R * E, union=True)
            return out
        F = 3 * ob + 4
        pk = torch.empty(T, E, F, device=self.device)
        pk[:, :, :ob] = mem["obs"]
        pk[:, :, ob:2 * ob] = mem["act"]
        pk[:, :, 2 * ob] = mem["lp"]
        pk[:, :, 2 * ob + 1] = mem["rew"]
        pk[:, :, 2 * ob + 2] = mem["done"].float()
        pk[:, :, 2 * ob + 3] = mem["end"].float()
        pk[:, :, 2 * ob + 4:] = mem["next_obs"]
        allp = torch.empty(W, T, E, F, device=self.device)
        dist.all_gather_into_tensor(allp.view(W * T, E, F), pk.view(T, E, F))
        u = allp.permute(1, 0, 2, 3).reshape(T, W * E, F)  # [T][rank][env] -> [T][rank * E + env]
        return {"obs": u[:, :, :ob], "act": u[:, :, ob:2 * ob], "lp": u[:, :, 2 * ob].contiguous(),
                "rew": u[:, :, 2 * ob + 1].contiguous(), "done": u[:, :, 2 * ob + 2].to(torch.uint8),
                "end": u[:, :, 2 * ob + 3].to(torch.uint8), "next_obs": u[:, :, 2 * ob + 4:], "T": T, "E": W * E,
                "union": True}

    # ---------------------------------------------------------------- update (critic, GAE, actor)
    def _flatten(self, mem):
        """(T, E, N = T * E, obs [N][ob], the raw and the normalised next obs [N][ob], rew [N], done [N] float)."""
        T, E, ob = mem["T"], mem.get("E", self.n_envs), self.ob_dim
        N = T * E
        raw_next = mem["next_obs"].reshape(N, ob).contiguous()
        return (T, E, N, mem["obs"].reshape(N, ob), raw_next, self.normalize(raw_next), mem["rew"].reshape(N),
                mem["done"].reshape(N).float())

    def update(self, mem):
        """critic, GAE, actor on the iteration's batch: this rank's rollout, or (data parallel) the union of every
        rank's (self._union; a caller may pass the union itself)."""
        if self.dp and self.dp_update == "union":
            mem = self._union(mem)
        T, E, N, obs, _, nobs, rew, done = self._flatten(mem)
        self.nets.update_critic(obs, nobs, rew, done)  # a2c.py:186-225
        v = self.nets.value(obs).reshape(T, E)
        v_next = self.nets.value(nobs).reshape(T, E)
        _, adv = calculate_gae(mem["rew"].reshape(T, E), v, v_next, mem["done"].reshape(T, E),
                               mem["end"].reshape(T, E), self.gamma, self.gae_lambda)
        acts = mem["act"].reshape(N, self.ob_dim)
        nxt = nobs
        if not self.norm_closs:  # on_policy.py:191-193
            nxt, acts = self.denormalize(nobs), self.denormalize(acts)
        self.nets.update_actor(adv.reshape(N), obs, acts, mem["lp"].reshape(N), nxt)
        self.loss.update(self.nets.loss)
        self.loss["acm"] = None

    # ---------------------------------------------------------------- test (a2c.py test)
    def _test_action(self, obs):
        n_obs = self.normalize(obs)
        act, _ = self.nets.act(n_obs, None)  # deterministic mean
        return self.process_action(act, n_obs)

    # ---------------------------------------------------------------- checkpoints (rl.py:263-279 + ACM)
    def collect_params_dict(self):
        return {**self._nets_state(), **self.replay_buffer.normalizer_state(),
                "acm": self.acm.net_state(_lib.SPP_NET_ACM)}

    def apply_params_dict(self, d):  # (acm/on_policy.py)
        self._load_nets(d)
        self.acm.load_net(_lib.SPP_NET_ACM, d["acm"])
        self.replay_buffer.load_normalizer_state(d)
