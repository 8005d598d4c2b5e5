"""Vanilla DDPG: rltoolkit/algorithms/ddpg/ddpg.py (train/vanilla_ddpg_hcheetah.py) on the MI355X library.

The baseline of the SPP-DDPG curves.  The update is DDPG_AcM's device path with no ACM: the deterministic
actor (and its target) emit the env action (ac dims, tanh * action high), the critic (and its target) take
cat(obs, action), there is no custom loss and nothing is denormalised.
Kept from the reference:
  - constructor kwargs of DDPG / RL / MetaLearner (ddpg.py:19-33, rl.py:17-26); DDPG forwards ``tau`` and
    ``act_noise`` itself, so both are honoured (quirk Q1 is SAC's)
  - quirk Q3: time-limit ends are not ``done`` (rl.py:185, ddpg.py:210-212)
  - ``update(obs, next_obs, action, reward, done)`` (ddpg.py:286-327): critic step, actor step, polyak of
    both targets; ``loss`` keys {actor, critic}
  - ``noise_action`` / ``initial_act`` / ``process_action`` (ddpg.py:171-180, 371-383) as ``act`` modes 1 / 0 / 2
  - ``collect_params_dict`` keys (ddpg.py:331-339)
"""
import ctypes

import numpy as np
import torch

from . import _lib, config, nets
from ._lib import call, ptr, stream_handle
from .ddpg_acm import DDPG_AcM
from .replay import ReplayBuffer

_ACM_ONLY = ("custom_loss", "norm_closs", "denormalize_actor_out", "unbiased_update", "acm_critic")


class DDPG(DDPG_AcM):
    ALGO = _lib.SPP_ALGO_DDPG
    VANILLA = True

    def __init__(self, env_name="HalfCheetah-v2", gamma=config.GAMMA, actor_lr=config.DDPG_LR,
                 critic_lr=config.DDPG_LR, tau=config.TAU, act_noise=config.ACT_NOISE,
                 update_batch_size=config.UPDATE_BATCH_SIZE, buffer_size=config.BUFFER_SIZE,
                 obs_norm=config.OBS_NORM, max_batch=None, device="cuda", env_spec=None, seed=None, **loop_kw):
        # DDPG -> RL -> MetaLearner (ddpg.py:19-33, rl.py:17-26) take no AcMTrainer / AcMOffPolicy / DDPG_AcM
        # keyword: the reference raises TypeError on them, and so does this class, before the library is touched
        acm_only = sorted(k for k in loop_kw if k.startswith("acm_") or k in _ACM_ONLY)
        if acm_only:
            raise TypeError("DDPG got unexpected keyword argument(s): %s (SPP / AcM options: use DDPG_AcM)"
                            % ", ".join(acm_only))
        loop_kw.pop("min_max_denormalize", None)  # MetaLearner's; without obs_norm it normalises nothing here
        self._check_kwargs(loop_kw)
        loop_kw["acm_epochs"] = 0  # no ACM anywhere
        _lib.load()
        ob, ac, ac_high, max_ep = env_spec or config.ENV_SPECS[env_name]
        self.env_spec = tuple(env_spec or config.ENV_SPECS[env_name])
        self.env_name, self.ob_dim, self.ac_dim = env_name, ob, ac
        self.max_ep_len = int(max_ep)  # Q3: RL masks the time-limit done (rl.py:185)
        self.device = torch.device(device)
        self.gamma, self.actor_lr, self.critic_lr, self.tau = gamma, actor_lr, critic_lr, tau
        self.act_noise = act_noise
        self.update_batch_size = update_batch_size
        self.acm_critic, self.custom_loss, self.norm_closs, self.unbiased_update = False, 0.0, False, False
        self.min_max_denormalize, self.denormalize_actor_out = False, False
        self.actor_output_dim = aout = ac
        self.actor_ac_lim = torch.full((ac,), float(ac_high))  # Actor(ob, self.ac_lim, ac) (ddpg.py:117)
        self.max_batch = int(max_batch or config.default_max_batch(update_batch_size, loop_kw))
        cin = ob + ac
        self.layouts = {_lib.SPP_NET_ACTOR: nets.ddpg_actor_layout(ob, aout),
                        _lib.SPP_NET_ACTOR_TARG: nets.ddpg_actor_layout(ob, aout),
                        _lib.SPP_NET_CRITIC1: nets.critic_layout(cin), _lib.SPP_NET_CRITIC1_TARG: nets.critic_layout(cin)}
        # min-max mode with the identity pair below: the kernels' denormalisation of the actor output is exact
        cfg = _lib.AgentConfig(self.ALGO, ob, aout, ac, 0, 1, 0, 0.0, gamma, tau, actor_lr, critic_lr, 0.0, 0.0, 0.0,
                               self.max_batch)
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        h = ctypes.c_void_p()
        call("sppAgentCreate", ctypes.byref(h), ctypes.byref(cfg), dev)
        self._h = h
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        self.params, self.grads, self.exp_avg, self.exp_avg_sq = {}, {}, {}, {}
        for net, lay in self.layouts.items():
            n = ctypes.c_int64()
            call("sppAgentNetSize", self._h, net, ctypes.byref(n))
            assert n.value == nets.numel(lay), (net, n.value, nets.numel(lay))
            self.params[net] = nets.linear_init_(torch.empty(n.value, device=self.device), lay, gen)
        # gradient buckets (the data-parallel exchange units): [critic], [actor]
        for net in (_lib.SPP_NET_CRITIC1, _lib.SPP_NET_ACTOR):
            n = self.params[net].numel()
            self.grads[net] = torch.zeros(n, device=self.device)
            self.exp_avg[net] = torch.zeros(n, device=self.device)
            self.exp_avg_sq[net] = torch.zeros(n, device=self.device)
        self.bucket_critic, self.bucket_actor = self.grads[_lib.SPP_NET_CRITIC1], self.grads[_lib.SPP_NET_ACTOR]
        self.bucket_acm = None
        # ddpg.py:120-125: targets start as deep copies
        self.params[_lib.SPP_NET_CRITIC1_TARG].copy_(self.params[_lib.SPP_NET_CRITIC1])
        self.params[_lib.SPP_NET_ACTOR_TARG].copy_(self.params[_lib.SPP_NET_ACTOR])
        for net in self.layouts:
            call("sppAgentBindNet", self._h, net, ptr(self.params[net]), ptr(self.grads.get(net)),
                 ptr(self.exp_avg.get(net)), ptr(self.exp_avg_sq.get(net)))
        a_lim = self.actor_ac_lim.numpy().astype(np.float32)
        call("sppAgentSetLimits", self._h, a_lim.ctypes.data_as(ctypes.c_void_p), a_lim.ctypes.data_as(ctypes.c_void_p))
        # obs_norm (ddpg.py:101-115): the plain ReplayBuffer z-scores sampled obs / next obs
        # (replay_buffer.py:246-249) and the rollout's act input (ddpg.py:203)
        self.replay_buffer = ReplayBuffer(buffer_size, ob, ac, device=self.device, obs_norm=bool(obs_norm),
                                          n_envs=int(loop_kw.get("n_envs", 1)))
        # identity denormalisation of the actor output: min-max over [-1, 1] is 0 + x * 1, exact; the z-score
        # pair is the ring's own statistics (the staged batch's normalisation, sppAgentStagePost mode 2)
        self._ident = torch.stack([-torch.ones(ob), torch.ones(ob)]).to(self.device)
        rb = self.replay_buffer
        call("sppAgentBindNormalizer", self._h, ptr(self._ident[0]), ptr(self._ident[1]), ptr(rb.obs_mean),
             ptr(rb.obs_std))
        self._losses = torch.zeros(_lib.NUM_LOSSES, device=self.device)
        self.acm_kind = None
        self._init_loop(update_batch_size=update_batch_size, **loop_kw)

    # ------------------------------------------------------------------ update
    def update(self, obs, next_obs, action, reward, done):
        """DDPG.update (ddpg.py:286-327): 5-tuple batch (ReplayBuffer.sample_batch, replay_buffer.py:233-261)."""
        super().update(obs, next_obs, action, reward, done, action)

    def update_from_replay(self, idx, seed=None, counter=None):
        """The reference cadence's staged grad step (trainer.make_update): gather the sampled transitions on the
        device and update.  DDPG draws no noise in its update: seed / counter are unused."""
        idx = torch.as_tensor(idx, dtype=torch.int64).to(self.device).contiguous()
        self.update_from_replay_dp(idx)
        self._keep_idx_ref = idx

    @property
    def loss(self):
        v = self._losses.detach().cpu().numpy()
        return {"actor": float(v[1]), "critic": float(v[0])}

    # ------------------------------------------------------------------ acting
    def act(self, obs, eps=None, noise=None, mode=1, act_noise=None):
        """mode 1: noise_action (ddpg.py:171-176) with ``noise`` the N(0, 1) draw; mode 0: initial_act, ``eps`` is
        the caller's action_space.sample() (ddpg.py:178-180); mode 2: deterministic.  Returns (action, action):
        process_action is the identity (ddpg.py:371-383)."""
        obs = torch.as_tensor(obs, dtype=torch.float32).to(self.device).contiguous()
        E = obs.shape[0]
        tgt = torch.empty(E, self.ac_dim, device=self.device)
        env = torch.empty(E, self.ac_dim, device=self.device)
        call("sppPolicyAct", self._h, ptr(obs), E, ptr(eps), ptr(noise),
             self.act_noise if act_noise is None else act_noise, mode, 0, ptr(tgt), ptr(env), stream_handle())
        self._keep_act = (obs, eps, noise)
        return tgt, env

    def batch_update_acm(self, x, y):
        raise AttributeError("vanilla DDPG has no ACM (rltoolkit DDPG defines none)")

    def pre_train(self):
        raise AttributeError("vanilla DDPG has no ACM pre-training (rltoolkit DDPG defines none)")

    # ------------------------------------------------------------------ checkpoints (ddpg.py:331-352)
    def collect_params_dict(self):
        rb = self.replay_buffer
        return {"actor": self.net_state(_lib.SPP_NET_ACTOR), "critic": self.net_state(_lib.SPP_NET_CRITIC1),
                "obs_mean": rb.obs_mean.cpu(), "obs_std": rb.obs_std.cpu(),
                "min_obs": rb.min_obs.cpu() if rb._have_minmax else None,
                "max_obs": rb.max_obs.cpu() if rb._have_minmax else None}

    def apply_params_dict(self, d):
        for k, net in (("actor", _lib.SPP_NET_ACTOR), ("critic", _lib.SPP_NET_CRITIC1)):
            self.load_net(net, d[k])
        rb = self.replay_buffer
        rb.obs_mean.copy_(torch.as_tensor(d["obs_mean"]))
        rb.obs_std.copy_(torch.as_tensor(d["obs_std"]))
        if d.get("min_obs") is not None and d.get("max_obs") is not None:
            rb.min_obs.copy_(torch.as_tensor(d["min_obs"]))
            rb.max_obs.copy_(torch.as_tensor(d["max_obs"]))
            rb._have_minmax = True
