"""What the off-policy agents share: the library handle, the flat networks, acting, the ACM step, checkpoints.

``SAC_AcM`` and ``DDPG_AcM`` declare what tells them apart as class data -- ``ALGO``, ``TRAINABLE``, ``TARGETS``,
``CHECKPOINT`` and the ordered ``_net_layouts()`` -- and keep their own constructor signature, update calls and
``loss``; ``OffPolicyAgent`` turns the data into a bound handle once.  ``Vanilla`` is what the reference's plain SAC
and DDPG change on top of their AcM class: the actor emits the env action, the ring is the plain ReplayBuffer and a
time-limit end is not ``done``.
"""
import ctypes

import numpy as np
import torch

from . import _lib, config, nets
from ._lib import call, ptr, stream_handle
from .replay import BufferAcMOffPolicy, ReplayBuffer
from .trainer import OffPolicyLoop

NORMALIZER = None  # CHECKPOINT key: the place of the replay ring's four normaliser entries in the dict


class OffPolicyAgent(OffPolicyLoop):
    ALGO = None  # SPP_ALGO_* of the handle
    TRAINABLE = ()  # the nets with a gradient and Adam moments
    TARGETS = {}  # target net -> the net it starts as a deep copy of
    CHECKPOINT = ()  # (key, net) in the key order of the reference's dict, (NORMALIZER, None) among them
    IDENTITY_MINMAX = False  # Vanilla: the library runs in min-max mode over an identity pair
    alpha_lr = acm_lr = target_entropy = 0.0  # AgentConfig fields only some classes set
    mlp_bf16 = False

    # ------------------------------------------------------------------ construction
    def _init_spaces(self, env_name, env_spec, device, acm_ob_idx, update_batch_size, max_batch, loop_kw):
        """The env's dims, the actor's output space and the scratch size (after the min_max_denormalize flag)."""
        ob, ac, ac_high, _ = self.env_spec = tuple(env_spec or config.ENV_SPECS[env_name])
        self.env_name, self.ob_dim, self.ac_dim = env_name, ob, ac
        self.device = torch.device(device)
        self.update_batch_size = update_batch_size
        self._acm_cols = config.acm_columns(acm_ob_idx, ob)  # (acm.py:94-99; refuses lists the reference can't run)
        self.acm_ob_idx = list(range(ob)) if acm_ob_idx is None else [int(i) for i in acm_ob_idx]
        self.actor_output_dim, lim = self._actor_space(ac_high)
        self.actor_ac_lim = torch.full((self.actor_output_dim,), lim)
        self.ac_lim = torch.full((ac,), float(ac_high))  # the AcM's limit (unused by BasicAcM: its scale is t1)
        self.max_batch = int(max_batch or config.default_max_batch(update_batch_size, loop_kw))

    def _actor_space(self, ac_high):
        """(actor output dim, its limit), acm.py:102-108: the actor emits the acm_ob_idx columns of an observation."""
        # obs spaces of these envs are unbounded
        return len(self.acm_ob_idx), 1.0 if self.min_max_denormalize else float(config.MAX_ABS_OBS_VALUE)

    def _critic_in(self):
        return self.ob_dim + (self.ac_dim if self.acm_critic else self.actor_output_dim)

    def _create(self, seed):
        """The handle with every net of ``_net_layouts()`` drawn (one generator, in that order), bound and limited."""
        self.layouts = self._net_layouts()
        cfg = _lib.AgentConfig(self.ALGO, self.ob_dim, self.actor_output_dim, self.ac_dim, int(self.acm_critic),
                               int(self.min_max_denormalize or self.IDENTITY_MINMAX), int(self.norm_closs),
                               self.custom_loss, self.gamma, self.tau, self.actor_lr, self.critic_lr, self.alpha_lr,
                               self.acm_lr, self.target_entropy, self.max_batch, int(self.mlp_bf16))
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        h = ctypes.c_void_p()
        call("sppAgentCreate", ctypes.byref(h), ctypes.byref(cfg), dev)
        self._h = h
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        self.params, self.exp_avg, self.exp_avg_sq = {}, {}, {}
        for net, lay in self.layouts.items():
            n = ctypes.c_int64()
            call("sppAgentNetSize", self._h, net, ctypes.byref(n))
            assert n.value == nets.numel(lay), (net, n.value, nets.numel(lay))
            self.params[net] = nets.linear_init_(torch.empty(n.value, device=self.device), lay, gen)
        self._alloc_grads()
        for net in self.TRAINABLE:
            self.exp_avg[net] = torch.zeros_like(self.params[net])
            self.exp_avg_sq[net] = torch.zeros_like(self.params[net])
        # sac.py:127,136, ddpg.py:120-125: the targets start as deep copies (drawn above all the same: the draws
        # of the nets after them must not move)
        for targ, src in self.TARGETS.items():
            self.params[targ].copy_(self.params[src])
        for net in self.layouts:
            call("sppAgentBindNet", self._h, net, ptr(self.params[net]), ptr(self.grads.get(net)),
                 ptr(self.exp_avg.get(net)), ptr(self.exp_avg_sq.get(net)))
        a_lim = self.actor_ac_lim.numpy().astype(np.float32)
        m_lim = self.ac_lim.numpy().astype(np.float32)
        call("sppAgentSetLimits", self._h, a_lim.ctypes.data_as(ctypes.c_void_p), m_lim.ctypes.data_as(ctypes.c_void_p))
        self._losses = torch.zeros(_lib.NUM_LOSSES, device=self.device)

    def _alloc_grads(self):
        """Gradient buckets = the data-parallel exchange units (one all-reduce each): one flat tensor per net."""
        self.grads = {net: torch.zeros_like(self.params[net]) for net in self.TRAINABLE}
        self.bucket_critic, self.bucket_actor = self.grads[_lib.SPP_NET_CRITIC1], self.grads[_lib.SPP_NET_ACTOR]
        self.bucket_acm = self.grads.get(_lib.SPP_NET_ACM)

    def _bind_replay(self, buffer_size, obs_norm, n_envs):
        """The AcM ring, its normaliser bound to the handle."""
        self.replay_buffer = BufferAcMOffPolicy(buffer_size, self.ob_dim, self.actor_output_dim, self.ac_dim,
                                                device=self.device, min_max_denormalize=self.min_max_denormalize,
                                                obs_norm=obs_norm, n_envs=n_envs)
        self.bind_normalizer(self.replay_buffer)
        if self._acm_cols is not None:
            self.replay_buffer.set_acm_columns(self._acm_cols)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib._lib is not None:
            _lib.load().sppAgentDestroy(h)
            self._h = None

    # ------------------------------------------------------------------ wiring
    def bind_normalizer(self, buf, min_obs=None, max_obs=None):
        """The handle reads ``buf``'s statistics in place (min_obs / max_obs: another min-max pair than buf's)."""
        call("sppAgentBindNormalizer", self._h, ptr(buf.min_obs if min_obs is None else min_obs),
             ptr(buf.max_obs if max_obs is None else max_obs), ptr(buf.obs_mean), ptr(buf.obs_std))

    def net_state(self, net):
        return nets.state_dict(self.params[net], self.layouts[net])

    def load_net(self, net, state):
        nets.load_state(self.params[net], self.layouts[net], state)

    def _batch(self, obs, next_obs, action, reward, done, acm_action):
        """update()'s arguments as a library Batch and the device tensors it points into."""
        d = self.device
        t = lambda x, dt=torch.float32: torch.as_tensor(x, dtype=dt).to(d).contiguous()  # noqa: E731
        tens = [t(obs), t(next_obs), t(action) if action is not None else None, t(reward).reshape(-1),
                t(done, torch.int8).reshape(-1), t(acm_action)]
        return _lib.Batch(tens[0].shape[0], *[ptr(x) for x in tens]), tens

    # ------------------------------------------------------------------ ACM regression + acting
    def batch_update_acm(self, x, y):
        """AcMTrainer.batch_update (acm.py:246-258); on the BasicAcM t and t1 are trained too."""
        x = torch.as_tensor(x, dtype=torch.float32).to(self.device).contiguous()
        y = torch.as_tensor(y, dtype=torch.float32).to(self.device).contiguous()
        loss = torch.zeros(1, device=self.device)
        call("sppAcmRegressStep", self._h, ptr(x), ptr(y), x.shape[0], ptr(loss), stream_handle())
        self._keep_acm = (x, y)
        return loss

    def act(self, obs, eps=None, noise=None, mode=1, act_noise=None):
        """noise_action + process_action for E observations (ddpg_acm.py:40-50, off_policy.py:89-106).
        Returns (target_state [E, aout], env_action [E, ac]).
        On a Vanilla class (ddpg.py:171-180, 371-383) mode 1 is noise_action with ``noise`` the N(0, 1) draw, mode 0
        initial_act with ``eps`` the caller's action_space.sample(), mode 2 deterministic, and both results are the
        action: process_action is the identity."""
        obs = torch.as_tensor(obs, dtype=torch.float32).to(self.device).contiguous()
        E = obs.shape[0]
        tgt = torch.empty(E, self.actor_output_dim, device=self.device)
        env = torch.empty(E, self.ac_dim, device=self.device)
        call("sppPolicyAct", self._h, ptr(obs), E, ptr(eps), ptr(noise),
             self.act_noise if act_noise is None else act_noise, mode, int(self.denormalize_actor_out), ptr(tgt),
             ptr(env), stream_handle())
        self._keep_act = (obs, eps, noise)  # inputs must outlive the async work
        return tgt, env

    # ------------------------------------------------------------------ checkpoints (rl.py:263-301)
    def collect_params_dict(self):
        d = {}
        for key, net in self.CHECKPOINT:
            if key is NORMALIZER:
                d.update(self.replay_buffer.normalizer_state())
            else:
                d[key] = self.net_state(net)
        return d

    def apply_params_dict(self, d):
        for key, net in self.CHECKPOINT:
            if key is NORMALIZER:
                self.replay_buffer.load_normalizer_state(d)
            else:
                self.load_net(net, d[key])


class Vanilla:
    """Mixed in before an AcM agent class: the reference's plain algorithm (SAC, DDPG) on that class's device path.
    No ACM anywhere; the critics take cat(obs, action); nothing is denormalised."""
    VANILLA = True
    IDENTITY_MINMAX = True  # with the pair below the kernels' denormalisation of the actor output is exact

    def _init_spaces(self, *a):
        super()._init_spaces(*a)
        self.max_ep_len = int(self.env_spec[3])  # Q3: RL masks the time-limit done (rl.py:185); AcMOffPolicy never

    def _actor_space(self, ac_high):
        return self.ac_dim, float(ac_high)  # the env action: Actor(ob, self.ac_lim, ac) (sac.py:97, ddpg.py:117)

    def _bind_replay(self, buffer_size, obs_norm, n_envs):
        # obs_norm (DDPG.__init__, ddpg.py:101-115): the plain ReplayBuffer normalises sampled obs / next obs
        # (z-score, replay_buffer.py:246-249) and the rollout's act input (ddpg.py:203); its statistics start
        # as zeros / ones (replay_buffer.py:113-115), i.e. only the clip, until the first update_obs_mean_std
        self.replay_buffer = ReplayBuffer(buffer_size, self.ob_dim, self.ac_dim, device=self.device,
                                          obs_norm=bool(obs_norm), n_envs=n_envs)
        # identity denormalisation of the actor output: min-max over [-1, 1] is 0 + x * 1, exact; the z-score
        # pair is the ring's own statistics (the staged batch's obs_norm normalisation, sppAgentStagePost 2)
        self._ident = torch.stack([-torch.ones(self.ob_dim), torch.ones(self.ob_dim)]).to(self.device)
        self.bind_normalizer(self.replay_buffer, self._ident[0], self._ident[1])

    def pre_train(self):
        name = type(self).__name__
        raise AttributeError("vanilla %s has no ACM pre-training (rltoolkit %s defines none)" % (name, name))
