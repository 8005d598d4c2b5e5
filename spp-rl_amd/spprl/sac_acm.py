"""SAC_AcM agent: rltoolkit's SPP-SAC update path on the MI355X library.

Mirrors rltoolkit/acm/off_policy/sac_acm.py (reference @ v0) and the pieces of
its MRO that shape the update (SAC sac.py:16-110, DDPG ddpg.py:18-130,
AcMTrainer acm.py:15-183, AcMOffPolicy off_policy.py:8-47):
  - constructor kwargs and defaults (quirks kept: Q1 tau/act_noise are the
    config values whatever is passed; Q4 target entropy = -env ac_dim)
  - ``update(obs, next_obs, action, reward, done, acm_action)``  (sac_acm.py:89-162)
  - ``loss`` dict, ``alpha``, ``collect_params_dict`` / ``apply_params_dict`` /
    ``save`` / ``load`` (rl.py:263-301, sac.py:287-309, ddpg_acm.py:87-94)
Parameters, Adam moments, log_alpha and the normaliser stay on the GPU; the
update never synchronises the host (losses are read lazily).
"""
import ctypes
import math

import torch

from . import _lib, config, nets
from ._lib import call, ptr, stream_handle
from .offpolicy import NORMALIZER, OffPolicyAgent


class SAC_AcM(OffPolicyAgent):
    ALGO = _lib.SPP_ALGO_SAC_ACM
    TRAINABLE = (_lib.SPP_NET_CRITIC1, _lib.SPP_NET_CRITIC2, _lib.SPP_NET_ACTOR, _lib.SPP_NET_ACM)
    TARGETS = {_lib.SPP_NET_CRITIC1_TARG: _lib.SPP_NET_CRITIC1, _lib.SPP_NET_CRITIC2_TARG: _lib.SPP_NET_CRITIC2}
    # key order of the reference's dict (sac.py:287-296 + acm/off_policy/sac_acm.py collect_params_dict)
    CHECKPOINT = (("actor", _lib.SPP_NET_ACTOR), ("critic_1", _lib.SPP_NET_CRITIC1),
                  ("critic_2", _lib.SPP_NET_CRITIC2), (NORMALIZER, None), ("acm", _lib.SPP_NET_ACM))

    def __init__(self, env_name="Hopper-v2", gamma=config.GAMMA, actor_lr=config.DDPG_LR,
                 critic_lr=config.DDPG_LR, alpha_lr=config.ALPHA_LR, alpha=config.ALPHA, tau=config.TAU,
                 act_noise=0.0, update_batch_size=config.UPDATE_BATCH_SIZE, buffer_size=config.BUFFER_SIZE,
                 acm_lr=config.ACM_LR, acm_critic=config.ACM_CRITIC, custom_loss=0.0, norm_closs=config.NORM_CLOSS,
                 min_max_denormalize=config.MIN_MAX_DENORMALIZE, denormalize_actor_out=config.DENORMALIZE_ACTOR_OUT,
                 acm_ob_idx=None, obs_norm=config.OBS_NORM, max_batch=None, device="cuda", env_spec=None,
                 seed=None, mlp_bf16=False, unbiased_update=False, **loop_kw):
        self._check_kwargs(loop_kw)
        _lib.load()
        self.gamma, self.actor_lr, self.critic_lr, self.alpha_lr, self.acm_lr = gamma, actor_lr, critic_lr, alpha_lr, acm_lr
        self.tau = config.TAU  # Q1: SAC consumes `tau` (sac.py:21) -> DDPG default
        self.act_noise = config.ACT_NOISE  # Q1: likewise (ddpg.py:29,100)
        self.acm_critic, self.custom_loss, self.norm_closs = bool(acm_critic), float(custom_loss), bool(norm_closs)
        self.unbiased_update = bool(unbiased_update)  # DDPG_AcM.make_update (ddpg_acm.py:59-79), inherited
        self.min_max_denormalize, self.denormalize_actor_out = bool(min_max_denormalize), bool(denormalize_actor_out)
        self.mlp_bf16 = bool(mlp_bf16)  # bf16 MFMA MLP layers, fp32 everything else (BASELINE configs[4])
        self._init_spaces(env_name, env_spec, device, acm_ob_idx, update_batch_size, max_batch, loop_kw)
        self.target_entropy = -float(self.ac_dim)  # Q4 (sac.py:104-106)
        self.alpha = alpha
        self._create(seed)
        self.alpha_state = torch.tensor([math.log(alpha), 0.0, 0.0, alpha], dtype=torch.float64, device=self.device)
        self.alpha_f32 = torch.tensor([alpha], dtype=torch.float32, device=self.device)
        call("sppAgentBindAlpha", self._h, ptr(self.alpha_state), ptr(self.alpha_f32))
        call("sppAgentBindAlphaGrad", self._h, ptr(self.alpha_grad))
        self._bind_replay(buffer_size, obs_norm, int(loop_kw.get("n_envs", 1)))
        self._init_loop(update_batch_size=update_batch_size, **loop_kw)

    def _net_layouts(self):
        ob, cin = self.ob_dim, self._critic_in()
        return {_lib.SPP_NET_ACTOR: nets.sac_actor_layout(ob, self.actor_output_dim),
                _lib.SPP_NET_CRITIC1: nets.critic_layout(cin), _lib.SPP_NET_CRITIC2: nets.critic_layout(cin),
                _lib.SPP_NET_CRITIC1_TARG: nets.critic_layout(cin), _lib.SPP_NET_CRITIC2_TARG: nets.critic_layout(cin),
                _lib.SPP_NET_ACM: nets.acm_layout(2 * ob, self.ac_dim)}

    def _alloc_grads(self):
        # gradient buckets = the data-parallel exchange units (one all-reduce each):
        #   critic: [critic_1 | critic_2], actor: [actor | d alpha operand], acm: [acm]
        c1, c2, na, nm = (self.params[net].numel() for net in self.TRAINABLE)
        self.bucket_critic = torch.zeros(c1 + c2, device=self.device)
        self.bucket_actor = torch.zeros(na + 1, device=self.device)
        self.bucket_acm = torch.zeros(nm, device=self.device)
        self.grads = {_lib.SPP_NET_CRITIC1: self.bucket_critic[:c1], _lib.SPP_NET_CRITIC2: self.bucket_critic[c1:],
                      _lib.SPP_NET_ACTOR: self.bucket_actor[:na], _lib.SPP_NET_ACM: self.bucket_acm}
        self.alpha_grad = self.bucket_actor[na:]

    def set_steps(self, actor=0, critic=0, alpha=0, acm=0):
        call("sppAgentSetSteps", self._h, actor, critic, alpha, acm)

    # ------------------------------------------------------------------ update
    def update(self, obs, next_obs, action, reward, done, acm_action, eps_next=None, eps_cur=None):
        """SAC_AcM.update (sac_acm.py:89-162).  eps_* are the rsample draws (sac_acm.py:44, :137);
        when omitted they are drawn from torch's generator on the device."""
        b, keep = self._batch(obs, next_obs, action, reward, done, acm_action)
        shape = (b.B, self.actor_output_dim)
        e1 = torch.as_tensor(eps_next, dtype=torch.float32).to(self.device).contiguous() if eps_next is not None \
            else torch.randn(shape, device=self.device)
        e2 = torch.as_tensor(eps_cur, dtype=torch.float32).to(self.device).contiguous() if eps_cur is not None \
            else torch.randn(shape, device=self.device)
        call("sppSacAcmUpdate", self._h, ctypes.byref(b), ptr(e1), ptr(e2), ptr(self._losses), stream_handle())
        self._keep = (keep, e1, e2)  # inputs must outlive the async work

    def update_from_replay(self, idx, seed, counter):
        """Fused path: gather the sampled transitions on device and update with device eps."""
        idx = torch.as_tensor(idx, dtype=torch.int64).to(self.device).contiguous()
        self._stage(idx)
        call("sppSacAcmUpdateStaged", self._h, seed, counter, ptr(self._losses), stream_handle())

    def update_from_replay_dp(self, idx, seed, counter, allreduce=None, beside=None):
        """The same grad step split at its exchange points: allreduce(bucket) averages a
        flat gradient bucket across data-parallel ranks (RCCL) between grads and apply.  beside()
        enqueues independent work (the ACM step's gradients) under the actor bucket's exchange."""
        st = stream_handle()
        self._stage(idx)
        call("sppSacAcmDrawEps", self._h, seed, counter, st)
        call("sppSacAcmCriticGrads", self._h, None, None, ptr(self._losses), st)
        if allreduce is not None:
            allreduce(self.bucket_critic)
        call("sppSacAcmCriticApply", self._h, st)
        call("sppSacAcmActorGrads", self._h, None, ptr(self._losses), st)
        self._exchange(allreduce, self.bucket_actor, beside)
        call("sppSacAcmActorApply", self._h, ptr(self._losses), st)

    def _fused_update(self, idx, counter, allreduce=None, beside=None):
        self.update_from_replay_dp(idx, self._key_update, counter, allreduce, beside)

    def acm_update_from_replay(self, idx, x, y, loss, allreduce=None):
        """update_acm_batches body (acm.py:356-372) for one device-sampled batch."""
        st = stream_handle()
        B = idx.numel()
        call("sppReplayGatherAcm", self.replay_buffer._h, ptr(idx), B, ptr(x), ptr(y), st)
        call("sppAcmRegressGrads", self._h, ptr(x), ptr(y), B, ptr(loss), st)
        if allreduce is not None:
            allreduce(self.bucket_acm)
        call("sppAcmRegressApply", self._h, st)

    @property
    def loss(self):
        v = self._losses.detach().cpu().numpy()
        out = {"critic_1": float(v[0]), "critic_2": float(v[1]), "actor": float(v[2])}
        if self.custom_loss:
            out["sac"], out["dist"] = float(v[3]), float(v[4])
        return out

    @property
    def log_alpha(self):
        return float(self.alpha_state[0].item())

    def current_alpha(self):
        return float(self.alpha_state[3].item())
