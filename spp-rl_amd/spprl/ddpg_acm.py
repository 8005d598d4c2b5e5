"""DDPG_AcM agent: rltoolkit's SPP-DDPG update path on the MI355X library.

Mirrors rltoolkit/acm/off_policy/ddpg_acm.py (reference @ v0) with the BasicAcM
the SPP-DDPG scripts inject (train/spp_ddpg_hcheetah.py):
  - ``update(obs, next_obs, action, reward, done, acm_action)``  (ddpg_acm.py:147-201):
    critic step, actor step, polyak of the critic AND actor targets (ddpg.py:273-284)
  - ``loss`` dict {critic, actor[, ddpg, dist]}, ``act`` (noise_action + process_action),
    ``batch_update_acm`` (AcMTrainer.batch_update, acm.py:246-258, BasicAcM incl. t / t1)
Parameters, Adam moments and the normaliser stay on the GPU.
"""
import ctypes

from . import _lib, config, nets
from ._lib import call, ptr, stream_handle
from .offpolicy import NORMALIZER, OffPolicyAgent


class DDPG_AcM(OffPolicyAgent):
    ALGO = _lib.SPP_ALGO_DDPG_ACM
    TRAINABLE = (_lib.SPP_NET_CRITIC1, _lib.SPP_NET_ACTOR, _lib.SPP_NET_ACM)
    TARGETS = {_lib.SPP_NET_CRITIC1_TARG: _lib.SPP_NET_CRITIC1, _lib.SPP_NET_ACTOR_TARG: _lib.SPP_NET_ACTOR}
    CHECKPOINT = (("actor", _lib.SPP_NET_ACTOR), ("critic", _lib.SPP_NET_CRITIC1), (NORMALIZER, None),
                  ("acm", _lib.SPP_NET_ACM))
    acm_kind = "basic"  # BasicAcM: per-step regression path

    def __init__(self, env_name="HalfCheetah-v2", gamma=config.GAMMA, actor_lr=config.DDPG_LR,
                 critic_lr=config.DDPG_LR, tau=config.TAU, act_noise=config.ACT_NOISE,
                 update_batch_size=config.UPDATE_BATCH_SIZE, buffer_size=config.BUFFER_SIZE, acm_lr=config.ACM_LR,
                 acm_critic=config.ACM_CRITIC, custom_loss=0.0, norm_closs=config.NORM_CLOSS,
                 min_max_denormalize=config.MIN_MAX_DENORMALIZE, denormalize_actor_out=config.DENORMALIZE_ACTOR_OUT,
                 obs_norm=config.OBS_NORM, max_batch=None, device="cuda", env_spec=None, seed=None,
                 unbiased_update=False, acm_ob_idx=None, **loop_kw):
        self._check_kwargs(loop_kw)
        _lib.load()
        self.gamma, self.actor_lr, self.critic_lr, self.acm_lr, self.tau = gamma, actor_lr, critic_lr, acm_lr, tau
        self.act_noise = act_noise
        self.acm_critic, self.custom_loss, self.norm_closs = bool(acm_critic), float(custom_loss), bool(norm_closs)
        self.unbiased_update = bool(unbiased_update)  # make_unbiased_update (ddpg_acm.py:59-79)
        self.min_max_denormalize, self.denormalize_actor_out = bool(min_max_denormalize), bool(denormalize_actor_out)
        self._init_spaces(env_name, env_spec, device, acm_ob_idx, update_batch_size, max_batch, loop_kw)
        self._create(seed)
        self._bind_replay(buffer_size, obs_norm, int(loop_kw.get("n_envs", 1)))
        self._init_loop(update_batch_size=update_batch_size, **loop_kw)

    def _net_layouts(self):
        ob, aout, cin = self.ob_dim, self.actor_output_dim, self._critic_in()
        return {_lib.SPP_NET_ACTOR: nets.ddpg_actor_layout(ob, aout),
                _lib.SPP_NET_ACTOR_TARG: nets.ddpg_actor_layout(ob, aout),
                _lib.SPP_NET_CRITIC1: nets.critic_layout(cin), _lib.SPP_NET_CRITIC1_TARG: nets.critic_layout(cin),
                _lib.SPP_NET_ACM: nets.basic_acm_layout(2 * ob, self.ac_dim)}

    # ------------------------------------------------------------------ update
    def update(self, obs, next_obs, action, reward, done, acm_action):
        """DDPG_AcM.update (ddpg_acm.py:147-201)."""
        b, keep = self._batch(obs, next_obs, action, reward, done, acm_action)
        call("sppDdpgAcmUpdate", self._h, ctypes.byref(b), ptr(self._losses), stream_handle())
        self._keep = keep  # inputs must outlive the async work

    def update_from_replay_dp(self, idx, allreduce=None, beside=None):
        """Device-sampled step split at its exchange points (allreduce averages a flat bucket); beside()
        enqueues independent work under the actor bucket's exchange."""
        st = stream_handle()
        self._stage(idx)
        call("sppDdpgAcmCriticGrads", self._h, None, ptr(self._losses), st)
        if allreduce is not None:
            allreduce(self.bucket_critic)
        call("sppDdpgAcmCriticApply", self._h, st)
        call("sppDdpgAcmActorGrads", self._h, ptr(self._losses), st)
        self._exchange(allreduce, self.bucket_actor, beside)
        call("sppDdpgAcmActorApply", self._h, st)

    def _fused_update(self, idx, counter, allreduce=None, beside=None):
        self.update_from_replay_dp(idx, allreduce, beside)

    @property
    def loss(self):
        v = self._losses.detach().cpu().numpy()
        out = {"critic": float(v[0]), "actor": float(v[1])}
        if self.custom_loss:
            out["ddpg"], out["dist"] = float(v[2]), float(v[3])
        return out
