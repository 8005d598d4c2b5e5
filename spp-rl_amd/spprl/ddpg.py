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
import torch

from . import _lib, config
from .ddpg_acm import DDPG_AcM
from .offpolicy import Vanilla


class DDPG(Vanilla, DDPG_AcM):
    ALGO = _lib.SPP_ALGO_DDPG
    TRAINABLE = DDPG_AcM.TRAINABLE[:-1]  # no ACM net at all: bucket_acm is None
    CHECKPOINT = DDPG_AcM.CHECKPOINT[:-1]  # ddpg.py:331-352
    acm_kind = None

    def __init__(self, env_name="HalfCheetah-v2", gamma=config.GAMMA, actor_lr=config.DDPG_LR,
                 critic_lr=config.DDPG_LR, tau=config.TAU, act_noise=config.ACT_NOISE,
                 update_batch_size=config.UPDATE_BATCH_SIZE, buffer_size=config.BUFFER_SIZE,
                 obs_norm=config.OBS_NORM, max_batch=None, device="cuda", env_spec=None, seed=None, **loop_kw):
        # DDPG -> RL -> MetaLearner (ddpg.py:19-33, rl.py:17-26) take no AcMTrainer / AcMOffPolicy / DDPG_AcM
        # keyword: the reference raises TypeError on them, and so does this class, before the library is touched
        config.refuse_keywords("DDPG", loop_kw, config.ACM_ONLY_OFF_POLICY)
        loop_kw.pop("min_max_denormalize", None)  # MetaLearner's; without obs_norm it normalises nothing here
        super().__init__(env_name=env_name, gamma=gamma, actor_lr=actor_lr, critic_lr=critic_lr, tau=tau,
                         act_noise=act_noise, update_batch_size=update_batch_size, buffer_size=buffer_size,
                         acm_lr=0.0, acm_critic=False, custom_loss=0.0, norm_closs=False, min_max_denormalize=False,
                         denormalize_actor_out=False, obs_norm=obs_norm, max_batch=max_batch, device=device,
                         env_spec=env_spec, seed=seed, acm_epochs=0, **loop_kw)  # (acm_epochs: no ACM anywhere)

    def _net_layouts(self):
        lay = super()._net_layouts()
        del lay[_lib.SPP_NET_ACM]
        return lay

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

    def batch_update_acm(self, x, y):
        raise AttributeError("vanilla DDPG has no ACM (rltoolkit DDPG defines none)")
