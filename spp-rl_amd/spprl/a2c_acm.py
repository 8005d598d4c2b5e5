"""A2C_AcM: rltoolkit's SPP-A2C (acm/on_policy.py:17-157, AcMOnPolicyTrainer on A2C) on the MI355X library.
``PPO_AcM``'s rollout, ACM ring, ACM cadence, side stream and checkpoints (ppo_acm.py) with A2C's update:

  update_critic        a2c.py:186-225, then the one-step TD advantage (a2c.py:227-265, sppOnpTdAdvantage) -- not GAE
  update_actor         custom_loss == 0: A2C.update_actor (a2c.py:267-286), loss["actor"] only
  update_actor_acm     custom_loss != 0 (on_policy.py:100-124): the same gradient -- the buffer's actions come from
                       dist.sample(), so the distance term carries none -- plus loss["dist"] = MSE(actions, next obs)
                       and loss["policy"] = actor + custom_loss * dist.  Without norm_closs the distance is taken on
                       the DENORMALISED actions against the raw next observations while the log-prob stays the stored
                       action's; with norm_closs on the stored actions against the normalised next observations.

Quirks kept: update_actor_acm never calls zero_grad (on_policy.py:117-124), so with custom_loss != 0
the actor's gradient ACCUMULATES over the iterations; the running sum lives on the device (``_actor_grad_sum``) and is
what Adam applies.  It is not part of a checkpoint (the reference's optimizer state is not either).  And the
reference's norm_closs branch calls ``buffer.normalize(next_obs, force=True)``, a keyword Memory.normalize does not
take (memory.py:76): it raises there; here it is MemoryAcM.normalize of the next observations.
Out of scope: data parallelism (single process), discrete actions.
"""
import torch

from . import config
from .onpolicy_loop import refuse_process_group
from .ppo_acm import PPO_AcM


class A2C_AcM(PPO_AcM):
    def __init__(self, env_name="HalfCheetah-v2", gamma=config.GAMMA, actor_lr=3e-3, critic_lr=3e-4,
                 batch_size=config.BATCH_SIZE, custom_loss=0.0, **kw):
        config.refuse_keywords("A2C_AcM", kw, ppo_only=config.PPO_ONLY)
        refuse_process_group("A2C_AcM")
        for k in ("rehearse_world", "dp_update", "comm"):  # PPO_AcM's data-parallel options
            if kw.get(k) is not None:
                raise NotImplementedError("spprl.A2C_AcM is single-process: %s is PPO_AcM's" % k)
        super().__init__(env_name=env_name, gamma=gamma, actor_lr=actor_lr, critic_lr=critic_lr,
                         batch_size=batch_size, custom_loss=custom_loss, **kw)
        self.normalize_adv = bool(self.nets.normalize_adv)
        self.loss = {"actor": 0.0, "critic": 0.0}  # a2c.py:91
        if self.custom_loss:  # on_policy.py:27-29
            self.loss.update(policy=0.0, dist=0.0)
        # update_actor_acm's never-zeroed gradient (on_policy.py:117-124)
        self._actor_grad_sum = torch.zeros_like(self.nets.grads[0]) if self.custom_loss else None

    kl_div_updates_counter = None  # (PPO's counter: A2C_AcM has none)

    def update(self, mem):
        """on_policy.py:74-75: update_critic, TD advantages, one actor step on this iteration's batch."""
        _, _, N, obs, raw_next, nobs, rew, done = self._flatten(mem)
        self.nets.update_critic(obs, nobs, rew, done, advantages=False)  # a2c.py:186-222
        adv, mom = self.nets.td_advantage(obs, nobs, rew, done)  # a2c.py:223, 227-265
        self.last_advantages = adv
        mom = mom if self.normalize_adv else None
        acts = mem["act"].reshape(N, self.ob_dim)
        self.loss["critic"] = self.nets.loss["critic"]
        if not self.custom_loss:  # A2C.update_actor
            out = self.nets.pg_actor_step(obs, acts, adv, mom)
            self.loss["actor"] = float(out[0].item())
        else:  # update_actor_acm
            if self.norm_closs:
                dist_act, nxt = None, nobs
            else:
                dist_act, nxt = self.denormalize(acts), raw_next
            out = self.nets.pg_actor_step(obs, acts, adv, mom, dist_act=dist_act, next_obs=nxt,
                                          grad_sum=self._actor_grad_sum).cpu()
            actor, dist = float(out[0]), float(out[2])
            self.loss.update(actor=actor, dist=dist, policy=actor + self.custom_loss * dist)
        self.loss["acm"] = None
