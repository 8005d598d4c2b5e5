"""Torch restatement of vanilla DDPG (rltoolkit/algorithms/ddpg/ddpg.py), test infrastructure only.

  compute_qfunc_targ :239-258  y = r + g (1 - d) Qt(s', mu_t(s'))
  compute_pi_loss    :260-271  -Q(s, mu(s)).mean()
  update             :286-327  critic step, actor step, polyak of the critic AND actor targets (:273-284)
  noise_action       :171-176  clip(mu(s) + act_noise * N(0, 1), +-ac_lim); initial_act / process_action
                     (:178-180, :371-383) pass the action through

``last["grads"]`` and ``layouts`` have the shape oracle/sac.py uses, so bf16_cases.assert_tensor_grads applies.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import nets
from oracle.adam import OracleAdam
from weights import fill_params

NETS = ("actor", "critic", "actor_targ", "critic_targ")


def layouts_of(ob, ac):
    return {"actor": nets.ddpg_actor_layout(ob, ac), "critic": nets.critic_layout(ob + ac),
            "actor_targ": nets.ddpg_actor_layout(ob, ac), "critic_targ": nets.critic_layout(ob + ac)}


class DdpgRef:
    def __init__(self, ob, ac, *, ac_lim=1.0, gamma=0.95, tau=0.005, actor_lr=1e-3, critic_lr=1e-3, params=None,
                 dtype=torch.float32):
        self.dt = dtype
        self.ac_lim = torch.as_tensor(ac_lim, dtype=dtype)
        self.gamma, self.tau = gamma, tau
        self.layouts = layouts_of(ob, ac)
        self.p = {k: {n: torch.as_tensor(params[k][n]).to(dtype).clone().requires_grad_(k in ("actor", "critic"))
                      for n, _ in lay} for k, lay in self.layouts.items()}
        self.opt = {"actor": OracleAdam(self.p["actor"].values(), actor_lr),
                    "critic": OracleAdam(self.p["critic"].values(), critic_lr)}

    def update(self, obs, next_obs, action, reward, done):
        t = lambda a, dt=self.dt: torch.as_tensor(np.asarray(a)).to(dt)  # noqa: E731
        obs, next_obs, action, reward, done = t(obs), t(next_obs), t(action), t(reward), t(done)
        P, losses = self.p, {}
        with torch.no_grad():
            na = nets.ddpg_actor(P["actor_targ"], next_obs, self.ac_lim)
            y = reward + self.gamma * (1 - done) * nets.ddpg_critic(P["critic_targ"], next_obs, na)
        lq = F.mse_loss(nets.ddpg_critic(P["critic"], obs, action), y)
        losses["critic"] = lq.item()
        gq = torch.autograd.grad(lq, list(P["critic"].values()))
        self.opt["critic"].step(gq)
        loss = -nets.ddpg_critic(P["critic"], obs, nets.ddpg_actor(P["actor"], obs, self.ac_lim)).mean()
        losses["actor"] = loss.item()
        ga = torch.autograd.grad(loss, list(P["actor"].values()))
        self.opt["actor"].step(ga)
        flat = lambda gs: torch.cat([x.reshape(-1) for x in gs]).numpy()  # noqa: E731
        self.last = {"y": y, "grads": {"critic": flat(gq), "actor": flat(ga)}}
        with torch.no_grad():
            for c, tg in (("critic", "critic_targ"), ("actor", "actor_targ")):
                for n in P[c]:
                    P[tg][n].mul_(1 - self.tau)
                    P[tg][n].add_(self.tau * P[c][n])
        return losses

    def flat(self, k):
        return nets.flatten(self.p[k]).numpy()


def noise_action(actor_params, obs, ac_lim, noise, act_noise, dtype=torch.float32):
    """DDPG.noise_action with the torch.randn draw given (``noise`` [E, ac], None or act_noise 0: deterministic)."""
    P = {n: torch.as_tensor(v).to(dtype) for n, v in actor_params.items()}
    lim = torch.as_tensor(ac_lim, dtype=dtype)
    with torch.no_grad():
        a = nets.ddpg_actor(P, torch.as_tensor(obs).to(dtype), lim)
        if noise is not None:
            a = a + act_noise * torch.as_tensor(noise).to(dtype)
        return torch.max(torch.min(a, lim), -lim).numpy()


# ---------------------------------------------------------------- the reference-generated fixture
GOLDEN_SEED = 47


def golden_inputs(seed, ob, ac, B, steps):
    """Parameters and batches of tests/golden/ddpg_vanilla_hcheetah.npz, rebuilt from its seed (the fixture
    carries expected outputs only): (params, [batch5 ...], act_obs, act_noise_draw)."""
    from golden_cases import make_batch

    lay = layouts_of(ob, ac)
    params = {k: fill_params(lay[k], seed * 100 + i) for i, k in enumerate(NETS)}
    rng = np.random.RandomState(seed)
    batches = []
    for _ in range(steps):
        obs, next_obs, act, rew, done, _ = make_batch(rng, B, ob, ac, ac)
        batches.append((obs, next_obs, np.clip(act, -1, 1), rew, done))
    act_obs = (rng.randn(5, ob) * 1.3).astype(np.float32)
    act_draw = rng.randn(5, ac).astype(np.float32)
    return params, batches, act_obs, act_draw


def ddpg_vanilla_case():
    """(fixture, params, batches, act_obs, act_draw) of the vanilla DDPG fixture."""
    from golden_cases import load

    fx = load("ddpg_vanilla_hcheetah")
    ob, ac, B = (int(v) for v in fx["dims"])
    params, batches, act_obs, act_draw = golden_inputs(int(fx["seed"]), ob, ac, B, len(fx["losses"]))
    return fx, params, batches, act_obs, act_draw
