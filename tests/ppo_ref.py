"""Restatement of vanilla PPO's update (rltoolkit/algorithms/ppo/ppo.py on algorithms/a2c/a2c.py), test
infrastructure only; built on oracle.onpolicy (network steps) and oracle.ppo (GAE).

  update_obs_mean_std   buffer/memory.py:283-302, float64: mean / unbiased std over every observation blended as
                        (1 - alpha) new + alpha old; max / min of the 99th / 1st np.percentile (cast to float32 as
                        the reference's ``.float()``) of the frames' obs rows
  standardize_and_clip  utils.py:62-73
  ppo_update            one iteration's update (a2c.py:137-142): statistics, A2C.update_critic (:186-225, ONE Adam
                        over all targets), PPO.calculate_advantage (ppo.py:101-150), PPO.update_actor (:152-192:
                        AdvantageDataset normalisation, epochs with the KL stop, losses SUMMED over the steps)
  golden_inputs         the hand-filled memory of tests/golden/ppo_vanilla_hcheetah.npz, rebuilt from its seed
"""
import numpy as np
import torch

from oracle import onpolicy as oo
from oracle import ppo as oppo
from oracle.adam import OracleAdam
from weights import fill_params

GOLDEN_SEED = 83
# (frames, how the rollout ended): "limit" = a time-limit end, end but not done (a2c.py:170-171)
GOLDEN_ROLLOUTS = ((40, "done"), (25, "done"), (31, "limit"))


def standardize_and_clip(x, mean, std, max_abs=10.0):
    x, mean, std = (np.asarray(v, np.float64) for v in (x, mean, std))
    return np.clip((x - mean) / (std + 1e-8), -max_abs, max_abs)


def update_obs_mean_std(start_obs, next_obs, obs, alpha, mean, std, max_obs=None, min_obs=None):
    """Returns (mean, std, max_obs, min_obs); mean / std float64, max / min float32 (the reference's casts)."""
    every = np.concatenate([np.asarray(start_obs, np.float64), np.asarray(next_obs, np.float64)])
    new_mean, new_std = every.mean(0), every.std(0, ddof=1)
    mean = (1 - alpha) * new_mean + alpha * np.asarray(mean, np.float64)
    std = (1 - alpha) * new_std + alpha * np.asarray(std, np.float64)
    obs = np.asarray(obs, np.float64)
    cur_max = np.percentile(obs, 99, axis=0).astype(np.float32)
    cur_min = np.percentile(obs, 1, axis=0).astype(np.float32)
    if max_obs is not None and min_obs is not None:
        cur_max, cur_min = np.maximum(cur_max, max_obs), np.minimum(cur_min, min_obs)
    return mean, std, cur_max, cur_min


def normalize_adv(adv, dtype):
    a = torch.as_tensor(np.asarray(adv)).to(dtype)
    return ((a - a.mean()) / (a.std() + 1.2e-7)).numpy()  # advantage_dataset.py:9-12


def update_critic(flat, ob, obs, nobs, rew, done, gamma, lr, targets, steps, dtype=torch.float32):
    """A2C.update_critic: returns (flat, mean loss).  One Adam state across every target's steps."""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    p = torch.from_numpy(np.array(flat, np_dt, copy=True))
    opt = OracleAdam([p], lr)
    lay = oo.critic_layout(ob)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
    total = 0.0
    for _ in range(targets):
        with torch.no_grad():
            vn = oo.critic(oo._params(p.numpy(), lay, dtype), t(nobs)).squeeze(-1)
            q = (t(rew) + gamma * (1 - t(done)) * vn).numpy()
        for _ in range(steps):
            loss, g = oo.critic_step(p.numpy(), ob, np.asarray(obs, np_dt), q, dtype=dtype)
            opt.step([torch.from_numpy(np.asarray(g, np_dt))])
            total += loss
    return p.numpy(), total / (targets * steps)


def values(flat, ob, x, dtype=torch.float32):
    with torch.no_grad():
        return oo.critic(oo._params(flat, oo.critic_layout(ob), dtype),
                         torch.as_tensor(np.asarray(x)).to(dtype)).squeeze(-1).numpy()


def advantages(flat, ob, obs, nobs, rew, done, end, gamma, lam, dtype=torch.float32):
    """PPO.calculate_advantage: q = r + g (1 - d) V(s'), deltas = q - V(s), the reverse GAE scan (one stream)."""
    v, vn = values(flat, ob, obs, dtype), values(flat, ob, nobs, dtype)
    rew, done = np.asarray(rew, v.dtype), np.asarray(done, v.dtype)
    delta = rew + gamma * (1 - done) * vn - v
    return oppo.gae_loop(delta, np.asarray(done, bool), np.asarray(end, bool), vn, gamma, lam)


def update_actor(flat, ob, ac, lim, obs, act, lp_old, adv, lr, max_epochs, kl_threshold, batch_size, eps_clip=0.2,
                 entropy_coef=0.0, perms=None, dtype=torch.float32):
    """PPO.update_actor on already normalised advantages.  Returns (flat, loss sums {actor, entropy, sum}, the KL
    of every epoch run, the counter increment i + 1)."""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    p = torch.from_numpy(np.array(flat, np_dt, copy=True))
    opt = OracleAdam([p], lr)
    n = len(obs)
    tot = {"actor": 0.0, "entropy": 0.0, "sum": 0.0}
    kl, kls, i = 0.0, [], 0
    for i in range(max_epochs):
        if kl >= kl_threshold:
            break
        perm = np.arange(n) if perms is None else np.asarray(perms[i])
        for s in range(0, n, batch_size):
            b = perm[s:s + batch_size]
            out, g = oo.actor_step(p.numpy(), ob, ac, lim, obs[b], act[b], lp_old[b], adv[b], eps_clip=eps_clip,
                                   entropy_coef=entropy_coef, dtype=dtype)
            opt.step([torch.from_numpy(np.asarray(g, np_dt))])
            tot["actor"] += out["actor"]
            tot["entropy"] += out["entropy"]
            tot["sum"] += out["actor"] - entropy_coef * out["entropy"]
            kl = out["kl"]  # of the epoch's last minibatch, before its step (ppo.py:189)
        kls.append(kl)
    return p.numpy(), tot, kls, i + 1


def ppo_update(actor, critic, mem, ob, ac, lim, *, alpha, gamma, gae_lambda, actor_lr, critic_lr, targets, steps,
               max_epochs, kl_threshold, batch_size, eps_clip=0.2, entropy_coef=0.0, mean=None, std=None, perms=None,
               dtype=torch.float32):
    """One iteration's update on a memory dict of RAW observations (obs / next_obs [N][ob], start_obs [R][ob], act,
    lp, rew, done, end).  Returns a dict with the statistics and every intermediate the fixture records."""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    out = {}
    if alpha is not None:
        mean = np.zeros(ob) if mean is None else mean
        std = np.ones(ob) if std is None else std
        mean, std, mx, mn = update_obs_mean_std(mem["start_obs"], mem["next_obs"], mem["obs"], alpha, mean, std)
        out.update(obs_mean=mean, obs_std=std, max_obs=mx, min_obs=mn)
        # the reference holds float32 statistics: normalise with those
        m32, s32 = mean.astype(np.float32), std.astype(np.float32)
        obs = standardize_and_clip(mem["obs"], m32, s32).astype(np_dt)
        nobs = standardize_and_clip(mem["next_obs"], m32, s32).astype(np_dt)
    else:
        obs, nobs = np.asarray(mem["obs"], np_dt), np.asarray(mem["next_obs"], np_dt)
    rew, done, end = mem["rew"], np.asarray(mem["done"], np.float32), mem["end"]
    critic, closs = update_critic(critic, ob, obs, nobs, rew, done, gamma, critic_lr, targets, steps, dtype)
    adv = advantages(critic, ob, obs, nobs, rew, done, end, gamma, gae_lambda, dtype)
    out.update(norm_obs=obs, critic=critic, critic_loss=closs, adv=adv)
    actor, sums, kls, cnt = update_actor(actor, ob, ac, lim, obs, np.asarray(mem["act"], np_dt),
                                         np.asarray(mem["lp"], np_dt), normalize_adv(adv, dtype), actor_lr, max_epochs,
                                         kl_threshold, batch_size, eps_clip, entropy_coef, perms, dtype)
    out.update(actor=actor, loss=dict(sums, critic=closs), kls=kls, counter=cnt)
    return out


# ---------------------------------------------------------------- seeded inputs
def flat_of(layout, seed):
    p = fill_params(layout, seed)
    return np.concatenate([p[n].ravel() for n, _ in layout])


def golden_params(seed, ob, ac):
    """(actor flat, critic flat) of the fixture: fill_params in state_dict order (log_scale first)."""
    return flat_of(oo.actor_layout(ob, ac), seed * 100), flat_of(oo.critic_layout(ob), seed * 100 + 1)


def rollout_memory(rng, ob, ac, rollouts, clip_col=None):
    """A hand-filled memory of whole rollouts: raw observations with per-column offsets and scales (so no column
    mean sits near zero), one column with outliers beyond the +-10 clip, actions, rewards, done / end flags.
    ``lp`` is left to the caller (it depends on the actor)."""
    offs = rng.uniform(0.5, 2.0, ob) * rng.choice([-1.0, 1.0], ob)
    scale = rng.uniform(0.3, 2.5, ob)
    obs, nobs, start, done, end = [], [], [], [], []
    for frames, how in rollouts:
        seq = (offs + scale * rng.randn(frames + 1, ob)).astype(np.float32)
        if clip_col is not None:
            seq[frames // 2, clip_col] += np.float32(60.0)
        start.append(seq[:1])
        obs.append(seq[:-1])
        nobs.append(seq[1:])
        d = np.zeros(frames, np.float32)
        e = np.zeros(frames, np.float32)
        e[-1] = 1.0
        d[-1] = 1.0 if how == "done" else 0.0
        done.append(d)
        end.append(e)
    obs, nobs = np.concatenate(obs), np.concatenate(nobs)
    N = len(obs)
    return {"obs": obs, "next_obs": nobs, "start_obs": np.concatenate(start), "done": np.concatenate(done),
            "end": np.concatenate(end), "act": rng.uniform(-1.1, 1.1, (N, ac)).astype(np.float32),
            "rew": rng.randn(N).astype(np.float32), "lp_noise": (0.2 * rng.randn(N)).astype(np.float32), "T": N, "E": 1}


def golden_inputs(seed=GOLDEN_SEED, ob=17, ac=6):
    """(actor flat, critic flat, memory without ``lp``) of tests/golden/ppo_vanilla_hcheetah.npz."""
    actor, critic = golden_params(seed, ob, ac)
    return actor, critic, rollout_memory(np.random.RandomState(seed), ob, ac, GOLDEN_ROLLOUTS, clip_col=3)


def ppo_vanilla_case():
    """(fixture, actor flat, critic flat, memory with the fixture's lp_old)."""
    from golden_cases import load

    fx = load("ppo_vanilla_hcheetah")
    ob, ac = (int(v) for v in fx["dims"])
    actor, critic, mem = golden_inputs(int(fx["seed"]), ob, ac)
    mem["lp"] = fx["lp_old"]
    return fx, actor, critic, mem
