"""Restatement of A2C's update (rltoolkit/algorithms/a2c/a2c.py) and of A2C_AcM's actor step
(rltoolkit/acm/on_policy.py:88-124), test infrastructure only; torch on the CPU, parameterised by dtype, built on
oracle.onpolicy (networks) and tests/ppo_ref.py (statistics, update_critic, the seeded memory).

  td_advantage      A2C.calculate_advantage (a2c.py:227-265): q = r + gamma (1 - d) V(s'), adv = q - V(s)
  normalize_adv     a2c.py:274-277: (adv - mean) / (std(ddof 1) + 1e-8) over the whole batch
  pg_actor_grad     A2C.update_actor's loss and gradient (a2c.py:279-284): (-logp(act | x) * A).mean(); the AcM's
                    distance MSE(dist_act or act, next_obs) is data only (on_policy.py:106-121)
  a2c_update        one iteration's update (a2c.py:137-142): statistics, update_critic, advantages, ONE Adam step of
                    the actor through the log-probs of the rollout-normalised observations
  acm_updates       A2C_AcM over consecutive memories: update_critic, advantages, update_actor_acm, whose gradient is
                    never zeroed (on_policy.py:117-124): step k applies g_1 + ... + g_k
"""
import numpy as np
import torch

import ppo_ref
from oracle import onpolicy as oo
from oracle.adam import OracleAdam
from ppo_ref import flat_of, golden_inputs, standardize_and_clip, update_critic, update_obs_mean_std  # noqa: F401

ACM_SEED = 87
ACM_ROLLOUTS = (ppo_ref.GOLDEN_ROLLOUTS, ((33, "limit"), (28, "done"), (35, "done")))  # two memories of 96 frames


def _np(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def td_advantage(critic, ob, obs, nobs, rew, done, gamma, dtype=torch.float32):
    """(adv, q) in the reference's operation order."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
    with torch.no_grad():
        p = oo._params(critic, oo.critic_layout(ob), dtype)
        q = t(rew) + gamma * (1 - t(done)) * oo.critic(p, t(nobs)).squeeze(-1)
        adv = q - oo.critic(p, t(obs)).squeeze(-1)
    return adv.numpy(), q.numpy()


def normalize_adv(adv, dtype=torch.float32):
    a = torch.as_tensor(np.asarray(adv)).to(dtype)
    return ((a - a.mean()) / (a.std() + 1e-8)).numpy()


def pg_actor_grad(flat, ob, aout, lim, x, act, adv_hat, dist_act=None, next_obs=None, dtype=torch.float32):
    """Returns ({actor, logp, entropy[, dist]}, grad) of (-logp * adv_hat).mean()."""
    p = oo._params(flat, oo.actor_layout(ob, aout), dtype)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
    dist = oo.actor_dist(p, t(x), t(lim))
    lp = dist.log_prob(t(act))
    loss = (-lp * t(adv_hat)).mean()
    g = oo._flat(torch.autograd.grad(loss, list(p.values())))
    out = {"actor": loss.item(), "logp": lp.mean().item(), "entropy": dist.entropy().mean().item()}
    if next_obs is not None:
        out["dist"] = torch.nn.functional.mse_loss(t(act if dist_act is None else dist_act), t(next_obs)).item()
    return out, g


def a2c_update(actor, critic, mem, ob, ac, lim, *, alpha, gamma, actor_lr, critic_lr, targets, steps,
               normalize=True, mean=None, std=None, actor_new_stats=False, dtype=torch.float32):
    """One iteration's update on a memory dict of RAW observations.  ``actor_new_stats`` is the WRONG order (the
    actor on observations normalised with the updated statistics): tests use it to show the fixture sees the quirk."""
    np_dt = _np(dtype)
    out = {}
    mean = np.zeros(ob) if mean is None else mean
    std = np.ones(ob) if std is None else std
    old = (np.asarray(mean, np.float32), np.asarray(std, np.float32))
    if alpha is not None:
        mean, std, mx, mn = update_obs_mean_std(mem["start_obs"], mem["next_obs"], mem["obs"], alpha, mean, std)
        out.update(obs_mean=mean, obs_std=std, max_obs=mx, min_obs=mn)
    m32, s32 = np.asarray(mean, np.float32), np.asarray(std, np.float32)  # (the reference holds float32 statistics)
    obs = standardize_and_clip(mem["obs"], m32, s32).astype(np_dt)
    nobs = standardize_and_clip(mem["next_obs"], m32, s32).astype(np_dt)
    rew, done = mem["rew"], np.asarray(mem["done"], np.float32)
    critic, closs = update_critic(critic, ob, obs, nobs, rew, done, gamma, critic_lr, targets, steps, dtype)
    adv, q = td_advantage(critic, ob, obs, nobs, rew, done, gamma, dtype)
    out.update(critic=critic, critic_loss=closs, adv=adv, q=q)
    x = obs if actor_new_stats else standardize_and_clip(mem["obs"], *old).astype(np_dt)
    res, g = pg_actor_grad(actor, ob, ac, lim, x, mem["act"], normalize_adv(adv, dtype) if normalize else adv,
                           dtype=dtype)
    p = torch.from_numpy(np.array(actor, np_dt, copy=True))
    OracleAdam([p], actor_lr).step([torch.from_numpy(np.asarray(g, np_dt))])
    out.update(actor=p.numpy(), actor_loss=res["actor"], actor_grad=g)
    return out


# ---------------------------------------------------------------- A2C_AcM
def minmax_normalize(x, lo, hi):
    """MemoryAcM.normalize with min_max_denormalize (memory.py:77-82), float32 as the reference."""
    x, lo, hi = (np.asarray(v, np.float32) for v in (x, lo, hi))
    mean = (hi + lo) / np.float32(2)
    return (x - mean) / (hi - mean + np.float32(1e-8))


def minmax_denormalize(x, lo, hi):
    """MemoryAcM.denormalize (memory.py:119-121)."""
    x, lo, hi = (np.asarray(v, np.float32) for v in (x, lo, hi))
    return (hi + lo) / np.float32(2) + x * ((hi - lo) / np.float32(2))


def acm_updates(actor, critic, mems, ob, lim, lo, hi, *, gamma, actor_lr, critic_lr, targets, steps, custom_loss,
                norm_closs=False, zero_grad=False, dtype=torch.float32):
    """A2C_AcM's update_critic + update_actor_acm over ``mems`` in turn (one Adam per network for all of them).
    ``zero_grad`` is what the reference does NOT do.  Returns one dict per memory."""
    np_dt = _np(dtype)
    pa = torch.from_numpy(np.array(actor, np_dt, copy=True))
    opt = OracleAdam([pa], actor_lr)
    gsum = np.zeros(len(actor), np_dt)
    res = []
    # (A2C.update_critic builds no optimizer of its own: one Adam state over every call)
    pc = torch.from_numpy(np.array(critic, np_dt, copy=True))
    copt = OracleAdam([pc], critic_lr)
    for mem in mems:
        obs = minmax_normalize(mem["obs"], lo, hi).astype(np_dt)
        nobs = minmax_normalize(mem["next_obs"], lo, hi).astype(np_dt)
        rew, done = mem["rew"], np.asarray(mem["done"], np.float32)
        total = 0.0
        t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
        for _ in range(targets):
            with torch.no_grad():
                vn = oo.critic(oo._params(pc.numpy(), oo.critic_layout(ob), dtype), t(nobs)).squeeze(-1)
                q = (t(rew) + gamma * (1 - t(done)) * vn).numpy()
            for _ in range(steps):
                loss, g = oo.critic_step(pc.numpy(), ob, obs, q, dtype=dtype)
                copt.step([torch.from_numpy(np.asarray(g, np_dt))])
                total += loss
        adv, _ = td_advantage(pc.numpy(), ob, obs, nobs, rew, done, gamma, dtype)
        if norm_closs:
            dist_act, nxt = None, nobs
        else:
            dist_act, nxt = minmax_denormalize(mem["act"], lo, hi), mem["next_obs"]
        out, g = pg_actor_grad(pa.numpy(), ob, ob, lim, obs, mem["act"], normalize_adv(adv, dtype), dist_act, nxt,
                               dtype)
        gsum = np.asarray(g, np_dt) if zero_grad else gsum + np.asarray(g, np_dt)
        opt.step([torch.from_numpy(gsum.copy())])
        res.append({"actor": out["actor"], "dist": out["dist"], "policy": out["actor"] + custom_loss * out["dist"],
                    "critic_loss": total / (targets * steps), "adv": adv, "critic_post": pc.numpy().copy(),
                    "actor_post": pa.numpy().copy(), "grad": np.asarray(g, np_dt)})
    return res


def acm_inputs(seed=ACM_SEED, ob=17):
    """(actor flat, critic flat, [memory, memory], min_obs, max_obs) of tests/golden/a2c_acm_hcheetah.npz: the
    actor emits ob-dim actions; the min / max of the normaliser bracket the seeded observations' bulk."""
    actor = flat_of(oo.actor_layout(ob, ob), seed * 100)
    critic = flat_of(oo.critic_layout(ob), seed * 100 + 1)
    rng = np.random.RandomState(seed)
    mems = [ppo_ref.rollout_memory(rng, ob, ob, r) for r in ACM_ROLLOUTS]
    every = np.concatenate([m["obs"] for m in mems])
    lo = np.percentile(every.astype(np.float64), 1, axis=0).astype(np.float32)
    hi = np.percentile(every.astype(np.float64), 99, axis=0).astype(np.float32)
    return actor, critic, mems, lo, hi


def vanilla_start_stats(seed, ob):
    """The running (mean, std) the vanilla fixture's iteration starts from: an earlier iteration's, far enough from
    the memory's own that alpha = 0.95 moves them visibly."""
    rng = np.random.RandomState(seed + 1)
    return rng.uniform(-3.0, 3.0, ob).astype(np.float32), rng.uniform(0.2, 0.6, ob).astype(np.float32)


def a2c_vanilla_case():
    """(fixture, actor flat, critic flat, memory) of tests/golden/a2c_vanilla_hcheetah.npz."""
    from golden_cases import load

    fx = load("a2c_vanilla_hcheetah")
    ob, ac = (int(v) for v in fx["dims"])
    actor, critic, mem = golden_inputs(int(fx["seed"]), ob, ac)
    return fx, actor, critic, mem


def a2c_acm_case():
    from golden_cases import load

    fx = load("a2c_acm_hcheetah")
    return (fx,) + acm_inputs(int(fx["seed"]), int(fx["dims"][0]))
