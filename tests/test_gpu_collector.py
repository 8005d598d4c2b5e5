"""GPU: the vectorised collector's bookkeeping kernels, and the loop against what its envs saw.

sppEpisodeAccum (k_episode_accum: the running returns perform_iteration reports and return_done stops on),
sppSynthEnvReset (k_synth_reset) and sppRandUniform (k_rand_uniform: the pre-train collector's action draw) against
plain restatements; then OffPolicyLoop._vector_step (spprl/trainer.py) on host envs that log every transition they
serve, record by record.

No tolerance here is a measured number.  The equalities are exact by construction: the kernel does one fp32 add per
step in the order of the restatement, and rewards on the 2^-8 grid keep every partial sum exact in fp32 and fp64
whatever the order.  The two bounds are derived: any-order fp64 summation of K terms is within (K - 1) * 2^-53 *
sum|x| of the exact sum, and a sample mean / variance lies within 5 standard errors of its expectation.
"""
import math

import numpy as np
import pytest
import torch

import ring_cases as rc
import spprl
from spprl._lib import call, ptr, stream_handle
from spprl.trainer import HostVecEnv
from test_trainer import _NpSynthEnv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ sppEpisodeAccum
STEPS = 20
ALL_END, NONE_END_NULL, NONE_END_ZEROS = 7, 3, 12  # steps where every env ends / none does (end NULL / all zero)


def _ends(rng, E):
    end = rng.rand(STEPS, E) < 0.15
    end[ALL_END] = True
    end[NONE_END_NULL] = end[NONE_END_ZEROS] = False
    return end


def _accum_run(rew, end, sums0):
    """The kernel over STEPS calls -> ep_ret after every call [STEPS, E], sums after every call [STEPS, 2]; and the
    restatement: one np.float32 add per step, the finished returns in (step, env) order."""
    E = rew.shape[1]
    ep = torch.zeros(E, device=DEV)
    sums = _t(np.array(sums0, np.float64))
    got_ep, got_sums = [], []
    want = np.zeros(E, np.float32)
    want_ep, fin = [], []
    for t in range(STEPS):
        r_dev, e_dev = _t(rew[t]), None if t == NONE_END_NULL else _t(end[t].astype(np.uint8))
        call("sppEpisodeAccum", ptr(r_dev), ptr(e_dev), E, ptr(ep), ptr(sums), stream_handle())
        got_ep.append(ep.cpu().numpy())
        got_sums.append(sums.cpu().numpy())
        want = want + rew[t]  # float32 + float32
        assert want.dtype == np.float32
        fin.append(want[end[t]].copy())
        want[end[t]] = 0.0
        want_ep.append(want.copy())
    return np.stack(got_ep), np.stack(got_sums), np.stack(want_ep), fin


@pytest.mark.parametrize("E", [1, 63, 64, 65, 255, 257, 1000])
def test_episode_accum_exact_on_the_grid(E):
    """Rewards k / 256 with |k| <= 1024: every partial sum (at most 20 * 1000 terms of at most 4) is a multiple of
    2^-8 below 2^17, exact in fp32 and fp64, so sums[0] does not depend on the order of the atomics."""
    rng = np.random.RandomState(E)
    rew = (rng.randint(-1024, 1025, (STEPS, E)) / 256.0).astype(np.float32)
    end = _ends(rng, E)
    sums0 = (3.5, 2.0)  # the kernel accumulates into sums and never zeroes it
    got_ep, got_sums, want_ep, fin = _accum_run(rew, end, sums0)
    np.testing.assert_array_equal(got_ep.view(np.uint32), want_ep.view(np.uint32))
    assert (got_ep[end] == 0).all() and (got_ep[ALL_END] == 0).all()
    tot, cnt = sums0
    for t in range(STEPS):
        tot += float(fin[t].astype(np.float64).sum())
        cnt += len(fin[t])
        assert got_sums[t, 0] == tot and got_sums[t, 1] == cnt, t
    for t in (NONE_END_NULL, NONE_END_ZEROS):  # no env ended: sums untouched, bit for bit
        np.testing.assert_array_equal(got_sums[t].view(np.uint64), got_sums[t - 1].view(np.uint64))
    assert cnt - sums0[1] >= E  # (the ALL_END step alone finishes E episodes)


@pytest.mark.parametrize("E", [1, 63, 64, 65, 255, 257, 1000])
def test_episode_accum_gaussian_rewards(E):
    rng = np.random.RandomState(1000 + E)
    rew = rng.randn(STEPS, E).astype(np.float32)
    end = _ends(rng, E)
    got_ep, got_sums, want_ep, fin = _accum_run(rew, end, (0.0, 0.0))
    np.testing.assert_array_equal(got_ep.view(np.uint32), want_ep.view(np.uint32))
    rets = np.concatenate(fin).astype(np.float64)
    K = len(rets)
    exact = math.fsum(rets)  # the exact sum of the fp32 returns, correctly rounded
    bound = (K - 1) * 2.0 ** -53 * float(np.abs(rets).sum())
    print("E=%d K=%d |sums[0] - exact| = %.3g, bound %.3g" % (E, K, abs(got_sums[-1, 0] - exact), bound))
    assert abs(got_sums[-1, 0] - exact) <= bound
    assert got_sums[-1, 1] == K


def test_episode_accum_null_end_leaves_sums_alone():
    E = 300
    rng = np.random.RandomState(5)
    rew = rng.randn(E).astype(np.float32)
    ep0 = rng.randn(E).astype(np.float32)
    ep, r_dev = _t(ep0), _t(rew)
    sums = _t(np.array([-1.25, 7.0]))
    call("sppEpisodeAccum", ptr(r_dev), None, E, ptr(ep), ptr(sums), stream_handle())
    np.testing.assert_array_equal(ep.cpu().numpy().view(np.uint32), (ep0 + rew).view(np.uint32))
    np.testing.assert_array_equal(sums.cpu().numpy(), [-1.25, 7.0])


# ------------------------------------------------------------------ sppSynthEnvReset
RESET_SHAPES = [(1, 3), (23, 11), (24, 11), (300, 17)]  # 253 and 264 elements: either side of the 256-thread block


def _reset(E, ob, mask, seed, offset, fill=None):
    obs = torch.empty(E, ob, device=DEV) if fill is None else _t(fill)
    m = None if mask is None else _t(mask.astype(np.uint8))
    call("sppSynthEnvReset", ptr(obs), ptr(m), E, ob, seed, offset, stream_handle())
    return obs.cpu().numpy()


@pytest.mark.parametrize("E,ob", RESET_SHAPES)
def test_synth_env_reset_draws(E, ob):
    seed, offset = 0x5EED0000 + E, 3
    n = E * ob
    got = _reset(E, ob, None, seed, offset)
    normal = torch.empty(4 * n, device=DEV)
    call("sppRandNormal", ptr(normal), 4 * n, seed, offset, stream_handle())
    # element i is the first normal of Philox group i (k_synth_reset), i.e. element 4 i of the plain draw
    np.testing.assert_array_equal(got.reshape(-1).view(np.uint32), normal.cpu().numpy()[::4].view(np.uint32))
    np.testing.assert_array_equal(_reset(E, ob, None, seed, offset).view(np.uint32), got.view(np.uint32))
    other = _reset(E, ob, None, seed, offset + 1)
    assert (other != got).any(1).all()  # the next offset: every row is another row
    # masked: the rows not asked for keep their bits, the others are the unmasked call's
    rng = np.random.RandomState(E)
    mask = rng.rand(E) < 0.5
    mask[0] = True
    if E > 1:
        mask[-1] = False
    fill = (rng.rand(E, ob) + 2).astype(np.float32)
    part = _reset(E, ob, mask, seed, offset, fill)
    np.testing.assert_array_equal(part[~mask].view(np.uint32), fill[~mask].view(np.uint32))
    np.testing.assert_array_equal(part[mask].view(np.uint32), got[mask].view(np.uint32))
    if n >= 5000:  # N(0, 1): mean within 5 / sqrt(n), variance within 5 * sqrt(2 / (n - 1))
        assert abs(got.mean()) < 5 / math.sqrt(n)
        assert abs(got.astype(np.float64).var(ddof=1) - 1) < 5 * math.sqrt(2 / (n - 1))


# ------------------------------------------------------------------ sppRandUniform
UNIFORM_N = [1, 5, 8, 1001, 1 << 20]


def _uniform(n, lo, hi, seed, offset):
    out, lo_dev, hi_dev = torch.empty(n, device=DEV), _t(lo), _t(hi)  # (named: all three live until the copy back)
    call("sppRandUniform", ptr(out), n, ptr(lo_dev), ptr(hi_dev), len(lo), seed, offset, stream_handle())
    return out.cpu().numpy()


@pytest.mark.parametrize("period", [1, 3, 6, 8])
def test_rand_uniform_columns_and_prefix(period):
    """Column c of the [n / period, period] draw lies in its own interval [10 c, 10 c + 1] (disjoint: a wrong
    j % period fails on every element); the first values do not depend on n; the same (seed, offset) repeats."""
    seed, offset = 99, 4
    lo = (10.0 * np.arange(period)).astype(np.float32)
    hi = lo + 1
    full = _uniform(UNIFORM_N[-1], lo, hi, seed, offset)
    for n in UNIFORM_N:
        x = _uniform(n, lo, hi, seed, offset)
        c = np.arange(n) % period
        assert (x >= lo[c]).all() and (x <= hi[c]).all(), n
        np.testing.assert_array_equal(x.view(np.uint32), full[:n].view(np.uint32), err_msg=str(n))
    assert not np.array_equal(_uniform(1001, lo, hi, seed, offset + 1), full[:1001])
    # the unit draw: 24-bit fractions; column c of the scaled draw is lo + u * (hi - lo) of the same u
    u = _uniform(UNIFORM_N[-1], np.zeros(period, np.float32), np.ones(period, np.float32), seed, offset)
    k = u.astype(np.float64) * 2.0 ** 24
    assert (k == np.floor(k)).all() and (k >= 0).all() and (k < 2 ** 24).all()
    c = np.arange(len(u)) % period
    np.testing.assert_array_equal(full.view(np.uint32), (lo[c] + u * (hi[c] - lo[c])).view(np.uint32))


def test_rand_uniform_chi_square():
    from scipy import stats

    n = 1 << 20
    u = _uniform(n, np.zeros(1, np.float32), np.ones(1, np.float32), 1234, 9)
    counts = np.bincount((u * 64).astype(np.int64), minlength=64)
    assert len(counts) == 64
    p = stats.chisquare(counts).pvalue  # (the threshold of test_rand_index_range_and_uniformity)
    assert p > 1e-4, p
    assert abs(u.mean() - 0.5) < 6 / math.sqrt(12 * n)


# ------------------------------------------------------------------ the loop against what the envs saw
class _LogEnv(_NpSynthEnv):
    """_NpSynthEnv with rewards on the 2^-8 grid, an optional early termination at a seeded step of every episode,
    and a log of everything it serves: per transition (obs, action, reward, next_obs, ended, early) and every reset
    observation."""

    def __init__(self, ob, ac, T, seed, early=False):
        super().__init__(ob=ob, ac=ac, T=T, seed=seed)
        self._early, self._stop = early, None
        self.log, self.resets = [], []

    def reset(self):
        o = super().reset()
        self._stop = int(self._rng.randint(2, self._max_episode_steps)) if self._early else None
        self.resets.append(o.copy())
        return o

    def step(self, a):
        a = np.array(a, np.float32).reshape(-1)  # (a copy: the caller's staging buffer is reused)
        before = self._s.copy()
        o, r, d, info = super().step(a)
        r = float(np.round(r * 256.0) / 256.0)
        early = self._stop is not None and self._t == self._stop
        self.log.append((before, a, r, o.copy(), bool(d or early), bool(early)))
        return o, r, bool(d or early), info


def _run_and_check(ag, envs, vanilla):
    """Train, then compare the ring, the counters and every iteration's return with the envs' logs."""
    E = len(envs)
    iters = []  # (return, frames) after every perform_iteration
    orig = ag.perform_iteration

    def logged():
        r = orig()
        iters.append((r, ag.stats_logger.frames))
        return r

    ag.perform_iteration = logged
    ag.train()
    torch.cuda.synchronize()
    rb = ag.replay_buffer
    n = len(rb)
    K = n // E
    assert n == K * E and all(len(e.log) == K for e in envs)  # the ring did not wrap: record k E + e is (env e, k)
    field = lambda i: np.stack([np.stack([np.asarray(e.log[k][i]) for e in envs]) for k in range(K)])  # noqa: E731
    obs, act, rew, nobs, ended, early = (field(i) for i in range(6))
    got = rb.gather(torch.arange(n))
    g = [x.cpu().numpy() for x in got]
    flat = lambda a: a.reshape((n,) + a.shape[2:])  # noqa: E731
    np.testing.assert_array_equal(g[0].view(np.uint32), flat(obs).view(np.uint32))
    np.testing.assert_array_equal(g[1].view(np.uint32), flat(nobs).view(np.uint32))
    np.testing.assert_array_equal(g[3].view(np.uint32), flat(rew).astype(np.float32).view(np.uint32))
    # the action the env received: the ACM action of the AcM ring, the action itself of the vanilla ring
    np.testing.assert_array_equal(g[2 if vanilla else 5].view(np.uint32), flat(act).view(np.uint32))
    # done: the end flag, except that a vanilla class does not call a time-limit end done (Q3)
    want_done = flat(early) if vanilla else flat(ended)
    np.testing.assert_array_equal(g[4], want_done.astype(np.int8))
    heads = rc.record_heads(rb, n)
    np.testing.assert_array_equal(heads[:, 3] >> 8, flat(ended))  # end: time limit and early termination alike
    np.testing.assert_array_equal(heads[:, 3] & 1, want_done)
    assert flat(ended).sum() > flat(early).sum() > 0 or not vanilla
    # the record after an episode end starts from that env's next reset observation
    for e, env in enumerate(envs):
        ends = np.flatnonzero(ended[:, e])
        assert len(env.resets) in (len(ends), len(ends) + 1)  # (no reset after an end on the very last step)
        np.testing.assert_array_equal(g[0][e].view(np.uint32), env.resets[0].view(np.uint32))
        for j, k in enumerate(ends):
            if k + 1 < K:
                np.testing.assert_array_equal(g[0][(k + 1) * E + e].view(np.uint32),
                                              env.resets[j + 1].view(np.uint32))
    assert ag.stats_logger.frames == n == sum(len(e.log) for e in envs)
    assert ag.stats_logger.rollouts == sum(len(e.resets) for e in envs)
    # each iteration reports the mean return of the episodes that finished in it (running fp32 sums: exact on the grid)
    k0, seen = 0, 0
    ep = np.zeros(E, np.float32)
    for ret, frames in iters:
        k1 = frames // E
        fin = []
        for k in range(k0, k1):
            ep = ep + rew[k].astype(np.float32)
            fin.extend(ep[ended[k]].tolist())
            ep[ended[k]] = 0
        assert ret == (float(np.sum(np.array(fin, np.float64)) / len(fin)) if fin else None)
        seen += len(fin)
        k0 = k1
    assert k0 == K and seen == ended.sum() and seen >= 3
    return iters


def _sac(**kw):
    args = dict(env_name="Hopper-v2", gamma=0.99, acm_critic=True, custom_loss=0.2, norm_closs=False,
                min_max_denormalize=True, denormalize_actor_out=True, buffer_size=10_000, device="cuda:0", seed=0,
                update_freq=50, grad_steps=50, acm_update_freq=1000, acm_update_batches=100, acm_batch_size=100,
                random_frames=60, loop_seed=3, max_batch=600)
    args.update(kw)
    return spprl.SAC_AcM(**args)


def test_fused_loop_records_what_the_envs_served():
    """SAC_AcM, six host envs with ragged limits (two of them also terminating early), 3 iterations of 10 vector
    steps, pipelined with the update."""
    envs = [_LogEnv(11, 3, T=5 + 3 * i, seed=i, early=i in (1, 4)) for i in range(6)]
    ag = _sac(env=HostVecEnv(envs, device="cuda:0"), batch_size=60, iterations=3)
    assert ag.schedule == "fused" and ag.max_ep_len is None
    iters = _run_and_check(ag, envs, vanilla=False)
    assert [f for _, f in iters] == [60, 120, 180]


def test_fused_vanilla_loop_masks_the_time_limit_done():
    """spprl.DDPG (max_ep_len set, Q3): done is 0 on the records that ended at the env_spec's time limit and 1 on
    early terminations; end is 1 on both."""
    T = 7
    envs = [_LogEnv(17, 6, T=T, seed=10 + i, early=i in (0, 2, 5)) for i in range(6)]
    ag = spprl.DDPG(env_name="HalfCheetah-v2", env_spec=(17, 6, 1.0, T), gamma=0.99, buffer_size=10_000,
                    device="cuda:0", seed=0, max_batch=600, update_freq=50, grad_steps=50, random_frames=60,
                    loop_seed=3, env=HostVecEnv(envs, device="cuda:0"), batch_size=60, iterations=3)
    assert ag.schedule == "fused" and ag.max_ep_len == T
    _run_and_check(ag, envs, vanilla=True)


def test_reference_schedule_records_what_the_env_served():
    """One env on the reference schedule: whole episodes per iteration, a reset through _start_episodes."""
    envs = [_LogEnv(11, 3, T=9, seed=21, early=True)]
    ag = _sac(env=HostVecEnv(envs, device="cuda:0"), batch_size=20, iterations=3, random_frames=10,
              update_freq=10, grad_steps=2, acm_update_freq=20, acm_update_batches=2, max_batch=128)
    assert ag.schedule == "reference"
    _run_and_check(ag, envs, vanilla=False)
