"""GPU parity of vanilla PPO (spprl.PPO, rltoolkit/algorithms/ppo/ppo.py on a2c.py): the fused rollout act
(sppOnpRolloutAct), the one-launch actor epoch at aout != ob, the Hopper (11, 3) shape, the running-statistics
kernel (sppOnpObsStats), the reference-generated fixture tests/golden/ppo_vanilla_hcheetah.npz and the loop.
Oracles: oracle/onpolicy.py and the restatement tests/ppo_ref.py.  Tolerances are those the existing on-policy
tests hold the same quantities to (tests/test_gpu_onpolicy.py), named at each use."""
import numpy as np
import pytest
import torch

import ppo_ref
import spprl
from oracle import onpolicy as oo
from spprl import _lib
from spprl.onpolicy import FUSED_ACT_MAX_ROWS, OnPolicyNets, obs_stats

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(17, 6), (11, 3), (3, 1)]


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def t(z):
    return torch.from_numpy(np.ascontiguousarray(z)).to(DEV)


def seeded_nets(ob, aout, seed, lim=1.0, **kw):
    n = OnPolicyNets(ob, aout, ac_lim=lim, device=DEV, **kw)
    a = oo.init_flat(oo.actor_layout(ob, aout), seed)
    a[:aout] += np.random.RandomState(seed).uniform(-0.3, 0.3, aout).astype(np.float32)
    c = oo.init_flat(oo.critic_layout(ob), seed + 1)
    n.load_net(0, a)
    n.load_net(1, c)
    return n, a, c


# ------------------------------------------------------------------ fused rollout act
@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "ob%d_ac%d" % s)
def act_nets(request):
    ob, aout = request.param
    lim = 2.0 if aout == 1 else 1.0  # (Pendulum's action high)
    n, a, _ = seeded_nets(ob, aout, 9, lim=lim, max_batch=512)
    return ob, aout, lim, n, a


@pytest.mark.parametrize("E", [1, 2, 3, 33, 65])
def test_fused_rollout_act(act_nets, E):
    """One launch (normalise, draw, forward from the canonical parameters, log-prob) against the float64-normalised
    oracle and the unfused sequence sppObsNormalize + sppRandNormal + sppOnpAct.  E = 1, 2, 3: a Philox group of
    four straddles rows for aout 6, 3, 1; E = 33, 65: more rows than a 32-sample tile / a wave.  Noise bit-equal to
    sppRandNormal's; normalised observations BIT-EQUAL to sppObsNormalize's (the same obs_norm1 arithmetic);
    actions rtol / atol 1e-5 and log-probs 1e-4 (test_act_sample_and_deterministic's bounds for k_onp_act)."""
    ob, aout, lim, n, a = act_nets
    assert E <= FUSED_ACT_MAX_ROWS
    rng = np.random.RandomState(100 * ob + E)
    mean = (rng.randn(ob) * 0.5 + 1.0).astype(np.float32)
    std = rng.uniform(0.5, 2.0, ob).astype(np.float32)
    x = (mean + std * rng.randn(E, ob) * 1.5).astype(np.float32)
    x[0, ob - 1] = mean[ob - 1] + 25.0 * std[ob - 1]  # beyond the +10 clip
    x[E - 1, 0] = mean[0] - 31.0 * std[0]             # and the -10 one
    seed, offset = 0x1234567890ABCDEF & ((1 << 63) - 1), 41 + E
    want_eps = torch.empty(E, aout, device=DEV)
    _lib.call("sppRandNormal", _lib.ptr(want_eps), E * aout, seed, offset, _lib.stream_handle())
    want_eps = want_eps.cpu().numpy()
    limv = np.full(aout, lim, np.float32)
    for stats in (True, False):
        m, s = (t(mean), t(std)) if stats else (None, None)
        if stats:
            xn_ref = ppo_ref.standardize_and_clip(x, mean, std).astype(np.float32)
            assert xn_ref[0, ob - 1] == 10.0 and xn_ref[E - 1, 0] == -10.0
            xn_dev = torch.empty(E, ob, device=DEV)
            _lib.call("sppObsNormalize", _lib.ptr(t(x)), E, ob, None, None, _lib.ptr(m), _lib.ptr(s), 0, 0,
                      _lib.ptr(xn_dev), _lib.stream_handle())
            xn_dev = xn_dev.cpu().numpy()
            np.testing.assert_allclose(xn_dev, xn_ref, rtol=1e-6, atol=1e-7)  # (three fp32 roundings)
        else:
            xn_ref = xn_dev = x
        for det in (False, True):
            act, lp, xn, eps = n.rollout_act(t(x), m, s, seed, offset, deterministic=det, fused=True, want_noise=True)
            act2, lp2, xn2, _ = n.rollout_act(t(x), m, s, seed, offset, deterministic=det, fused=False)
            torch.cuda.synchronize()
            what = "stats=%s det=%s" % (stats, det)
            np.testing.assert_array_equal(xn.cpu().numpy(), xn_dev, err_msg=what)  # bit-equal to sppObsNormalize
            np.testing.assert_array_equal(xn2.cpu().numpy(), xn_dev, err_msg=what)
            if det:
                assert not eps.cpu().numpy().any()
            else:
                np.testing.assert_array_equal(eps.cpu().numpy(), want_eps, err_msg=what)  # bit-equal draws
            want_a, want_lp = oo.act(a, ob, aout, limv, xn_ref, None if det else want_eps)
            for got_a, got_lp, path in ((act, lp, "fused"), (act2, lp2, "unfused")):
                np.testing.assert_allclose(got_a.cpu().numpy(), want_a, rtol=1e-5, atol=1e-5, err_msg=what + path)
                np.testing.assert_allclose(got_lp.cpu().numpy(), want_lp, rtol=1e-4, atol=1e-4, err_msg=what + path)
            np.testing.assert_allclose(act.cpu().numpy(), act2.cpu().numpy(), rtol=1e-5, atol=1e-5, err_msg=what)
            np.testing.assert_allclose(lp.cpu().numpy(), lp2.cpu().numpy(), rtol=1e-4, atol=1e-4, err_msg=what)


def test_fused_act_follows_the_parameters_and_the_env_switch(monkeypatch):
    """No packed images: a parameter change shows in the next call.  SPP_PPO_FUSED_ACT=0 and more rows than
    FUSED_ACT_MAX_ROWS take the unfused sequence (the noise output is then sppRandNormal's own buffer)."""
    n, a, _ = seeded_nets(17, 6, 4, max_batch=512)
    x = t(np.random.RandomState(1).randn(5, 17).astype(np.float32))
    a1 = n.rollout_act(x, None, None, 7, 1, deterministic=True)[0].cpu().numpy()
    n.params[0][6:].mul_(0.5)
    a2 = n.rollout_act(x, None, None, 7, 1, deterministic=True)[0].cpu().numpy()
    b = a.copy()
    b[6:] *= 0.5
    np.testing.assert_allclose(a2, oo.act(b, 17, 6, np.ones(6, np.float32), x.cpu().numpy())[0], rtol=1e-5, atol=1e-5)
    assert np.abs(a1 - a2).max() > 1e-3
    calls = []
    real = _lib.call
    monkeypatch.setattr("spprl.onpolicy.call", lambda name, *args: (calls.append(name), real(name, *args))[1])
    n.rollout_act(x, None, None, 7, 1)
    assert calls == ["sppOnpRolloutAct"]
    del calls[:]
    monkeypatch.setenv("SPP_PPO_FUSED_ACT", "0")
    n.rollout_act(x, None, None, 7, 1)
    assert calls == ["sppRandNormal", "sppOnpAct"]
    monkeypatch.delenv("SPP_PPO_FUSED_ACT")
    del calls[:]
    big = t(np.zeros((FUSED_ACT_MAX_ROWS + 1, 17), np.float32))
    n.rollout_act(big, x[0], x[1].abs() + 1, 7, 1)
    assert calls == ["sppObsNormalize", "sppRandNormal", "sppOnpAct"]


# ------------------------------------------------------------------ one-launch actor epoch, aout != ob
@pytest.mark.parametrize("ob,aout", [(17, 6), (11, 3)])
@pytest.mark.parametrize("N,mb", [(300, 64), (2050, 512)])
def test_actor_epoch_kernel_vanilla_shapes(ob, aout, N, mb):
    """The scheme of test_actor_epoch_kernel_matches_per_step_path_and_oracle with next_obs = None: (300, 64) one
    workgroup with a ragged last step, (2050, 512) eight workgroups with a last minibatch of 2 rows.  One launch
    per epoch against the per-minibatch path and the oracle's epoch loop (ppo_ref.update_actor on
    oracle.onpolicy.actor_step) on the same permutations: losses rtol 1e-4, parameters within 2 lr per Adam step,
    mean <= 0.01 lr (that test's tolerances); KL rtol 1e-3 with the fp32 resolution of the log-probs as the absolute
    term (worked out below)."""
    lr, ent = 3e-4, 0.01
    rng = np.random.RandomState(N + mb + ob)
    a0 = oo.init_flat(oo.actor_layout(ob, aout), 21)
    a0[:aout] += rng.uniform(-0.3, 0.3, aout).astype(np.float32)
    lim = np.ones(aout, np.float32)
    x = (rng.randn(N, ob) * 1.2).astype(np.float32)
    act = rng.uniform(-1.1, 1.1, (N, aout)).astype(np.float32)
    with torch.no_grad():
        lp_cur = oo.actor_dist(oo._params(a0, oo.actor_layout(ob, aout)), torch.from_numpy(x),
                               torch.ones(aout)).log_prob(torch.from_numpy(act)).numpy()
    lp_old = (lp_cur + 0.2 * rng.randn(N)).astype(np.float32)
    adv = rng.randn(N).astype(np.float32)
    adv = ((adv - adv.mean()) / adv.std()).astype(np.float32)  # already normalised (normalize_adv off)
    res = []
    for one_launch in (True, False):
        n = OnPolicyNets(ob, aout, ac_lim=1.0, actor_lr=lr, entropy_coef=ent, max_ppo_epochs=2, ppo_batch_size=mb,
                         kl_div_threshold=1e9, normalize_adv=False, max_batch=max(N, 512), device=DEV)
        n.load_net(0, a0)
        if one_launch:
            assert n._epoch_kernel_ok(mb)
        else:
            n._epoch_max_bs = 0
            assert not n._epoch_kernel_ok(mb)
        kl = n.update_actor(adv, x, act, lp_old, None, generator=torch.Generator().manual_seed(7))
        torch.cuda.synchronize()
        if one_launch:
            n.check_actor_epochs()
        assert "dist" not in n.loss and "policy" not in n.loss
        res.append((n.params[0].cpu().numpy().copy(), dict(n.loss), dict(n.loss_sums), kl))
    g = torch.Generator().manual_seed(7)
    perms = [torch.randperm(N, generator=g).numpy() for _ in range(2)]
    flat, sums, kls, cnt = ppo_ref.update_actor(a0, ob, aout, lim, x, act, lp_old, adv, lr, 2, 1e9, mb,
                                                entropy_coef=ent, perms=perms)
    nsteps = 2 * -(-N // mb)
    assert cnt == 2
    # The KL is the mean of lp_old - lp_new over the LAST minibatch (2 rows at N = 2050), a difference of fp32
    # log-probs of magnitude |lp| (tens here: aout quadratic terms of up to (2.1 / sigma)^2 / 2 each).  One fp32
    # evaluation of lp_new rounds each of the aout terms three times (sub, mul, div) and the running sum aout
    # times, so two correct fp32 evaluations (the kernel's, the float32 oracle's) differ by up to about
    # (3 + aout) 2^-24 max|lp| per row, and so does their mean: that, on top of that test's floor of 2e-6.
    kl_abs = 2e-6 + (3 + aout) * 2.0 ** -24 * float(np.abs(lp_old).max())
    print("max |lp_old| %.1f: KL abs tolerance %.3g" % (np.abs(lp_old).max(), kl_abs))
    for p, loss, loss_sums, kl in res:
        for k in ("actor", "entropy", "sum"):
            assert loss_sums[k] == pytest.approx(sums[k], rel=1e-4, abs=1e-6), (k, loss_sums[k], sums[k])
        for k in ("actor", "entropy"):  # OnPolicyNets.loss itself is unchanged: divided by i + 1 = 2
            assert loss[k] == pytest.approx(sums[k] / 2, rel=1e-4, abs=1e-6), k
        assert kl == pytest.approx(kls[-1], rel=1e-3, abs=kl_abs), (kl, kls[-1], kl_abs)
        d = np.abs(p - flat)
        print("(%d, %d) N %d mb %d: |d|/lr max %.4f mean %.6f" % (ob, aout, N, mb, d.max() / lr, d.mean() / lr))
        assert d.max() <= 2 * lr * nsteps * 1.01 and d.mean() <= 0.01 * lr, (d.max(), d.mean())


def test_spp_ppo_epoch_shapes_unchanged():
    """(17, 17) and (11, 11) still have their one-launch epoch; a shape without an instantiation has none."""
    for ob, aout, ok in ((17, 17, True), (11, 11, True), (17, 6, True), (11, 3, True), (3, 1, False)):
        n = OnPolicyNets(ob, aout, max_batch=512, device=DEV)
        assert n._epoch_kernel_ok(64) == ok, (ob, aout)


# ------------------------------------------------------------------ Hopper (11, 3)
@pytest.fixture(scope="module")
def hopper():
    return seeded_nets(11, 3, 3, max_batch=512, entropy_coef=0.01)


@pytest.mark.parametrize("N", [1, 77, 500])
def test_hopper_value_and_critic_grad(hopper, N):
    """test_value_and_critic_grad's checks and tolerances at (ob, aout) = (11, 3)."""
    n, a, c = hopper
    rng = np.random.RandomState(N)
    x = (rng.randn(N, 11) * 1.5).astype(np.float32)
    q = rng.randn(N).astype(np.float32)
    v = n.value(x).cpu().numpy()
    with torch.no_grad():
        want = oo.critic(oo._params(c, oo.critic_layout(11)), torch.from_numpy(x)).squeeze(-1).numpy()
    np.testing.assert_allclose(v, want, rtol=1e-5, atol=1e-5)
    xd, qd = t(x), t(q)
    loss = torch.zeros(1, device=DEV)
    _lib.call("sppOnpCriticGrads", n._h, _lib.ptr(xd), _lib.ptr(qd), N, _lib.ptr(loss), _lib.stream_handle())
    torch.cuda.synchronize()
    l_ref, g_ref = oo.critic_step(c, 11, x, q)
    assert loss.item() == pytest.approx(l_ref, rel=1e-5)
    assert relerr(n.grads[1].cpu().numpy(), g_ref) < 2e-5


@pytest.mark.parametrize("N", [1, 77, 500])
def test_hopper_actor_grad(hopper, N):
    """test_actor_grad_clip_entropy's checks and tolerances at (11, 3), with no next obs (dist = 0)."""
    n, a, c = hopper
    ob, aout = 11, 3
    rng = np.random.RandomState(N + 1)
    x = (rng.randn(N, ob) * 1.2).astype(np.float32)
    act = rng.uniform(-1.2, 1.2, (N, aout)).astype(np.float32)
    with torch.no_grad():
        lp_cur = oo.actor_dist(oo._params(a, oo.actor_layout(ob, aout)), torch.from_numpy(x),
                               torch.ones(aout)).log_prob(torch.from_numpy(act)).numpy()
    lp_old = (lp_cur + rng.randn(N).astype(np.float32) * 0.2).astype(np.float32)  # ratios around 1 (both branches)
    adv = rng.randn(N).astype(np.float32)
    xd, ad, ld, vd = t(x), t(act), t(lp_old), t(adv)
    out = torch.zeros(4, device=DEV)
    _lib.call("sppOnpActorGrads", n._h, _lib.ptr(xd), _lib.ptr(ad), _lib.ptr(ld), _lib.ptr(vd), None, N,
              _lib.ptr(out), _lib.stream_handle())
    torch.cuda.synchronize()
    ref, g_ref = oo.actor_step(a, ob, aout, np.ones(aout, np.float32), x, act, lp_old, adv, entropy_coef=0.01)
    o = out.cpu().numpy()
    assert o[0] == pytest.approx(ref["actor"], rel=1e-4, abs=1e-6)
    assert o[1] == pytest.approx(ref["kl"], rel=1e-4, abs=1e-5)
    assert o[2] == 0.0
    assert o[3] == pytest.approx(ref["entropy"], rel=1e-5)
    g = n.grads[0].cpu().numpy()
    assert relerr(g, g_ref) < 2e-4, relerr(g, g_ref)
    np.testing.assert_allclose(g[:aout], g_ref[:aout], rtol=1e-3, atol=1e-6)  # log_scale


# ------------------------------------------------------------------ running statistics
@pytest.mark.parametrize("rows,starts", [(7, 1), (96, 3), (2999, 4)])
@pytest.mark.parametrize("alpha", [0.0, 0.95, 1.0])
def test_obs_stats_kernel(rows, starts, alpha):
    """sppOnpObsStats against ppo_ref.update_obs_mean_std (float64): mean / std rtol 1e-6 (a constant column's std
    is exactly 0 before the blend); percentiles EXACT: the float32 rounding of numpy's float64 np.percentile.  A
    second call takes the running max / min."""
    ob = 17
    rng = np.random.RandomState(rows + int(100 * alpha))
    offs = rng.uniform(0.5, 2.0, ob) * rng.choice([-1.0, 1.0], ob)
    scale = rng.uniform(0.3, 2.5, ob)
    start = (offs + scale * rng.randn(starts, ob)).astype(np.float32)
    nxt = (offs + scale * rng.randn(rows, ob)).astype(np.float32)
    obs = (offs + scale * rng.randn(rows, ob)).astype(np.float32)
    start[:, 5] = nxt[:, 5] = obs[:, 5] = np.float32(0.7)  # a constant column
    obs[: rows // 2, 9] = obs[0, 9]                          # ties around the order statistics
    mean0 = (rng.randn(ob) * 0.3 + offs).astype(np.float32)
    std0 = rng.uniform(0.5, 1.5, ob).astype(np.float32)
    mean, std = t(mean0), t(std0)
    mx, mn = torch.zeros(ob, device=DEV), torch.zeros(ob, device=DEV)
    keep = obs_stats(t(start), t(nxt), t(obs), alpha, mean, std, mx, mn, False)
    torch.cuda.synchronize()
    wm, ws, wmx, wmn = ppo_ref.update_obs_mean_std(start, nxt, obs, alpha, mean0, std0)
    np.testing.assert_allclose(mean.cpu().numpy(), wm, rtol=1e-6)
    np.testing.assert_allclose(std.cpu().numpy(), ws, rtol=1e-6)
    assert ws[5] == alpha * std0[5] or alpha not in (0.0, 1.0)
    np.testing.assert_array_equal(mx.cpu().numpy(), wmx)
    np.testing.assert_array_equal(mn.cpu().numpy(), wmn)
    # the second iteration: other rows, blended from the first's statistics; running max / min
    obs2 = (obs * np.float32(0.5)).astype(np.float32)
    m1, s1 = mean.cpu().numpy().copy(), std.cpu().numpy().copy()
    keep = obs_stats(t(start), t(obs2), t(obs2), alpha, mean, std, mx, mn, True)
    torch.cuda.synchronize()
    wm, ws, wmx, wmn = ppo_ref.update_obs_mean_std(start, obs2, obs2, alpha, m1, s1, wmx, wmn)
    np.testing.assert_allclose(mean.cpu().numpy(), wm, rtol=1e-6)
    np.testing.assert_allclose(std.cpu().numpy(), ws, rtol=1e-6)
    np.testing.assert_array_equal(mx.cpu().numpy(), wmx)
    np.testing.assert_array_equal(mn.cpu().numpy(), wmn)
    del keep


# ------------------------------------------------------------------ the reference fixture
@pytest.mark.parametrize("epoch_kernel", ["0", "1"])
def test_update_matches_reference_fixture(epoch_kernel, monkeypatch):
    """Per-minibatch actor steps (the default) and SPP_PPO_EPOCH_KERNEL=1 (one-launch epochs).  spprl.PPO.update(mem) on the fixture's memory (three rollouts, 96 raw frames): statistics rtol 1e-5; critic
    loss rtol 1e-4, critic parameters rtol 1e-4 / atol 5e-6; advantages 1e-4 / 1e-4; epochs run and the counter
    exact; KL rtol 1e-4 / abs 2e-5; loss sums rtol 1e-4; actor parameters within 2 lr per Adam step, mean <= 0.02 lr
    (the bounds of the existing reference-fixture tests, tests/test_gpu_onpolicy.py)."""
    monkeypatch.setenv("SPP_PPO_EPOCH_KERNEL", epoch_kernel)
    fx, actor, critic, mem = ppo_ref.ppo_vanilla_case()
    lr = float(fx["actor_lr"])
    ag = spprl.PPO("HalfCheetah-v2", gamma=float(fx["gamma"]), actor_lr=lr, critic_lr=float(fx["critic_lr"]),
                   epsilon=float(fx["eps"]), gae_lambda=float(fx["gae_lambda"]),
                   kl_div_threshold=float(fx["threshold"]), max_ppo_epochs=int(fx["max_epochs"]),
                   ppo_batch_size=int(fx["ppo_batch_size"]), entropy_coef=float(fx["entropy_coef"]),
                   critic_num_target_updates=int(fx["critic_num_target_updates"]),
                   num_critic_updates_per_target=int(fx["num_critic_updates_per_target"]),
                   obs_norm_alpha=float(fx["obs_norm_alpha"]), device=DEV, seed=0)
    ag.nets.load_net(0, actor)
    ag.nets.load_net(1, critic)
    N = len(mem["obs"])
    assert ag.nets._epoch_kernel_ok(N) == (epoch_kernel == "1") and ag.nets._critic_kernel_ok(N)
    ag.update({k: (v[:, None] if k in ("obs", "next_obs", "act", "lp", "rew", "done", "end") else v)
               for k, v in mem.items()})
    torch.cuda.synchronize()
    ag.nets.check_actor_epochs()
    d = ag.collect_params_dict()
    for k in ("obs_mean", "obs_std", "max_obs", "min_obs"):
        np.testing.assert_allclose(d[k].numpy(), fx[k], rtol=1e-5, err_msg=k)
    assert ag.loss["critic"] == pytest.approx(float(fx["crit_loss"]), rel=1e-4)
    np.testing.assert_allclose(ag.nets.params[1].cpu().numpy(), fx["crit_post"], rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(ag.last_advantages.reshape(-1).cpu().numpy(), fx["adv"], rtol=1e-4, atol=1e-4)
    assert ag.nets.last_epochs == len(fx["kls"]) == 3
    assert ag.kl_div_updates_counter == int(fx["counter"]) == 4
    assert ag.nets.loss["kl"] == pytest.approx(float(fx["kls"][-1]), rel=1e-4, abs=2e-5)
    assert set(ag.loss) == {"actor", "entropy", "sum", "critic"}
    for j, k in enumerate(("actor", "entropy", "sum")):
        assert ag.loss[k] == pytest.approx(float(fx["losses"][j]), rel=1e-4), k
    dp = np.abs(ag.nets.params[0].cpu().numpy() - fx["actor_post"])
    print("|d|/lr max %.4f mean %.5f" % (dp.max() / lr, dp.mean() / lr))
    assert dp.max() <= 2 * lr * 3 * 1.01 and dp.mean() <= 0.02 * lr, (dp.max(), dp.mean())


# ------------------------------------------------------------------ the loop
def _agent(n_envs, **kw):
    return spprl.PPO("HalfCheetah-v2", batch_size=200, ppo_batch_size=64, max_ppo_epochs=2, iterations=2, seed=0,
                     n_envs=n_envs, device=DEV, **kw)


@pytest.mark.parametrize("n_envs", [1, 4])
def test_loop_smoke_fused_and_unfused(n_envs, monkeypatch, tmp_path):
    first = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("SPP_PPO_FUSED_ACT", fused)
        ag = _agent(n_envs)
        assert isinstance(ag.env, spprl.SynthVecEnv) and ag.obs_norm_alpha == 0.99
        mem = ag.collect_batch()  # the first iteration by hand: its first step is compared below
        first[fused] = (mem["obs"][0].cpu().numpy(), mem["act"][0].cpu().numpy(), mem["lp"][0].cpu().numpy())
        ag.update(mem)
        ag.iteration += 1
        ag.train()  # the second
        torch.cuda.synchronize()
        per_iter = 1000 if n_envs == 1 else 200  # whole 1000-frame episodes / T = 50 lockstep steps of 4 envs
        assert ag.iteration == 2 and ag.stats_logger.frames == 2 * per_iter
        assert mem["obs"].shape == (per_iter // n_envs, n_envs, 17) and mem["start_obs"].shape == (n_envs, 17)
        assert int(mem["end"].sum()) == n_envs and int(mem["done"].sum()) == 0  # time limit / truncation: not done
        assert all(torch.isfinite(p).all() for p in ag.nets.params)
        assert all(np.isfinite(v) for v in ag.loss.values()) and set(ag.loss) == {"actor", "entropy", "sum", "critic"}
        d = ag.collect_params_dict()
        assert list(d) == ["actor", "critic", "obs_mean", "obs_std", "min_obs", "max_obs"]  # rl.py:263-271
        assert list(d["actor"])[0] == "log_scale" and not torch.equal(d["obs_std"], torch.ones(17))
        path = str(tmp_path / ("ppo%s.pt" % fused))
        ag.save(path)
        other = _agent(n_envs, loop_seed=5)
        other.load(path)
        d2 = other.collect_params_dict()
        for k in ("actor", "critic"):
            for name in d[k]:
                assert torch.equal(d[k][name], d2[k][name]), (k, name)
        for k in ("obs_mean", "obs_std", "min_obs", "max_obs"):
            assert torch.equal(d[k], d2[k]), k
        with pytest.raises(AttributeError):
            ag.pre_train()
    # the same env seed and the same draws: the first step's observation is identical, its action and log-prob
    # agree to the act tolerances
    np.testing.assert_array_equal(first["1"][0], first["0"][0])
    np.testing.assert_allclose(first["1"][1], first["0"][1], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(first["1"][2], first["0"][2], rtol=1e-4, atol=1e-4)


def test_no_normaliser_and_test_episodes():
    ag = spprl.PPO("Hopper-v2", batch_size=64, ppo_batch_size=64, max_ppo_epochs=1, iterations=1, seed=1, n_envs=8,
                   obs_norm_alpha=None, test_episodes=2, device=DEV)
    ag.train()
    d = ag.collect_params_dict()
    assert d["obs_mean"] is None and d["obs_std"] is None and d["min_obs"] is None  # memory.py:84-85: nothing updated
    assert np.isfinite(ag.stats_logger.test_return)
