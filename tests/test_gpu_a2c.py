"""GPU parity of A2C / A2C_AcM (spprl.A2C, spprl.A2C_AcM; rltoolkit/algorithms/a2c/a2c.py, acm/on_policy.py): the
one-launch TD advantage with its moments (sppOnpTdAdvantage), the policy-gradient actor step (sppOnpPgActorGrads),
the two reference-generated fixtures and the loops.  Oracle: the restatement tests/a2c_ref.py in float64.

Row counts: 1 (one lane live), 33 (a tile and one row), 77, 130 (a fifth tile: a second workgroup at 4 waves per
workgroup).  A wave takes a SECOND tile only when the tiles outnumber 4 waves x 2 workgroups per CU x the device's
CUs -- 2048 tiles, 65536 rows on 256 CUs -- which is not reachable below a few thousand rows; that stride loop is
the one every k_onp_* kernel shares."""
import numpy as np
import pytest
import torch

import a2c_ref
import spprl
from oracle import onpolicy as oo
from spprl import _lib
from spprl.onpolicy import OnPolicyNets

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAIRS = [(17, 6), (11, 3), (17, 17), (11, 11)]
ROWS = [1, 33, 77, 130]
F64 = torch.float64


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def t(z):
    return torch.from_numpy(np.ascontiguousarray(z)).to(DEV)


@pytest.fixture(scope="module", params=PAIRS, ids=lambda s: "ob%d_aout%d" % s)
def nets(request):
    ob, aout = request.param
    n = OnPolicyNets(ob, aout, ac_lim=1.0, gamma=0.97, max_batch=1024, device=DEV)
    a = oo.init_flat(oo.actor_layout(ob, aout), 13)
    a[:aout] += np.random.RandomState(13).uniform(-0.3, 0.3, aout).astype(np.float32)
    c = oo.init_flat(oo.critic_layout(ob), 14)
    n.load_net(0, a)
    n.load_net(1, c)
    return ob, aout, n, a, c


def _td_call(n, x, xn, rew, done, N, q, adv, mom):
    _lib.call("sppOnpTdAdvantage", n._h, _lib.ptr(x), _lib.ptr(xn), _lib.ptr(rew), _lib.ptr(done), N, 0.97,
              _lib.ptr(q), _lib.ptr(adv), _lib.ptr(mom), _lib.stream_handle())
    torch.cuda.synchronize()


# ------------------------------------------------------------------ (a) the TD advantage
@pytest.mark.parametrize("N", ROWS)
def test_td_advantage_matches_float64_restatement(nets, N):
    """adv and q rtol 1e-4 / atol 1e-4 (the fixture tests' advantages bound) against float64; done a mix of 0 and 1;
    q_out and moments2 each also NULL (adv then bit-equal to the full call's)."""
    ob, aout, n, _, c = nets
    rng = np.random.RandomState(N + ob)
    x, xn = (rng.randn(N, ob) * 1.3).astype(np.float32), (rng.randn(N, ob) * 1.3).astype(np.float32)
    rew = rng.randn(N).astype(np.float32)
    done = (np.arange(N) % 3 == 0).astype(np.float32) if N > 1 else np.ones(1, np.float32)
    want_adv, want_q = a2c_ref.td_advantage(c.astype(np.float64), ob, x, xn, rew, done, 0.97, F64)
    xd, xnd, rd, dd = t(x), t(xn), t(rew), t(done)
    q, adv, mom = (torch.full((k,), 7.0, device=DEV) for k in (N, N, 2))
    _td_call(n, xd, xnd, rd, dd, N, q, adv, mom)
    np.testing.assert_allclose(adv.cpu().numpy(), want_adv, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(q.cpu().numpy(), want_q, rtol=1e-4, atol=1e-4)
    if N > 1:
        a64 = adv.cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(mom.cpu().numpy(), [a64.mean(), a64.std(ddof=1)], rtol=1e-5)
    else:
        assert mom[0].item() == adv[0].item() and np.isnan(mom[1].item())  # torch.std of one element
    adv2, adv3 = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    _td_call(n, xd, xnd, rd, dd, N, None, adv2, mom)
    _td_call(n, xd, xnd, rd, dd, N, q, adv3, None)
    assert torch.equal(adv2, adv) and torch.equal(adv3, adv)


# ------------------------------------------------------------------ (b) the moments
@pytest.mark.parametrize("N", [2, 33, 130, 1000])
def test_moments_survive_a_mean_far_above_the_spread(N):
    """Rewards 1000 + 0.01 noise and a zeroed critic: adv ~ 1000 with spread 0.01.  mean rtol 1e-6, std rtol 1e-3
    against float64 numpy on the float32 adv the kernel wrote (only the reduction is judged)."""
    ob = 17
    n = OnPolicyNets(ob, 6, max_batch=1024, gamma=0.97, device=DEV)
    n.params[1].zero_()
    rng = np.random.RandomState(N)
    x, xn = t(rng.randn(N, ob).astype(np.float32)), t(rng.randn(N, ob).astype(np.float32))
    rew = (1000.0 + 0.01 * rng.randn(N)).astype(np.float32)
    adv, mom = torch.zeros(N, device=DEV), torch.zeros(2, device=DEV)
    _td_call(n, x, xn, t(rew), t(np.zeros(N, np.float32)), N, None, adv, mom)
    a = adv.cpu().numpy()
    np.testing.assert_array_equal(a, rew)  # V = 0 exactly
    a64 = a.astype(np.float64)
    m = mom.cpu().numpy()
    print("N %d: mean %.9g (want %.9g), std %.6g (want %.6g)" % (N, m[0], a64.mean(), m[1], a64.std(ddof=1)))
    np.testing.assert_allclose(m[0], a64.mean(), rtol=1e-6)
    np.testing.assert_allclose(m[1], a64.std(ddof=1), rtol=1e-3)


# ------------------------------------------------------------------ (c) the actor step's gradient
@pytest.mark.parametrize("N", ROWS)
def test_pg_actor_grads_match_float64_restatement(nets, N):
    """With and without moments2 (N = 1 only without: the std of one element is NaN in the reference too), with and
    without dist_act / next_obs.  Losses rtol 1e-4; per layout tensor ||g - g_ref|| / ||g_ref|| < 2e-4 (DESIGN.md
    §2); log_scale rtol 1e-3 / atol 1e-6 (test_hopper_actor_grad's bound)."""
    ob, aout, n, a, _ = nets
    rng = np.random.RandomState(7 * N + aout)
    lim = np.ones(aout, np.float32)
    x = (rng.randn(N, ob) * 1.2).astype(np.float32)
    act = rng.uniform(-1.2, 1.2, (N, aout)).astype(np.float32)
    adv = (rng.randn(N) * 2 + 0.5).astype(np.float32)
    dact = rng.uniform(-2, 2, (N, aout)).astype(np.float32)
    nxt = rng.randn(N, aout).astype(np.float32)
    xd, ad, vd, dd, nd = t(x), t(act), t(adv), t(dact), t(nxt)
    for use_mom in ((False, True) if N > 1 else (False,)):
        a64 = adv.astype(np.float64)
        mom = np.array([a64.mean(), a64.std(ddof=1)], np.float32) if use_mom else None
        hat = (a64 - np.float64(mom[0])) / (np.float64(mom[1]) + 1e-8) if use_mom else a64
        md = t(mom) if use_mom else None
        for dist_act, next_obs in ((None, None), (None, nd), (dd, nd)):
            what = "moments=%s dist_act=%s next_obs=%s" % (use_mom, dist_act is not None, next_obs is not None)
            out = torch.full((4,), 7.0, device=DEV)
            n.grads[0].fill_(3.0)
            _lib.call("sppOnpPgActorGrads", n._h, _lib.ptr(xd), _lib.ptr(ad), _lib.ptr(vd), _lib.ptr(md),
                      _lib.ptr(dist_act), _lib.ptr(next_obs), N, _lib.ptr(out), _lib.stream_handle())
            torch.cuda.synchronize()
            ref, g_ref = a2c_ref.pg_actor_grad(a.astype(np.float64), ob, aout, lim, x, act, hat,
                                               None if dist_act is None else dact,
                                               None if next_obs is None else nxt, dtype=F64)
            o = out.cpu().numpy()
            assert o[0] == pytest.approx(ref["actor"], rel=1e-4), what
            assert o[1] == pytest.approx(ref["logp"], rel=1e-4), what
            assert o[2] == (pytest.approx(ref["dist"], rel=1e-4) if next_obs is not None else 0.0), what
            assert o[3] == pytest.approx(ref["entropy"], rel=1e-4), what
            g, off = n.grads[0].cpu().numpy(), 0
            for name, shape in oo.actor_layout(ob, aout):
                k = int(np.prod(shape))
                if name != "log_scale":
                    e = relerr(g[off:off + k], g_ref[off:off + k])
                    assert e < 2e-4, (what, name, e)
                off += k
            np.testing.assert_allclose(g[:aout], g_ref[:aout], rtol=1e-3, atol=1e-6, err_msg=what)


# ------------------------------------------------------------------ (d) the vanilla fixture
def _vanilla_agent(fx):
    ag = spprl.A2C("HalfCheetah-v2", gamma=float(fx["gamma"]), actor_lr=float(fx["actor_lr"]),
                   critic_lr=float(fx["critic_lr"]), critic_num_target_updates=int(fx["critic_num_target_updates"]),
                   num_critic_updates_per_target=int(fx["num_critic_updates_per_target"]),
                   obs_norm_alpha=float(fx["obs_norm_alpha"]), device=DEV, seed=0)
    mean0, std0 = a2c_ref.vanilla_start_stats(int(fx["seed"]), 17)
    ag.obs_mean.copy_(t(mean0))
    ag.obs_std.copy_(t(std0))
    return ag


def _as_mem(mem):
    return {k: (v[:, None] if k in ("obs", "next_obs", "act", "rew", "done", "end") else v) for k, v in mem.items()}


def test_update_matches_reference_fixture():
    """spprl.A2C.update(mem) on the fixture's memory: statistics rtol 1e-5; critic loss rtol 1e-4, parameters rtol
    1e-4 / atol 5e-6; advantages 1e-4 / 1e-4; actor loss rtol 1e-4; actor parameters within 2 lr, mean <= 0.02 lr
    (test_gpu_ppo_vanilla.test_update_matches_reference_fixture's bounds).  Then the WRONG order -- the actor on
    observations normalised with the updated statistics -- misses the fixture's actor loss by more than 10x that
    tolerance (tests/test_a2c_ref_golden.py shows the fixture has this separation)."""
    fx, actor, critic, mem = a2c_ref.a2c_vanilla_case()
    lr = float(fx["actor_lr"])
    losses = []
    for wrong in (False, True):
        ag = _vanilla_agent(fx)
        ag.nets.load_net(0, actor)
        ag.nets.load_net(1, critic)
        if wrong:
            ag.actor_observations = lambda raw, m, s: ag.normalize(raw)  # noqa: B023
        ag.update(_as_mem(mem))
        torch.cuda.synchronize()
        losses.append(ag.loss["actor"])
        if wrong:
            break
        assert set(ag.loss) == {"actor", "critic"}
        d = ag.collect_params_dict()
        for k in ("obs_mean", "obs_std", "max_obs", "min_obs"):
            np.testing.assert_allclose(d[k].numpy(), fx[k], rtol=1e-5, err_msg=k)
        assert ag.loss["critic"] == pytest.approx(float(fx["crit_loss"]), rel=1e-4)
        np.testing.assert_allclose(ag.nets.params[1].cpu().numpy(), fx["crit_post"], rtol=1e-4, atol=5e-6)
        np.testing.assert_allclose(ag.last_advantages.cpu().numpy(), fx["adv"], rtol=1e-4, atol=1e-4)
        assert ag.loss["actor"] == pytest.approx(float(fx["actor_loss"]), rel=1e-4)
        dp = np.abs(ag.nets.params[0].cpu().numpy() - fx["actor_post"])
        print("|d|/lr max %.4f mean %.5f" % (dp.max() / lr, dp.mean() / lr))
        assert dp.max() <= 2 * lr * 1.01 and dp.mean() <= 0.02 * lr, (dp.max(), dp.mean())
    want = float(fx["actor_loss"])
    print("actor loss %.6g, with the new statistics %.6g, fixture %.6g" % (losses[0], losses[1], want))
    assert abs(losses[1] - want) > 10 * 1e-4 * abs(want)


# ------------------------------------------------------------------ (e) the AcM fixture
def test_acm_two_updates_match_reference_fixture():
    """spprl.A2C_AcM.update through the fixture's two memories: losses rtol 1e-4, advantages 1e-4 / 1e-4, critic
    parameters rtol 1e-4 / atol 5e-6 after the first update, actor parameters within 2 lr per Adam step after each.
    The second step applies g1 + g2 (update_actor_acm never zeroes the gradient)."""
    fx, actor, critic, mems, lo, hi = a2c_ref.a2c_acm_case()
    lr, ob = float(fx["actor_lr"]), 17
    ag = spprl.A2C_AcM("HalfCheetah-v2", gamma=float(fx["gamma"]), actor_lr=lr, critic_lr=float(fx["critic_lr"]),
                       critic_num_target_updates=int(fx["critic_num_target_updates"]),
                       num_critic_updates_per_target=int(fx["num_critic_updates_per_target"]),
                       custom_loss=float(fx["custom_loss"]), norm_closs=False, denormalize_actor_out=True,
                       min_max_denormalize=True, acm_pre_train_samples=200, batch_size=96, device=DEV, seed=0)
    ag.nets.load_net(0, actor)
    ag.nets.load_net(1, critic)
    rb = ag.replay_buffer
    rb.min_obs.copy_(t(lo))
    rb.max_obs.copy_(t(hi))
    rb._have_minmax = True
    g1 = None
    for k, mem in enumerate(mems, 1):
        N = len(mem["obs"])
        m = {"obs": ag.normalize(t(mem["obs"])).reshape(N, 1, ob), "next_obs": t(mem["next_obs"]).reshape(N, 1, ob),
             "act": t(mem["act"]).reshape(N, 1, ob), "rew": t(mem["rew"]).reshape(N, 1),
             "done": t(mem["done"].astype(np.uint8)).reshape(N, 1), "T": N, "E": 1}
        np.testing.assert_allclose(m["obs"].reshape(N, ob).cpu().numpy(),
                                   a2c_ref.minmax_normalize(mem["obs"], lo, hi), rtol=1e-5, atol=1e-6)
        ag.update(m)
        torch.cuda.synchronize()
        assert set(ag.loss) == {"actor", "critic", "dist", "policy", "acm"}
        assert ag.loss["critic"] == pytest.approx(float(fx["crit_loss%d" % k]), rel=1e-4)
        np.testing.assert_allclose(ag.last_advantages.cpu().numpy(), fx["adv%d" % k], rtol=1e-4, atol=1e-4)
        for j, name in enumerate(("actor", "dist", "policy")):
            assert ag.loss[name] == pytest.approx(float(fx["losses%d" % k][j]), rel=1e-4), (k, name)
        if k == 1:
            np.testing.assert_allclose(ag.nets.params[1].cpu().numpy(), fx["crit_post1"], rtol=1e-4, atol=5e-6)
            g1 = ag.nets.grads[0].clone()
        dp = np.abs(ag.nets.params[0].cpu().numpy() - fx["actor_post%d" % k])
        print("step %d: |d|/lr max %.4f mean %.5f" % (k, dp.max() / lr, dp.mean() / lr))
        assert dp.max() <= 2 * lr * k * 1.01, (k, dp.max(), dp.mean())
    assert torch.equal(ag.nets.grads[0], ag._actor_grad_sum) and not torch.equal(ag.nets.grads[0], g1)


# ------------------------------------------------------------------ (f) the loops
def _loop_checks(ag, make, tmp_path, frames, keys):
    torch.cuda.synchronize()
    assert ag.iteration == 2 and ag.stats_logger.frames == frames, ag.stats_logger.frames
    assert set(ag.loss) == keys and all(np.isfinite(v) for v in ag.loss.values() if v is not None), ag.loss
    assert all(torch.isfinite(p).all() for p in ag.nets.params)
    path = str(tmp_path / "a2c.pt")
    ag.save(path)
    other = make(loop_seed=5)
    other.load(path)
    x = t(np.random.RandomState(3).randn(5, ag.ob_dim).astype(np.float32))
    if isinstance(ag, spprl.A2C):
        got = [o.nets.rollout_act(x, o.obs_mean, o.obs_std, 0, 0, deterministic=True)[0] for o in (ag, other)]
    else:
        got = [o.nets.act(o.normalize(x), None)[0] for o in (ag, other)]
    assert torch.equal(got[0], got[1])


def _fused_and_unfused_agree(ag, obs, nobs, rew, done, monkeypatch):
    """The one-launch advantage against SPP_A2C_FUSED_ADV=0 (two sppOnpValue launches, torch arithmetic, moments by
    torch): rtol 1e-5 / atol 1e-5."""
    calls = []
    real = _lib.call
    monkeypatch.setattr("spprl.onpolicy.call", lambda name, *args: (calls.append(name), real(name, *args))[1])
    adv, mom = ag.nets.td_advantage(obs, nobs, rew, done)
    assert calls == ["sppOnpTdAdvantage"]
    del calls[:]
    monkeypatch.setenv("SPP_A2C_FUSED_ADV", "0")
    adv0, mom0 = ag.nets.td_advantage(obs, nobs, rew, done)
    assert calls == ["sppOnpValue", "sppOnpValue"]
    monkeypatch.undo()
    torch.cuda.synchronize()
    np.testing.assert_allclose(adv.cpu().numpy(), adv0.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(mom.cpu().numpy(), mom0.cpu().numpy(), rtol=1e-4)


@pytest.mark.parametrize("n_envs", [1, 4])
def test_a2c_loop_smoke(n_envs, monkeypatch, tmp_path):
    make = lambda **kw: spprl.A2C("HalfCheetah-v2", batch_size=200, iterations=2, seed=0, n_envs=n_envs,  # noqa: E731
                                  env_spec=(17, 6, 1.0, 100), device=DEV, **kw)
    ag = make()
    assert isinstance(ag.env, spprl.SynthVecEnv) and ag.obs_norm_alpha == 0.99 and ag.gamma == 0.95
    ag.train()
    _loop_checks(ag, make, tmp_path, 400, {"actor", "critic"})
    assert not torch.equal(ag.obs_std, torch.ones(17, device=DEV))
    with pytest.raises(AttributeError):
        ag.pre_train()
    mem = ag.collect_batch()
    N = mem["T"] * n_envs
    obs, nobs = ag.normalize(mem["obs"].reshape(N, 17)), ag.normalize(mem["next_obs"].reshape(N, 17))
    _fused_and_unfused_agree(ag, obs, nobs, mem["rew"].reshape(N), mem["done"].reshape(N).float(), monkeypatch)


def test_a2c_acm_loop_smoke(monkeypatch, tmp_path):
    make = lambda **kw: spprl.A2C_AcM("HalfCheetah-v2", batch_size=200, iterations=2, seed=0, n_envs=4,  # noqa: E731
                                      custom_loss=0.5, norm_closs=False, acm_pre_train_samples=300,
                                      acm_pre_train_epochs=1, acm_update_freq=1, acm_epochs=1,
                                      env_spec=(17, 6, 1.0, 100), device=DEV, **kw)
    ag = make()
    ag.pre_train()
    before = ag.stats_logger.frames
    ag.train()
    _loop_checks(ag, make, tmp_path, before + 400, {"actor", "critic", "dist", "policy", "acm"})
    assert float(ag._actor_grad_sum.abs().sum()) > 0
    mem = ag.collect_batch()
    N = mem["T"] * 4
    _fused_and_unfused_agree(ag, mem["obs"].reshape(N, 17), ag.normalize(mem["next_obs"].reshape(N, 17)),
                             mem["rew"].reshape(N), mem["done"].reshape(N).float(), monkeypatch)
    plain = spprl.A2C_AcM("HalfCheetah-v2", batch_size=64, iterations=1, seed=0, n_envs=4, acm_pre_train_samples=300,
                          acm_pre_train_epochs=1, env_spec=(17, 6, 1.0, 100), device=DEV)
    plain.pre_train()
    plain.train()
    assert plain.custom_loss == 0.0 and plain._actor_grad_sum is None
    assert set(plain.loss) == {"actor", "critic", "acm"} and np.isfinite(plain.loss["actor"])
