"""A2C and A2C_AcM without a GPU: the restatement (tests/a2c_ref.py) in float32 against the reference-generated
fixtures tests/golden/a2c_vanilla_hcheetah.npz and a2c_acm_hcheetah.npz (make_golden_a2c.py), the two reference
quirks the fixtures pin (the actor steps on rollout-normalised observations; update_actor_acm's gradient is never
zeroed), the constructor checks that raise before the library is touched, and the boundary's new symbols.

Bounds, as tests/test_ppo_ref_golden.py holds the same quantities: statistics rtol 1e-6, losses rtol 1e-5, advantages
rtol 1e-4 / atol 1e-4, parameters rtol 1e-4 / atol 5e-6."""
import inspect
import os
import re

import numpy as np
import pytest

import a2c_ref
import spprl

P_TOL = dict(rtol=1e-4, atol=5e-6)


def _hp(fx):
    return dict(gamma=float(fx["gamma"]), actor_lr=float(fx["actor_lr"]), critic_lr=float(fx["critic_lr"]),
                targets=int(fx["critic_num_target_updates"]), steps=int(fx["num_critic_updates_per_target"]))


@pytest.fixture(scope="module")
def vanilla():
    fx, actor, critic, mem = a2c_ref.a2c_vanilla_case()
    ob, ac = (int(v) for v in fx["dims"])
    mean0, std0 = a2c_ref.vanilla_start_stats(int(fx["seed"]), ob)
    run = lambda **kw: a2c_ref.a2c_update(actor, critic, mem, ob, ac, fx["ac_lim"],  # noqa: E731
                                          alpha=float(fx["obs_norm_alpha"]), mean=mean0, std=std0, **_hp(fx), **kw)
    return fx, mem, run(), run


@pytest.fixture(scope="module")
def acm():
    fx, actor, critic, mems, lo, hi = a2c_ref.a2c_acm_case()
    ob, lim = int(fx["dims"][0]), fx["actor_ac_lim"]
    run = lambda **kw: a2c_ref.acm_updates(actor, critic, mems, ob, lim, lo, hi,  # noqa: E731
                                           custom_loss=float(fx["custom_loss"]), **_hp(fx), **kw)
    return fx, mems, run(), run


def test_vanilla_fixture_shape(vanilla):
    fx, mem, _, _ = vanilla
    assert tuple(int(v) for v in fx["dims"]) == (17, 6) and float(fx["obs_norm_alpha"]) == 0.95
    assert mem["obs"].shape == (96, 17) and mem["start_obs"].shape == (3, 17) and fx["adv"].shape == (96,)
    assert int(fx["critic_num_target_updates"]) == 2 and int(fx["num_critic_updates_per_target"]) == 3


def test_vanilla_statistics_critic_and_advantages(vanilla):
    fx, _, res, _ = vanilla
    for k in ("obs_mean", "obs_std", "max_obs", "min_obs"):
        np.testing.assert_allclose(res[k], fx[k], rtol=1e-6, err_msg=k)
    assert res["critic_loss"] == pytest.approx(float(fx["crit_loss"]), rel=1e-5)
    np.testing.assert_allclose(res["critic"], fx["crit_post"], **P_TOL)
    np.testing.assert_allclose(res["adv"], fx["adv"], rtol=1e-4, atol=1e-4)


def test_vanilla_actor_step(vanilla):
    fx, _, res, _ = vanilla
    assert res["actor_loss"] == pytest.approx(float(fx["actor_loss"]), rel=1e-5)
    np.testing.assert_allclose(res["actor"], fx["actor_post"], **P_TOL)


def test_vanilla_fixture_sees_the_statistics_order(vanilla):
    """The actor on observations normalised with the UPDATED statistics misses the fixture's actor loss by far more
    than 10x the GPU test's tolerance (rtol 1e-4): test_gpu_a2c relies on this separation."""
    fx, _, res, run = vanilla
    wrong = run(actor_new_stats=True)
    want = float(fx["actor_loss"])
    sep = abs(wrong["actor_loss"] - want) / abs(want)
    print("actor loss: fixture %.6g, new-statistics order %.6g (relative distance %.3g)"
          % (want, wrong["actor_loss"], sep))
    assert sep > 10 * 1e-4
    assert not np.allclose(wrong["actor"], fx["actor_post"], **P_TOL)
    np.testing.assert_array_equal(wrong["adv"], res["adv"])  # (only the actor's inputs differ)


def test_acm_fixture_matches(acm):
    fx, mems, res, _ = acm
    assert len(mems) == 2 and all(m["obs"].shape == (96, 17) and m["act"].shape == (96, 17) for m in mems)
    for k, r in enumerate(res, 1):
        assert r["critic_loss"] == pytest.approx(float(fx["crit_loss%d" % k]), rel=1e-5)
        np.testing.assert_allclose(r["critic_post"], fx["crit_post%d" % k], **P_TOL)
        np.testing.assert_allclose(r["adv"], fx["adv%d" % k], rtol=1e-4, atol=1e-4)
        for j, n in enumerate(("actor", "dist", "policy")):
            assert r[n] == pytest.approx(float(fx["losses%d" % k][j]), rel=1e-5), (k, n)
        np.testing.assert_allclose(r["actor_post"], fx["actor_post%d" % k], **P_TOL, err_msg="step %d" % k)


def test_acm_fixture_sees_the_accumulated_gradient(acm):
    """Zeroing the gradient between the two update_actor_acm calls (what the reference does not do) reproduces the
    first step and misses the second."""
    fx, _, _, run = acm
    z = run(zero_grad=True)
    np.testing.assert_allclose(z[0]["actor_post"], fx["actor_post1"], **P_TOL)
    assert not np.allclose(z[1]["actor_post"], fx["actor_post2"], **P_TOL)
    d = np.abs(z[1]["actor_post"] - fx["actor_post2"])
    print("zeroed gradient: second step off by up to %.3g (lr %.3g)" % (d.max(), float(fx["actor_lr"])))
    assert d.max() > 0.1 * float(fx["actor_lr"])


def test_norm_closs_restatement(acm):
    """norm_closs (not in the fixture: the reference raises there, make_golden_a2c.py): the same gradient and actor
    loss, the distance on the stored actions against the normalised next observations."""
    fx, mems, res, run = acm
    n = run(norm_closs=True)
    _, _, _, _, lo, hi = a2c_ref.a2c_acm_case()
    for r, q, mem in zip(res, n, mems):
        np.testing.assert_array_equal(r["actor_post"], q["actor_post"])
        assert r["actor"] == q["actor"] and r["dist"] != q["dist"]
        want = np.mean((mem["act"].astype(np.float64) - a2c_ref.minmax_normalize(mem["next_obs"], lo, hi)) ** 2)
        assert q["dist"] == pytest.approx(want, rel=1e-5)


def test_normalize_adv_uses_1e_8():
    a = np.array([1.0, 1.0 + 1e-7, 1.0 - 1e-7], np.float64)
    got = a2c_ref.normalize_adv(a, dtype=__import__("torch").float64)
    np.testing.assert_allclose(got, (a - a.mean()) / (a.std(ddof=1) + 1e-8), rtol=1e-12)
    assert abs(got[1]) < 0.95  # (+ 1e-8 shows against a std of 1e-7; + 1.2e-7 would halve it)


# ---------------------------------------------------------------- constructors (no library, no GPU)
def test_defaults_are_the_references():
    d = {k: v.default for k, v in inspect.signature(spprl.A2C.__init__).parameters.items()}
    want = dict(actor_lr=3e-3, critic_lr=3e-4, critic_num_target_updates=10, num_critic_updates_per_target=10,
                normalize_adv=True, obs_norm_alpha=0.99, gamma=0.95, batch_size=200)
    assert {k: d[k] for k in want} == want
    d = {k: v.default for k, v in inspect.signature(spprl.A2C_AcM.__init__).parameters.items()}
    want = dict(actor_lr=3e-3, critic_lr=3e-4, gamma=0.95, batch_size=200, custom_loss=0.0)
    assert {k: d[k] for k in want} == want


PPO_KW = [dict(epsilon=0.2), dict(gae_lambda=0.9), dict(kl_div_threshold=0.1), dict(max_ppo_epochs=3),
          dict(ppo_batch_size=64), dict(entropy_coef=0.01)]
ACM_KW = [dict(acm_epochs=3), dict(custom_loss=0.1), dict(norm_closs=True), dict(denormalize_actor_out=True),
          dict(min_max_denormalize=True)]


@pytest.mark.parametrize("kw", PPO_KW + ACM_KW + [dict(foo=1)], ids=lambda kw: next(iter(kw)))
def test_a2c_refuses_ppo_acm_and_unknown_keywords(kw, monkeypatch):
    from spprl import _lib

    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    with pytest.raises(TypeError, match=next(iter(kw))):
        spprl.A2C(**kw)


@pytest.mark.parametrize("kw", PPO_KW, ids=lambda kw: next(iter(kw)))
def test_a2c_acm_refuses_ppo_keywords(kw, monkeypatch):
    from spprl import _lib

    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    with pytest.raises(TypeError, match=next(iter(kw))):
        spprl.A2C_AcM(**kw)


def test_a2c_keywords_reach_the_library(monkeypatch):
    from spprl import _lib, onpolicy_loop, trainer

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()

    monkeypatch.setattr(_lib, "load", stop)
    monkeypatch.setattr(_lib, "call", stop)
    monkeypatch.setattr(trainer, "SynthVecEnv", stop)
    monkeypatch.setattr(onpolicy_loop, "SynthVecEnv", stop)
    with pytest.raises(Reached):
        spprl.A2C(device="cpu", env_name="Hopper-v2", iterations=10, gamma=0.99, actor_lr=3e-4, critic_lr=1e-3,
                  batch_size=2000, tensorboard_dir="logs", log_dir="logs/basic_logs", verbose=0, render=False,
                  obs_norm_alpha=0.95, test_episodes=10, n_envs=4)


def test_exported_and_boundary():
    assert "A2C" in spprl.__all__ and "A2C_AcM" in spprl.__all__
    assert issubclass(spprl.A2C, spprl.PPO) and issubclass(spprl.A2C_AcM, spprl.PPO_AcM)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spprl.h")).read()
    declared = set(re.findall(r"^\s*(?:sppStatus|const char\*|int|int64_t)\s+(spp\w+)\s*\(", hdr, re.M))
    assert declared == set(spprl._lib.EXPORTED)
    for name in ("sppOnpTdAdvantage", "sppOnpPgActorGrads"):
        assert name in declared
    assert spprl.ppo_vanilla.PPO.update is not spprl.A2C.update
