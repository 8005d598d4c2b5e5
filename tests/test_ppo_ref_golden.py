"""Vanilla PPO without a GPU: the restatement (tests/ppo_ref.py) against the reference-generated fixture
tests/golden/ppo_vanilla_hcheetah.npz (make_golden_ppo.py: three hand-filled rollouts, 96 frames, statistics,
2 x 3 critic steps, GAE, actor epochs with the KL stop), the constructor checks of spprl.PPO that raise before the
library is touched, and the boundary's new symbols.

Bounds: statistics rtol 1e-6; the other quantities as tests/test_ddpg_ref_golden.py holds vanilla DDPG's -- losses
and KL rel 1e-4 / abs 1e-6, forward outputs (the advantages: critic forwards and a scan) rtol 1e-5 / atol 1e-6 per
unit of the largest |advantage| reached through the 6 critic steps' parameter allowance, post-Adam parameters
within 2 * steps * lr * 1.01 with at most 2e-3 of them beyond 1e-5; epochs and the counter exact."""
import os
import re

import numpy as np
import pytest

import spprl
import ppo_ref
from oracle import onpolicy as oo


@pytest.fixture(scope="module")
def case():
    fx, actor, critic, mem = ppo_ref.ppo_vanilla_case()
    ob, ac = (int(v) for v in fx["dims"])
    res = ppo_ref.ppo_update(actor, critic, mem, ob, ac, fx["ac_lim"], alpha=float(fx["obs_norm_alpha"]),
                             gamma=float(fx["gamma"]), gae_lambda=float(fx["gae_lambda"]),
                             actor_lr=float(fx["actor_lr"]), critic_lr=float(fx["critic_lr"]),
                             targets=int(fx["critic_num_target_updates"]),
                             steps=int(fx["num_critic_updates_per_target"]), max_epochs=int(fx["max_epochs"]),
                             kl_threshold=float(fx["threshold"]), batch_size=int(fx["ppo_batch_size"]),
                             eps_clip=float(fx["eps"]), entropy_coef=float(fx["entropy_coef"]))
    return fx, mem, res


def test_fixture_shape_and_hyperparameters(case):
    fx, mem, _ = case
    assert tuple(int(v) for v in fx["dims"]) == (17, 6) and float(fx["obs_norm_alpha"]) == 0.95
    assert mem["obs"].shape == (96, 17) and mem["start_obs"].shape == (3, 17)
    ends = np.flatnonzero(mem["end"])
    assert list(ends) == [39, 64, 95] and list(mem["done"][ends]) == [1, 1, 0]  # the last: a time-limit end
    assert int(fx["max_ep_len"]) == 1000 and int(fx["max_epochs"]) == 4
    np.testing.assert_array_equal(fx["ac_lim"], np.ones(6, np.float32))


def test_statistics_match_reference_fixture(case):
    fx, _, res = case
    for k in ("obs_mean", "obs_std", "max_obs", "min_obs"):
        np.testing.assert_allclose(res[k], fx[k], rtol=1e-6, err_msg=k)
    assert (res["norm_obs"] == 10.0).any()  # a column beyond the clip


def test_critic_and_advantages_match_reference_fixture(case):
    fx, _, res = case
    lr, steps = float(fx["critic_lr"]), 6
    assert res["critic_loss"] == pytest.approx(float(fx["crit_loss"]), rel=1e-4, abs=1e-6)
    d = np.abs(res["critic"] - fx["crit_post"])
    print("critic max |d| %.3g, share beyond 1e-5 %.3g" % (d.max(), np.mean(d > 1e-5)))
    assert d.max() <= 2 * steps * lr * 1.01 and np.mean(d > 1e-5) < 2e-3
    e = np.abs(res["adv"] - fx["adv"])
    print("adv max |d| %.3g of max |adv| %.3g" % (e.max(), np.abs(fx["adv"]).max()))
    np.testing.assert_allclose(res["adv"], fx["adv"], rtol=1e-5, atol=1e-6 * max(1.0, np.abs(fx["adv"]).max()))


def test_actor_epochs_match_reference_fixture(case):
    fx, _, res = case
    lr = float(fx["actor_lr"])
    assert len(res["kls"]) == len(fx["kls"]) == 3  # the stop triggers before the 4th epoch
    assert res["counter"] == int(fx["counter"]) == 4
    for got, want in zip(res["kls"], fx["kls"]):
        assert got == pytest.approx(float(want), rel=1e-4, abs=1e-6)
    for j, k in enumerate(("actor", "entropy", "sum")):
        assert res["loss"][k] == pytest.approx(float(fx["losses"][j]), rel=1e-4, abs=1e-6), k
    d = np.abs(res["actor"] - fx["actor_post"])
    print("actor max |d| %.3g, share beyond 1e-5 %.3g" % (d.max(), np.mean(d > 1e-5)))
    assert d.max() <= 2 * 3 * lr * 1.01 and np.mean(d > 1e-5) < 2e-3


def test_obs_statistics_restatement_properties():
    rng = np.random.RandomState(0)
    start, nxt = rng.randn(2, 5), rng.randn(30, 5)
    nxt[:, 2] = start[:, 2] = 1.5  # a constant column: std 0
    obs = np.concatenate([start[:1], nxt[:-1]])
    m0, s0 = rng.randn(5), rng.uniform(0.5, 2, 5)
    m, s, mx, mn = ppo_ref.update_obs_mean_std(start, nxt, obs, 1.0, m0, s0)
    np.testing.assert_array_equal(m, m0)  # alpha = 1: no update (a2c.py:41-45)
    m, s, mx, mn = ppo_ref.update_obs_mean_std(start, nxt, obs, 0.0, m0, s0)
    np.testing.assert_allclose(m, np.concatenate([start, nxt]).mean(0), rtol=1e-12)
    assert s[2] == 0.0 and mx.dtype == np.float32 and (mx >= mn).all()
    z = ppo_ref.standardize_and_clip(np.array([[100.0, -100.0, 0.5]]), np.zeros(3), np.ones(3))
    np.testing.assert_allclose(z, [[10.0, -10.0, 0.5 / (1 + 1e-8)]])


# every keyword train/vanilla_ppo_hcheetah.py hands the algorithm (through EvalsWrapper, log_all: tensorboard_dir)
TRAIN_KW = dict(iterations=1001, gamma=0.99, actor_lr=3e-4, critic_lr=1e-3, batch_size=2000, tensorboard_dir="logs",
                return_done=1e4, log_dir="logs/basic_logs", verbose=0, render=False, ppo_batch_size=512,
                kl_div_threshold=0.1, env_name="HalfCheetah-v2", max_frames=1e6, entropy_coef=0.0,
                tensorboard_comment="", max_ppo_epochs=10, obs_norm_alpha=0.95, test_episodes=10)


def test_training_script_keywords_reach_the_library(monkeypatch):
    """Every keyword is accepted up to the point where the library would be loaded."""
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
        spprl.PPO(device="cpu", **TRAIN_KW)


@pytest.mark.parametrize("kw,name", [(dict(foo=1), "foo"), (dict(acm_epochs=3), "acm_epochs"),
                                     (dict(custom_loss=0.1), "custom_loss"), (dict(norm_closs=True), "norm_closs"),
                                     (dict(denormalize_actor_out=True), "denormalize_actor_out"),
                                     (dict(min_max_denormalize=True), "min_max_denormalize")])
def test_constructor_refuses_acm_and_unknown_keywords(kw, name, monkeypatch):
    from spprl import _lib

    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    with pytest.raises(TypeError, match=name):
        spprl.PPO(**kw)


def test_defaults_are_the_references():
    import inspect

    d = {k: v.default for k, v in inspect.signature(spprl.PPO.__init__).parameters.items()}
    want = dict(actor_lr=3e-3, critic_lr=3e-4, epsilon=0.2, gae_lambda=0.95, kl_div_threshold=0.15, max_ppo_epochs=50,
                ppo_batch_size=1000, entropy_coef=0.0, critic_num_target_updates=10, num_critic_updates_per_target=10,
                normalize_adv=True, obs_norm_alpha=0.99, gamma=0.95, batch_size=200)
    assert {k: d[k] for k in want} == want


def test_exported_and_boundary():
    assert "PPO" in spprl.__all__ and spprl.PPO is not spprl.PPO_AcM
    assert spprl.ppo.calculate_gae  # the spprl.ppo module keeps its name and contents
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spprl.h")).read()
    declared = set(re.findall(r"^\s*(?:sppStatus|const char\*|int|int64_t)\s+(spp\w+)\s*\(", hdr, re.M))
    assert declared == set(spprl._lib.EXPORTED)
    for name in ("sppOnpRolloutAct", "sppOnpObsStats"):
        assert name in declared
    assert oo.actor_layout(11, 3)[0] == ("log_scale", (3,))
