"""Vanilla DDPG without a GPU: the fp32 torch restatement (tests/ddpg_ref.py) against the reference-generated
fixture tests/golden/ddpg_vanilla_hcheetah.npz (HalfCheetah dims, 2 updates of B = 100), at the tolerances of
tests/test_gpu_sac.py -- losses rel 1e-4 / abs 1e-6, post-Adam parameters within 2 * steps * lr * 1.01 with at
most 2e-3 of them beyond 1e-5 (the first-step sign-flip allowance) -- and the constructor checks of spprl.DDPG
that raise before the library is touched."""
import numpy as np
import pytest

import spprl
from ddpg_ref import NETS, DdpgRef, ddpg_vanilla_case, noise_action


def test_fixture_hyperparameters():
    fx = ddpg_vanilla_case()[0]
    assert tuple(int(v) for v in fx["dims"]) == (17, 6, 100)
    assert float(fx["tau"]) == 0.005 and float(fx["act_noise"]) == 0.1 and float(fx["gamma"]) == 0.99
    assert int(fx["max_ep_len"]) == 1000  # Q3: RL masks the time-limit done
    np.testing.assert_array_equal(fx["ac_lim"], np.ones(6, np.float32))


def test_restatement_matches_reference_fixture():
    fx, params, batches, _, _ = ddpg_vanilla_case()
    ob, ac, _ = (int(v) for v in fx["dims"])
    o = DdpgRef(ob, ac, ac_lim=fx["ac_lim"], gamma=0.99, tau=0.005, actor_lr=1e-3, critic_lr=1e-3, params=params)
    for i, batch in enumerate(batches):
        ol = o.update(*batch)
        assert set(ol) == {"actor", "critic"}
        for j, k in enumerate(("critic", "actor")):
            assert ol[k] == pytest.approx(float(fx["losses"][i][j]), rel=1e-4, abs=1e-6), (i, k)
    for k in NETS:
        d = np.abs(o.flat(k) - fx["post_" + k])
        print(k, "max |d| %.3g, share beyond 1e-5 %.3g" % (d.max(), np.mean(d > 1e-5)))
        assert d.max() <= 2 * len(batches) * 1e-3 * 1.01, (k, d.max())
        assert np.mean(d > 1e-5) < 2e-3, (k, np.mean(d > 1e-5))


def test_noise_action_matches_reference_fixture():
    fx, params, _, act_obs, act_draw = ddpg_vanilla_case()
    got = noise_action(params["actor"], act_obs, fx["ac_lim"], act_draw, 0.1)
    np.testing.assert_allclose(got, fx["noise_action"], rtol=1e-5, atol=1e-6)
    det = noise_action(params["actor"], act_obs, fx["ac_lim"], None, 0.0)
    np.testing.assert_allclose(det, fx["det_action"], rtol=1e-5, atol=1e-6)
    assert np.abs(got).max() <= 1.0
    assert np.abs(fx["noise_action"] - fx["det_action"]).max() > 0.01  # the injected draw reached the action


@pytest.mark.parametrize("kw", [dict(acm_epochs=3), dict(custom_loss=0.1), dict(foo=1), dict(acm_critic=True),
                                dict(denormalize_actor_out=True), dict(unbiased_update=True)])
def test_constructor_refuses_acm_and_unknown_keywords(kw):
    with pytest.raises(TypeError):
        spprl.DDPG(**kw)


def test_exported():
    assert "DDPG" in spprl.__all__ and spprl.DDPG.VANILLA is True
    assert spprl._lib.SPP_ALGO_DDPG == 4


def test_header_declares_the_algorithm_id():
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spprl.h")).read()
    m = re.search(r"SPP_ALGO_DDPG\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == spprl._lib.SPP_ALGO_DDPG


def test_update_macs_are_a_subset_of_sac():
    from spprl import flops

    d = flops.ddpg_macs(17, 6, aout=6, acm_critic=False, with_acm=False)
    s = flops.sac_macs(17, 6, aout=6, acm_critic=False, with_acm=False)
    assert d["M"] == 0 and d["acm_reg"] == 0
    assert d["update"] == d["critic_phase"] + d["actor_phase"] + d["dw"] < s["update"]
    # defaults unchanged: the DDPG_AcM count of bench.py's roofline
    assert flops.ddpg_macs(17, 6)["M"] == 2 * 17 * 100 + 100 * 50 + 2 * 17 * 50 + 50 * 6
