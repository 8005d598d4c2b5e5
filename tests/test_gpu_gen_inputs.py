"""GPU parity of the register hand-over of the 256-wide layers' input blocks (csrc/mlp.h dense_gen).

The fp32 narrow-input kernel sets produce fc2's input (relu(fc1)) and W2^T's input (delta2 = dq * w3 * relu'(h2))
in registers inside the consumer's MFMA loop instead of staging them through the wave's LDS image.  The cases are
the smallest that can break that hand-over: one live sample, a ragged second tile, several tiles (B = 1, 33, 100),
every instantiation whose register plan changed (SAC_AcM HalfCheetah, the acm_critic=False set, both DDPG_AcM
shapes, vanilla SAC through the one-wave kernels), and per algorithm one batch of 4 * CUs + 1 tiles, so that one
wave runs a second tile and its masks, dq and fragment prefetch carry across the tile loop.

Every case compares one update against the float64 oracle with tests/test_gpu_bigbatch.py's fp32 tolerances:
losses rtol 1e-4, gradient norms 2e-4 per network and per layout tensor, elements bf16_cases.fp32_elem_tol.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import spprl  # noqa: E402
import bf16_cases as bc  # noqa: E402
import test_gpu_bigbatch as bb  # noqa: E402
from spprl import _lib  # noqa: E402
from oracle.ddpg_acm import OracleDdpgAcm  # noqa: E402
from oracle.sac import OracleSac  # noqa: E402

DEV = bb.DEV
F64 = torch.float64
VANILLA_NETS = {"actor": _lib.SPP_NET_ACTOR, "critic_1": _lib.SPP_NET_CRITIC1, "critic_2": _lib.SPP_NET_CRITIC2,
                "critic_1_targ": _lib.SPP_NET_CRITIC1_TARG, "critic_2_targ": _lib.SPP_NET_CRITIC2_TARG}


def second_tile_batch():
    """One tile more than the phase grid's waves (min(tiles / 4, CUs) workgroups of 4 waves): 32,800 on 256 CUs."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 32 * (4 * cus + 1)


# ------------------------------------------------------------------ SAC_AcM
@pytest.mark.parametrize("B", [1, 33, 100])
def test_sac_acm_hcheetah_matches_oracle(B):
    bb._sac_update_vs_oracle("HalfCheetah-v2", 17, 6, B, False, params_check=False)


def test_sac_acm_hopper_plain_critic_matches_oracle():
    bb._sac_update_vs_oracle("Hopper-v2", 11, 3, 33, "acmc0", params_check=False)


def test_sac_acm_second_tile_per_wave_matches_oracle():
    bb._sac_update_vs_oracle("HalfCheetah-v2", 17, 6, second_tile_batch(), False, params_check=True)


# ------------------------------------------------------------------ DDPG_AcM
def _ddpg_update_vs_oracle(env_name, ob, ac, B):
    rng = np.random.RandomState(B % 977 + ob)
    ag = spprl.DDPG_AcM(env_name=env_name, gamma=0.95, actor_lr=5e-4, critic_lr=5e-4, acm_critic=True,
                        custom_loss=1.0, norm_closs=False, min_max_denormalize=True, denormalize_actor_out=True,
                        max_batch=B, buffer_size=64, device=DEV, seed=4)
    params = bb.snapshot(ag, bb.DDPG_NETS)
    norm = bb.set_minmax(ag, rng, ob)
    batch = bb.random_batch(rng, B, ob, ob, ac)
    ag.update(*batch)
    torch.cuda.synchronize()
    o = OracleDdpgAcm(ob, ob, ac, norm=norm, actor_lim=1.0, gamma=0.95, tau=0.005, params=params, dtype=F64)
    ol = o.update(*batch)
    gl = ag.loss
    for k in ("critic", "actor"):
        g = ag.grads[bb.DDPG_NETS[k]].cpu().numpy()
        e = bb.relerr(g, o.last["grads"][k])
        print(env_name, B, k, "grad rel err %.2e" % e)
        assert e < 2e-4, (k, e)
        bc.assert_tensor_grads(g, o.last["grads"][k], o.layouts[k], 2e-4, k, bc.fp32_elem_tol(B))
    for k in ("critic", "actor", "ddpg", "dist"):
        assert abs(gl[k] - ol[k]) <= 1e-4 * abs(ol[k]) + 1e-6, (k, gl[k], ol[k])


@pytest.mark.parametrize("env_name,ob,ac", [("Hopper-v2", 11, 3), ("HalfCheetah-v2", 17, 6)])
@pytest.mark.parametrize("B", [33, 100])
def test_ddpg_acm_matches_oracle(env_name, ob, ac, B):
    _ddpg_update_vs_oracle(env_name, ob, ac, B)


def test_ddpg_acm_second_tile_per_wave_matches_oracle():
    _ddpg_update_vs_oracle("HalfCheetah-v2", 17, 6, second_tile_batch())


# ------------------------------------------------------------------ vanilla SAC, one-wave kernels
def _vanilla_update_vs_oracle(B, monkeypatch):
    monkeypatch.setenv("SPP_SAC_TEAM", "0")  # read when the agent is made: the one-wave phase kernels at every batch
    ob, ac = 17, 6
    ag = spprl.SAC(env_name="HalfCheetah-v2", gamma=0.99, actor_lr=1e-3, critic_lr=1e-3, alpha_lr=1e-3, alpha=0.2,
                   max_batch=B, buffer_size=64, device=DEV, seed=5)
    params = bb.snapshot(ag, VANILLA_NETS)
    rng = np.random.RandomState(B % 991)
    batch = (rng.randn(B, ob).astype(np.float32), rng.randn(B, ob).astype(np.float32),
             rng.uniform(-1, 1, (B, ac)).astype(np.float32), rng.randn(B).astype(np.float32),
             (rng.rand(B) < 0.1).astype(np.int8))
    e1, e2 = rng.randn(B, ac).astype(np.float32), rng.randn(B, ac).astype(np.float32)
    ag.update(*batch, eps_next=e1, eps_cur=e2)
    torch.cuda.synchronize()
    o = OracleSac(ob, ac, params=params, dtype=F64)
    ol = o.update(*batch, e1, e2)
    for k in ("critic_1", "critic_2", "actor"):
        g = ag.grads[VANILLA_NETS[k]].cpu().numpy()
        e = bb.relerr(g, o.last["grads"][k])
        print("vanilla", B, k, "grad rel err %.2e" % e)
        assert e < 2e-4, (k, e)
        bc.assert_tensor_grads(g, o.last["grads"][k], o.layouts[k], 2e-4, k, bc.fp32_elem_tol(B))
        assert abs(ag.loss[k] - ol[k]) <= 1e-4 * abs(ol[k]) + 1e-6, (k, ag.loss[k], ol[k])


def test_vanilla_sac_one_wave_kernels_match_oracle(monkeypatch):
    _vanilla_update_vs_oracle(100, monkeypatch)


def test_vanilla_sac_second_tile_per_wave_matches_oracle(monkeypatch):
    _vanilla_update_vs_oracle(second_tile_batch(), monkeypatch)
