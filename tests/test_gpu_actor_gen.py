"""GPU parity of the register hand-over forms of the actor trunk kernels (csrc/sac.hip), chosen per handle by
SPP_ACTOR_GEN when the agent is made:
  bit 0  k_sac_trunk_fwd<C, ACT>  -> k_sac_trunk_fwd_gen<C, ACT>   fc1's blocks made under fc2's MFMAs (Fc1Gen)
  bit 1  k_sac_actor_trunk_bwd    -> k_sac_actor_trunk_bwd_gen     Wh^T's blocks made under W2^T's MFMAs (WhTGen)

The generators run the staged layers' MFMA chains (bias tile or zero, then the register quads in flat order) and
dense_gen has dense_lds's fragment ring, chunk order and epilogue placement, so the check is bit for bit: an agent
made under SPP_ACTOR_GEN = 1, 2 and 3 against one made under 0 (same seed, same inputs), after one full update:
both critics' gradients, the actor gradient, every loss, alpha and every parameter are identical.  Every case
asserts through sppAgentActorGen that the agent runs the kernels asked for and the reference agent the staged ones,
so a quiet fall-back to the staged kernels cannot pass.

Batches: B = 1, 33 and 100 (ragged tiles, one workgroup, up to 4 tiles) and one tile more than the grid's waves,
32 (4 CUs + 1), where one wave runs a second tile: the generator's fragment prefetch (its last block re-requests its
own fragments) and the mask words carry across the tile loop.  Kernel sets: tests/test_gpu_stage_split.py's SAC_AcM
sets, Hopper with and without the ACM in front of the critics, HalfCheetah (two pairing blocks: NBI = 2 in WhTGen)
and the 3-dim set.  Three updates of shrinking and growing batches run on one agent.  One case runs against the
float64 oracle with tests/test_gpu_bigbatch.py's fp32 tolerances.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import spprl  # noqa: E402
import test_gpu_bigbatch as bb  # noqa: E402
import test_gpu_gen_inputs as gi  # noqa: E402
import test_gpu_stage_split as ss  # noqa: E402
from spprl import _lib  # noqa: E402

GEN = [1, 2, 3]
SETS = ["dim3", "hcheetah", "hopper", "hopper_acmc0"]  # keys of ss.SETS: the SAC_AcM sets with the stage-split cuts


def _gen_of(ag):
    got = ctypes.c_int(-1)
    _lib.call("sppAgentActorGen", ag._h, ctypes.byref(got))
    return got.value


def _env(monkeypatch, bits):
    monkeypatch.setenv("SPP_SAC_TEAM", "0")  # read when the agent is made: the one-wave kernels at every batch
    monkeypatch.delenv("SPP_STAGE_SPLIT", raising=False)  # every cut (the default)
    monkeypatch.delenv("SPP_CRITIC_PAIRS", raising=False)
    monkeypatch.setenv("SPP_ACTOR_GEN", str(bits))


def _make(name, max_batch, bits, monkeypatch):
    cls, env, ob, aout, ac, kw = ss.SETS[name]
    _env(monkeypatch, bits)
    ag = cls(env_name=env, max_batch=max_batch, buffer_size=128, device=bb.DEV, seed=3, **kw)
    cuts = ctypes.c_int(-1)
    _lib.call("sppAgentStageSplit", ag._h, ctypes.byref(cuts))
    assert cuts.value == 7, "the agent runs cuts %d: the hand-over kernels sit behind the cuts" % cuts.value
    assert _gen_of(ag) == bits, "the agent runs hand-over forms %d, asked for %d" % (_gen_of(ag), bits)
    return ag


def _run(name, sizes, bits, monkeypatch):
    """One agent, one update per entry of sizes (max_batch = the largest); the state after each update."""
    ag = _make(name, max(sizes), bits, monkeypatch)
    states = []
    for B in sizes:
        ss._step(name, ag, ss._inputs(name, B))
        states.append(ss._state(name, ag))
    return states


_REF = {}


def _reference(name, sizes, monkeypatch):
    """The SPP_ACTOR_GEN=0 agent's states, computed once per (set, sizes) and shared by the bit sets."""
    key = (name, tuple(sizes))
    if key not in _REF:
        _REF[key] = _run(name, sizes, 0, monkeypatch)
    return _REF[key]


def _assert_bitwise(name, sizes, bits, monkeypatch):
    ref = _reference(name, sizes, monkeypatch)
    got = _run(name, sizes, bits, monkeypatch)
    for i, (r, g) in enumerate(zip(ref, got)):
        for k in ("grad critic_1", "grad critic_2", "grad actor"):
            assert np.isfinite(r[k]).all() and np.abs(r[k]).max() > 0, k
        for k in r:
            assert np.array_equal(r[k], g[k]), "update %d (B = %d) %s: %d elements differ" % (
                i, sizes[i], k, int(np.sum(r[k] != g[k])))


# ------------------------------------------------------------------ bit for bit against the staged kernels
@pytest.mark.parametrize("bits", GEN)
@pytest.mark.parametrize("B", [1, 33, 100, "second_tile"])
@pytest.mark.parametrize("name", SETS)
def test_hand_over_equals_staged_kernels_bitwise(name, B, bits, monkeypatch):
    _assert_bitwise(name, [gi.second_tile_batch() if B == "second_tile" else B], bits, monkeypatch)


@pytest.mark.parametrize("bits", GEN)
@pytest.mark.parametrize("name", ["hopper", "hcheetah"])  # one and two pairing blocks
def test_shrinking_and_growing_batches_bitwise(name, bits, monkeypatch):
    _assert_bitwise(name, [100, 33, 100], bits, monkeypatch)


# ------------------------------------------------------------------ against the float64 oracle
def test_matches_oracle(monkeypatch):
    """B = 100: 4 tiles on the 4 waves of one workgroup, both hand-overs."""
    _env(monkeypatch, max(GEN))
    created = []
    make = spprl.SAC_AcM

    def spy(*a, **kw):
        created.append(make(*a, **kw))
        return created[-1]

    monkeypatch.setattr(spprl, "SAC_AcM", spy)
    bb._sac_update_vs_oracle("Hopper-v2", 11, 3, 100, False, params_check=False)
    assert _gen_of(created[0]) == max(GEN)


# ------------------------------------------------------------------ handles without the kernels report none
@pytest.mark.parametrize("which", ["sac_ant", "sac_bf16", "ddpg_acm", "vanilla_sac"])
def test_handles_without_the_kernels_report_zero(which, monkeypatch):
    _env(monkeypatch, max(GEN))
    acm = dict(ss.ACM_KW, acm_critic=True)
    if which == "sac_ant":  # 111-dim observations: four observation blocks, wide heads
        ag = spprl.SAC_AcM(env_name="Ant-v2", max_batch=64, buffer_size=128, device=bb.DEV, seed=3, **acm)
    elif which == "sac_bf16":
        ag = spprl.SAC_AcM(env_name="Hopper-v2", max_batch=64, buffer_size=128, device=bb.DEV, seed=3, mlp_bf16=True,
                           **acm)
    elif which == "ddpg_acm":
        ag = spprl.DDPG_AcM(env_name="HalfCheetah-v2", gamma=0.95, acm_critic=True, custom_loss=1.0, norm_closs=False,
                            min_max_denormalize=True, denormalize_actor_out=True, max_batch=64, buffer_size=128,
                            device=bb.DEV, seed=3)
    else:
        ag = spprl.SAC(env_name="HalfCheetah-v2", gamma=0.99, alpha=0.2, max_batch=64, buffer_size=128, device=bb.DEV,
                       seed=3)
    assert _gen_of(ag) == 0
