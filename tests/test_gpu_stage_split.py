"""GPU parity of the stage split of the SAC phase kernels (csrc/sac.hip): the per-sample stages (squash, ACM
forward; the chosen critics' gradients read back, frozen-ACM backward, heads backward) as kernels of their own
with a small LDS layout, several workgroups per CU, between the MFMA kernels they were cut out of:
  cut 1 (bit 0)  k_sac_actor_heads<C, true> -> k_sac_heads_stage, k_sac_actor_trunk_bwd
  cut 2 (bit 1)  k_sac_actor_phase<C, true> -> k_sac_trunk_fwd<C, true>, k_sac_squash_stage<C, true>, the critics
  cut 3 (bit 2)  k_sac_critic_phase         -> k_sac_trunk_fwd<C, false>, k_sac_squash_stage<C, false>, the rest

The new kernels call the device functions of the kernels they come from on the same values in the same order, so
the check is bit for bit: against an agent made under SPP_STAGE_SPLIT=0 (same seed, same inputs), after one full
update, both critics' gradients, the actor gradient, every loss, alpha and every parameter are identical.  The
cases are the smallest that can break a hand-over: one live sample, ragged tiles (B = 1, 31, 33, 100), one tile
more than the phase grid's waves (gi.second_tile_batch()) and one tile more than the stage kernels' waves (their
grids hold STAGE_WG_PER_CU workgroups per CU), every narrow-head fp32 kernel set (Hopper with and without the ACM
in front of the critics, HalfCheetah: two pairing blocks, the 3-dim set, vanilla SAC through the one-wave
kernels), the forced and tied critic selections of test_gpu_minq_split, and three updates of shrinking and
growing batches on one agent (stale hand-over rows).  Two cases run against the float64 oracle with
tests/test_gpu_bigbatch.py's tolerances.  Every case asserts through sppAgentStageSplit that the split agent
runs the new kernels and the reference agent does not.

CUTS lists the bit sets under test: each cut alone and all together.
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
import test_gpu_minq_split as mq  # noqa: E402
from spprl import _lib  # noqa: E402

DEV = bb.DEV
CUTS = [1, 2, 4, 7]
STAGE_WG_PER_CU = 3  # csrc/api.hip kStageWGPerCU

# name: (class, env, ob, aout, ac, constructor keywords)
ACM_KW = dict(custom_loss=0.2, norm_closs=False, min_max_denormalize=True, denormalize_actor_out=True, gamma=0.99)
SETS = {
    "hopper": (spprl.SAC_AcM, "Hopper-v2", 11, 11, 3, dict(ACM_KW, acm_critic=True)),
    "hopper_acmc0": (spprl.SAC_AcM, "Hopper-v2", 11, 11, 3, dict(ACM_KW, acm_critic=False)),
    "hcheetah": (spprl.SAC_AcM, "HalfCheetah-v2", 17, 17, 6, dict(ACM_KW, acm_critic=True)),
    "dim3": (spprl.SAC_AcM, "Pendulum-v0", 3, 3, 1, dict(ACM_KW, acm_critic=True)),
    "vanilla": (spprl.SAC, "HalfCheetah-v2", 17, 6, 6, dict(gamma=0.99, alpha=0.2)),
}


def stage_second_tile_batch():
    """One tile more than the stage kernel's waves (STAGE_WG_PER_CU workgroups of 4 waves per CU)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 32 * (4 * STAGE_WG_PER_CU * cus + 1)


def _batch_size(B):
    return {"second_tile": gi.second_tile_batch, "stage_second_tile": stage_second_tile_batch}[B]() if isinstance(
        B, str) else B


def _make(name, max_batch, bits, monkeypatch):
    cls, env, ob, aout, ac, kw = SETS[name]
    monkeypatch.setenv("SPP_SAC_TEAM", "0")  # read when the agent is made: the one-wave kernels at every batch
    monkeypatch.setenv("SPP_STAGE_SPLIT", str(bits))
    ag = cls(env_name=env, max_batch=max_batch, buffer_size=128, device=DEV, seed=3, **kw)
    got = ctypes.c_int(-1)
    _lib.call("sppAgentStageSplit", ag._h, ctypes.byref(got))
    assert got.value == bits, "the agent runs cuts %d, asked for %d" % (got.value, bits)
    return ag


def _inputs(name, B):
    _, _, ob, aout, ac, _ = SETS[name]
    rng = np.random.RandomState(B % 1000 + ob + aout)
    lo = -rng.uniform(0.5, 2, ob).astype(np.float32)
    hi = rng.uniform(0.5, 2, ob).astype(np.float32)
    batch = bb.random_batch(rng, B, ob, aout, ac)
    return lo, hi, batch, rng.randn(B, aout).astype(np.float32), rng.randn(B, aout).astype(np.float32)


def _step(name, ag, inp):
    lo, hi, batch, e1, e2 = inp
    if name == "vanilla":
        ag.update(*batch[:5], eps_next=e1, eps_cur=e2)
    else:
        rb = ag.replay_buffer
        rb.min_obs.copy_(torch.from_numpy(lo))
        rb.max_obs.copy_(torch.from_numpy(hi))
        rb._have_minmax = True
        ag.update(*batch, eps_next=e1, eps_cur=e2)
    torch.cuda.synchronize()


def _nets(name):
    return gi.VANILLA_NETS if name == "vanilla" else bb.SAC_NETS


def _state(name, ag):
    nets = _nets(name)
    out = {"losses": ag._losses.detach().cpu().numpy().copy(), "alpha": ag.alpha_state.cpu().numpy().copy(),
           "alpha_f32": ag.alpha_f32.cpu().numpy().copy()}
    for k in ("critic_1", "critic_2", "actor"):
        out["grad " + k] = ag.grads[nets[k]].cpu().numpy().copy()
    for k, n in nets.items():
        out["param " + k] = ag.params[n].cpu().numpy().copy()
    return out


def _run(name, sizes, mode, bits, monkeypatch):
    """One agent, one update per entry of sizes (max_batch = the largest); the state after each update."""
    ag = _make(name, max(sizes), bits, monkeypatch)
    if mode != "random":
        mq._shape(ag, mode)
    states = []
    for B in sizes:
        _step(name, ag, _inputs(name, B))
        states.append(_state(name, ag))
    return states


_REF = {}


def _reference(name, sizes, mode, monkeypatch):
    """The SPP_STAGE_SPLIT=0 agent's states, computed once per (set, sizes, mode) and shared by the cuts."""
    key = (name, tuple(sizes), mode)
    if key not in _REF:
        _REF[key] = _run(name, sizes, mode, 0, monkeypatch)
    return _REF[key]


def _assert_bitwise(name, sizes, mode, bits, monkeypatch):
    ref = _reference(name, sizes, mode, monkeypatch)
    got = _run(name, sizes, mode, bits, monkeypatch)
    for i, (r, g) in enumerate(zip(ref, got)):
        ga = r["grad actor"]
        assert np.isfinite(ga).all() and np.abs(ga).max() > 0
        for k in r:
            assert np.array_equal(r[k], g[k]), "update %d (B = %d) %s: %d elements differ" % (
                i, sizes[i], k, int(np.sum(r[k] != g[k])))


# ------------------------------------------------------------------ bit for bit against today's kernels
@pytest.mark.parametrize("bits", CUTS)
@pytest.mark.parametrize("B", [1, 31, 33, 100, "second_tile"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_stage_split_equals_phase_kernels_bitwise(name, B, bits, monkeypatch):
    _assert_bitwise(name, [_batch_size(B)], "random", bits, monkeypatch)


@pytest.mark.parametrize("bits", CUTS)
@pytest.mark.parametrize("name", ["hopper", "hcheetah"])  # one and two pairing blocks
def test_second_tile_per_stage_wave_bitwise(name, bits, monkeypatch):
    _assert_bitwise(name, [stage_second_tile_batch()], "random", bits, monkeypatch)


@pytest.mark.parametrize("bits", CUTS)
@pytest.mark.parametrize("B,mode", [(100, "force1"), (100, "force2"), (33, "tie")])
def test_chosen_selections_bitwise(B, mode, bits, monkeypatch):
    _assert_bitwise("hopper", [B], mode, bits, monkeypatch)


@pytest.mark.parametrize("bits", CUTS)
@pytest.mark.parametrize("name", ["hopper", "hcheetah"])
def test_smaller_batch_after_larger_reads_nothing_stale(name, bits, monkeypatch):
    _assert_bitwise(name, [100, 33, 100], "random", bits, monkeypatch)


# ------------------------------------------------------------------ against the float64 oracle
@pytest.mark.parametrize("env_name,ob,ac", [("Hopper-v2", 11, 3), ("HalfCheetah-v2", 17, 6)])
def test_matches_oracle(env_name, ob, ac, monkeypatch):
    monkeypatch.setenv("SPP_STAGE_SPLIT", str(max(CUTS)))
    created = []
    make = spprl.SAC_AcM

    def spy(*a, **kw):
        created.append(make(*a, **kw))
        return created[-1]

    monkeypatch.setattr(spprl, "SAC_AcM", spy)
    bb._sac_update_vs_oracle(env_name, ob, ac, 33, False, params_check=False)
    got = ctypes.c_int(-1)
    _lib.call("sppAgentStageSplit", created[0]._h, ctypes.byref(got))
    assert got.value == max(CUTS)
