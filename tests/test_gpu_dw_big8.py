"""GPU parity of the two forms of the fp32 256 x 256 weight-gradient kernel (csrc/dw.hip): k_dw_big8 (8 waves per
workgroup, two per SIMD, a 4 x 2-block output tile per wave) against k_dw_big (4 waves, 4 x 4 blocks each).

Both run the same items; every 32 x 32 output block accumulates the same MFMA chain over the item's samples in the
same order, the bias sums are formed by the same expression and the slabs hold the same images, so the check is bit
for bit: an agent made under SPP_DW_BIG_WAVES=8 against one made under 4 (same seed, same inputs), after one full
update: every network's gradient buffer, every loss, alpha and every parameter are identical.  Every case asserts
through sppAgentDwBigWaves that the two agents run different forms.

The big kernel starts at Bp = 8,192 padded samples; the batches are the smallest that reach every path of its step
loop (items of n 32-sample steps, two LDS buffers, one barrier per step, the DMA for step t + 2 issued behind step
t's barrier).  With C = the device's CUs and one item per CU over a launch (the actor job alone, the two critics'
jobs together):
  B = 8,192            1 step per actor item (no loop barrier at all), 2 per critic item (at C = 256)
  B = 8,193            Bp = 8,224: ragged last items; the critics' items run 3 steps (C = 256): an odd count, both
                       buffer parities refilled or not, and a last item of another length
  B = 32 (4 C) + 32    5 and 9 steps per item: each buffer is refilled at least twice
  32,800 -> 8,192 -> 8,193 on one agent: shrinking and growing batches (job tables rebuilt, stale slabs)
on the kernel sets SAC_AcM Hopper, DDPG_AcM HalfCheetah and SAC_AcM Ant fp32 (whose fc1 jobs stay in k_dw beside the
big launch).  One Hopper case at B = 8,193 runs against the float64 oracle with tests/test_gpu_bigbatch.py's
tolerances.
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
from spprl import _lib  # noqa: E402

ACM_KW = dict(acm_critic=True, norm_closs=False, min_max_denormalize=True, denormalize_actor_out=True)
# name: (class, env, ob, ac, constructor keywords); the actor has ob outputs (the ACM maps them to ac actions)
SETS = {
    "sac_hopper": (spprl.SAC_AcM, "Hopper-v2", 11, 3, dict(ACM_KW, custom_loss=0.2, gamma=0.99)),
    "sac_ant": (spprl.SAC_AcM, "Ant-v2", 111, 8, dict(ACM_KW, custom_loss=0.2, gamma=0.99)),
    "ddpg_hcheetah": (spprl.DDPG_AcM, "HalfCheetah-v2", 17, 6,
                      dict(ACM_KW, custom_loss=1.0, gamma=0.95, actor_lr=5e-4, critic_lr=5e-4)),
}


def _batch_size(B):
    """"4C+1": one 32-sample step more than 4 per CU."""
    return 32 * (4 * torch.cuda.get_device_properties(0).multi_processor_count) + 32 if B == "4C+1" else B


def _waves_of(ag):
    got = ctypes.c_int(-1)
    _lib.call("sppAgentDwBigWaves", ag._h, ctypes.byref(got))
    return got.value


def _make(name, max_batch, waves, monkeypatch):
    cls, env, _, _, kw = SETS[name]
    monkeypatch.setenv("SPP_DW_BIG_WAVES", str(waves))  # read when the agent is made
    ag = cls(env_name=env, max_batch=max_batch, buffer_size=128, device=bb.DEV, seed=3, **kw)
    assert _waves_of(ag) == waves, "the agent runs the %d-wave form, asked for %d" % (_waves_of(ag), waves)
    return ag


def _inputs(name, B):
    _, _, ob, ac, _ = SETS[name]
    rng = np.random.RandomState(B % 1000 + ob)
    lo = -rng.uniform(0.5, 2, ob).astype(np.float32)
    hi = rng.uniform(0.5, 2, ob).astype(np.float32)
    batch = bb.random_batch(rng, B, ob, ob, ac)
    return lo, hi, batch, rng.randn(B, ob).astype(np.float32), rng.randn(B, ob).astype(np.float32)


def _step(name, ag, inp):
    lo, hi, batch, e1, e2 = inp
    rb = ag.replay_buffer
    rb.min_obs.copy_(torch.from_numpy(lo))
    rb.max_obs.copy_(torch.from_numpy(hi))
    rb._have_minmax = True
    if SETS[name][0] is spprl.SAC_AcM:
        ag.update(*batch, eps_next=e1, eps_cur=e2)
    else:
        ag.update(*batch)
    torch.cuda.synchronize()


def _state(ag):
    out = {"losses": ag._losses.detach().cpu().numpy().copy()}
    if hasattr(ag, "alpha_state"):
        out["alpha"] = ag.alpha_state.cpu().numpy().copy()
        out["alpha_f32"] = ag.alpha_f32.cpu().numpy().copy()
    for n, g in ag.grads.items():
        out["grad %d" % n] = g.cpu().numpy().copy()
    for n, p in ag.params.items():
        out["param %d" % n] = p.cpu().numpy().copy()
    return out


def _run(name, sizes, waves, monkeypatch):
    """One agent, one update per entry of sizes (max_batch = the largest); the state after each update."""
    ag = _make(name, max(sizes), waves, monkeypatch)
    states = []
    for B in sizes:
        _step(name, ag, _inputs(name, B))
        states.append(_state(ag))
    return states


def _assert_bitwise(name, sizes, monkeypatch):
    ref = _run(name, sizes, 4, monkeypatch)
    got = _run(name, sizes, 8, monkeypatch)
    for i, (r, g) in enumerate(zip(ref, got)):
        for n in (_lib.SPP_NET_ACTOR, _lib.SPP_NET_CRITIC1):
            k = "grad %d" % n
            assert np.isfinite(r[k]).all() and np.abs(r[k]).max() > 0, k
        assert sorted(r) == sorted(g)
        for k in r:
            assert np.array_equal(r[k], g[k]), "update %d (B = %d) %s: %d elements differ" % (
                i, sizes[i], k, int(np.sum(r[k] != g[k])))


# ------------------------------------------------------------------ bit for bit against the 4-wave kernel
@pytest.mark.parametrize("B", [8192, 8193, "4C+1"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_big8_equals_big_bitwise(name, B, monkeypatch):
    _assert_bitwise(name, [_batch_size(B)], monkeypatch)


@pytest.mark.parametrize("name", sorted(SETS))
def test_shrinking_and_growing_batches_bitwise(name, monkeypatch):
    _assert_bitwise(name, [32800, 8192, 8193], monkeypatch)


# ------------------------------------------------------------------ against the float64 oracle
def test_matches_oracle(monkeypatch):
    """B = 8,193: ragged items of 1 to 3 steps through k_dw_big8."""
    monkeypatch.setenv("SPP_DW_BIG_WAVES", "8")
    created = []
    make = spprl.SAC_AcM

    def spy(*a, **kw):
        created.append(make(*a, **kw))
        return created[-1]

    monkeypatch.setattr(spprl, "SAC_AcM", spy)
    bb._sac_update_vs_oracle("Hopper-v2", 11, 3, 8193, False)
    assert _waves_of(created[0]) == 8
