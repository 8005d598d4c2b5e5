"""GPU parity of the wave-pair forms of the SAC phase kernels (csrc/sac.hip): a tile's two critics on the two
waves of a pair, the q values crossing through an LDS slot behind one barrier per iteration:
  bit 0  k_sac_critic_phase<C, true>      -> k_sac_critic_phase<C, true, true>       (stage-split cut 3)
  bit 1  k_sac_actor_phase<C, true, true> -> k_sac_actor_phase<C, true, true, true>  (stage-split cut 2)

No arithmetic changes and the fused fc3 slabs hold the same sums of the same tiles in the same order, so the check
is bit for bit: an agent made under SPP_CRITIC_PAIRS = 1, 2 and 3 against one made under 0 (same seed, same
inputs), after one full update: both critics' gradients, the actor gradient, every loss, alpha and every
parameter are identical.  Every case asserts through sppAgentCriticPairs that the paired agent runs the pair
kernels and the reference agent does not.

The batches are the smallest that can break the mapping.  With P = 2 * CUs pairs in a full grid:
  B = 1, 31, 33, 100   ragged tiles; one workgroup, so an idle pair beside a working one (1 .. 2 tiles) and, at
                       4 tiles over 2 pairs, a second iteration: both fc3 accumulator sets
  P + 1 tiles          one pair runs a second iteration, every other pair only reaches its barrier
  2 P + 1 tiles        a third iteration: the even accumulator set is used again
  3 P + 3 tiles        the remainder lands in both halves of the grid
on the kernel sets of tests/test_gpu_stage_split.py (Hopper with and without the ACM in front of the critics,
HalfCheetah, the 3-dim set, vanilla SAC through the one-wave kernels), with the forced and tied critic selections
of tests/test_gpu_minq_split.py, and over three updates of shrinking and growing batches on one agent.  One case
runs against the float64 oracle with tests/test_gpu_bigbatch.py's tolerances.
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
import test_gpu_minq_split as mq  # noqa: E402
import test_gpu_stage_split as ss  # noqa: E402
from spprl import _lib  # noqa: E402

PAIRS = [1, 2, 3]
SETS = ss.SETS


def pairs_in_grid():
    """P: the pairs of a full phase grid (one workgroup of 4 waves = 2 pairs per CU)."""
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def _batch_size(B):
    P = pairs_in_grid()
    return {"P+1": 32 * (P + 1), "2P+1": 32 * (2 * P + 1), "3P+3": 32 * (3 * P + 3)}[B] if isinstance(B, str) else B


def _pairs_of(ag):
    got = ctypes.c_int(-1)
    _lib.call("sppAgentCriticPairs", ag._h, ctypes.byref(got))
    return got.value


def _make(name, max_batch, bits, monkeypatch):
    cls, env, ob, aout, ac, kw = SETS[name]
    monkeypatch.setenv("SPP_SAC_TEAM", "0")  # read when the agent is made: the one-wave kernels at every batch
    monkeypatch.delenv("SPP_STAGE_SPLIT", raising=False)  # every cut (the default)
    monkeypatch.setenv("SPP_CRITIC_PAIRS", str(bits))
    ag = cls(env_name=env, max_batch=max_batch, buffer_size=128, device=bb.DEV, seed=3, **kw)
    cuts = ctypes.c_int(-1)
    _lib.call("sppAgentStageSplit", ag._h, ctypes.byref(cuts))
    assert cuts.value == 7, "the agent runs cuts %d: the pair forms sit behind cuts 2 and 3" % cuts.value
    assert _pairs_of(ag) == bits, "the agent runs pair forms %d, asked for %d" % (_pairs_of(ag), bits)
    return ag


def _run(name, sizes, mode, bits, monkeypatch):
    """One agent, one update per entry of sizes (max_batch = the largest); the state after each update."""
    ag = _make(name, max(sizes), bits, monkeypatch)
    if mode != "random":
        mq._shape(ag, mode)
    states = []
    for B in sizes:
        ss._step(name, ag, ss._inputs(name, B))
        states.append(ss._state(name, ag))
    return states


_REF = {}


def _reference(name, sizes, mode, monkeypatch):
    """The SPP_CRITIC_PAIRS=0 agent's states, computed once per (set, sizes, mode) and shared by the bit sets."""
    key = (name, tuple(sizes), mode)
    if key not in _REF:
        _REF[key] = _run(name, sizes, mode, 0, monkeypatch)
    return _REF[key]


def _assert_bitwise(name, sizes, mode, bits, monkeypatch):
    ref = _reference(name, sizes, mode, monkeypatch)
    got = _run(name, sizes, mode, bits, monkeypatch)
    for i, (r, g) in enumerate(zip(ref, got)):
        for k in ("grad critic_1", "grad critic_2", "grad actor"):
            assert np.isfinite(r[k]).all() and np.abs(r[k]).max() > 0, k
        for k in r:
            assert np.array_equal(r[k], g[k]), "update %d (B = %d) %s: %d elements differ" % (
                i, sizes[i], k, int(np.sum(r[k] != g[k])))


# ------------------------------------------------------------------ bit for bit against the unpaired kernels
@pytest.mark.parametrize("bits", PAIRS)
@pytest.mark.parametrize("B", [1, 31, 33, 100, "P+1", "2P+1", "3P+3"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_pairs_equal_unpaired_kernels_bitwise(name, B, bits, monkeypatch):
    _assert_bitwise(name, [_batch_size(B)], "random", bits, monkeypatch)


@pytest.mark.parametrize("bits", PAIRS)
@pytest.mark.parametrize("B,mode", [(100, "force1"), (100, "force2"), (33, "tie")])
def test_chosen_selections_bitwise(B, mode, bits, monkeypatch):
    _assert_bitwise("hopper", [B], mode, bits, monkeypatch)


@pytest.mark.parametrize("bits", PAIRS)
@pytest.mark.parametrize("name", ["hopper", "hcheetah"])
def test_shrinking_and_growing_batches_bitwise(name, bits, monkeypatch):
    _assert_bitwise(name, [100, 33, 100], "random", bits, monkeypatch)


# ------------------------------------------------------------------ against the float64 oracle
def test_matches_oracle(monkeypatch):
    """B = 100: 4 tiles over the 2 pairs of one workgroup, two iterations each."""
    monkeypatch.setenv("SPP_SAC_TEAM", "0")
    monkeypatch.delenv("SPP_STAGE_SPLIT", raising=False)
    monkeypatch.setenv("SPP_CRITIC_PAIRS", str(max(PAIRS)))
    created = []
    make = spprl.SAC_AcM

    def spy(*a, **kw):
        created.append(make(*a, **kw))
        return created[-1]

    monkeypatch.setattr(spprl, "SAC_AcM", spy)
    bb._sac_update_vs_oracle("Hopper-v2", 11, 3, 100, False, params_check=False)
    assert _pairs_of(created[0]) == max(PAIRS)
