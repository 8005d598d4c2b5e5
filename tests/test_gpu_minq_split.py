"""GPU parity of the min-critic split of the SAC actor phase (csrc/sac.hip: k_sac_actor_phase<C, true>,
k_minq_scan / k_minq_scatter, k_sac_minq_backward, k_sac_actor_heads<C, true>).

The actor loss uses min(Q1, Q2), so per sample only the critic that took the min (both, with 1/2 each, on an exact
tie) has a non-zero upstream gradient.  The split regroups the samples by chosen critic over the whole batch and
runs each critic's backward on its own list only.  The cases are the smallest that can break the hand-over: one
live sample, ragged tiles, lists shorter than one 32-entry group, an empty list beside a ragged one (forced
selections), every sample in both lists (exact ties), every kernel-set family that instantiates the split (narrow
and wide heads, with and without the ACM in front of the critics, vanilla SAC through the one-wave kernels), and
one batch of 4 * CUs + 1 tiles, so that one wave runs a second tile and a second group.

Against the float64 oracle with tests/test_gpu_bigbatch.py's fp32 tolerances: losses rtol 1e-4, gradient norms
2e-4 per network and per layout tensor, elements bf16_cases.fp32_elem_tol.  Against the one-kernel phase
(an agent made under SPP_MINQ_SPLIT=0, same seed and inputs): the actor gradient, every loss and every parameter
after the step, bit for bit.
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
import test_gpu_gen_inputs as gi  # noqa: E402
from oracle.sac import OracleSac  # noqa: E402
from oracle.sac_acm import OracleSacAcm  # noqa: E402

DEV = bb.DEV
F64 = torch.float64
N = bb.SAC_NETS


# ------------------------------------------------------------------ random parameters, against the oracle
@pytest.mark.parametrize("B", [1, 31, 33, 100])
def test_hopper_matches_oracle(B):
    bb._sac_update_vs_oracle("Hopper-v2", 11, 3, B, False, params_check=False)


def test_hopper_plain_critic_matches_oracle():
    bb._sac_update_vs_oracle("Hopper-v2", 11, 3, 33, "acmc0", params_check=False)


def test_hcheetah_matches_oracle():
    bb._sac_update_vs_oracle("HalfCheetah-v2", 17, 6, 33, False, params_check=False)


def test_ant_wide_heads_match_oracle():
    bb._sac_update_vs_oracle("Ant-v2", 111, 8, 33, False, params_check=False)


def test_vanilla_sac_one_wave_kernels_match_oracle(monkeypatch):
    gi._vanilla_update_vs_oracle(100, monkeypatch)


def test_hopper_second_tile_and_group_per_wave_matches_oracle():
    bb._sac_update_vs_oracle("Hopper-v2", 11, 3, gi.second_tile_batch(), False, params_check=True)


# ------------------------------------------------------------------ chosen selections
def _agent(B, seed=3):
    return spprl.SAC_AcM(env_name="Hopper-v2", acm_critic=True, custom_loss=0.2, norm_closs=False,
                         min_max_denormalize=True, denormalize_actor_out=True, gamma=0.99, max_batch=B,
                         buffer_size=128, device=DEV, seed=seed)


def _shape(ag, mode):
    """random: as initialised.  force1 / force2: the other critic is this one plus 100 on its fc3 bias, so every
    sample's min is critic 1 / critic 2 (Q is O(1); the critic step in front of the actor phase moves a parameter
    by ~1e-3).  tie: critic 2 and its target are critic 1 and its target, so both take identical steps and
    q1 == q2 bit for bit."""
    if mode in ("force1", "force2"):
        src, dst = ("critic_1", "critic_2") if mode == "force1" else ("critic_2", "critic_1")
        st = ag.net_state(N[src])
        st["fc3.bias"] = st["fc3.bias"] + 100.0
        ag.load_net(N[dst], st)
    elif mode == "tie":
        ag.load_net(N["critic_2"], ag.net_state(N["critic_1"]))
        ag.load_net(N["critic_2_targ"], ag.net_state(N["critic_1_targ"]))


def _inputs(B, ob=11, ac=3):
    rng = np.random.RandomState(B % 1000 + ob + 1)
    lo = -rng.uniform(0.5, 2, ob).astype(np.float32)
    hi = rng.uniform(0.5, 2, ob).astype(np.float32)
    batch = bb.random_batch(rng, B, ob, ob, ac)
    return lo, hi, batch, rng.randn(B, ob).astype(np.float32), rng.randn(B, ob).astype(np.float32)


def _step(ag, inp):
    lo, hi, batch, e1, e2 = inp
    rb = ag.replay_buffer
    rb.min_obs.copy_(torch.from_numpy(lo))
    rb.max_obs.copy_(torch.from_numpy(hi))
    rb._have_minmax = True
    ag.update(*batch, eps_next=e1, eps_cur=e2)
    torch.cuda.synchronize()


def _vs_oracle(B, mode):
    ag = _agent(B)
    _shape(ag, mode)
    params = bb.snapshot(ag, N)
    inp = _inputs(B)
    _step(ag, inp)
    lo, hi, batch, e1, e2 = inp
    norm = bb.Norm(True, torch.from_numpy(lo), torch.from_numpy(hi))
    o = OracleSacAcm(11, 11, 3, acm_critic=True, custom_loss=0.2, norm_closs=False, norm=norm, actor_lim=1.0,
                     acm_lim=np.ones(3, np.float32), gamma=0.99, params=params, dtype=F64)
    bb.check_sac(ag, o, o.update(*batch, e1, e2), grad_tol=2e-4, loss_tol=1e-4, params_check=False)
    return ag


@pytest.mark.parametrize("mode", ["force1", "force2"])
def test_forced_selection_matches_oracle(mode):
    """One list is empty, the other holds all 100 samples: 4 groups, the last one ragged."""
    _vs_oracle(100, mode)


def test_exact_ties_match_oracle():
    """Every sample is in both lists with 1/2."""
    ag = _vs_oracle(33, "tie")
    for k in ("critic_1", "critic_1_targ"):  # the premise: the critics took identical steps, so q1 == q2 held
        a = ag.params[N[k]].cpu().numpy()
        b = ag.params[N[k.replace("_1", "_2")]].cpu().numpy()
        assert np.array_equal(a, b), k


# ------------------------------------------------------------------ bit for bit against the one-kernel phase
def _bitwise_cases():
    return [(33, "random"), (100, "random"), ("second_tile", "random"), (100, "force1"), (100, "force2"), (33, "tie")]


@pytest.mark.parametrize("B,mode", _bitwise_cases())
def test_split_equals_one_kernel_phase_bitwise(B, mode, monkeypatch):
    if B == "second_tile":
        B = gi.second_tile_batch()
    inp = _inputs(B)
    out = []
    for split in ("0", "1"):
        monkeypatch.setenv("SPP_MINQ_SPLIT", split)  # read when the agent is made
        ag = _agent(B)
        _shape(ag, mode)
        _step(ag, inp)
        out.append((ag.grads[N["actor"]].cpu().numpy(), ag._losses.detach().cpu().numpy().copy(),
                    {k: ag.params[n].cpu().numpy() for k, n in N.items()}))
    (g0, l0, p0), (g1, l1, p1) = out
    assert np.isfinite(g0).all() and np.abs(g0).max() > 0
    assert np.array_equal(g0, g1), "actor gradient: %d elements differ" % int(np.sum(g0 != g1))
    assert np.array_equal(l0, l1), (l0, l1)
    for k in p0:
        assert np.array_equal(p0[k], p1[k]), k
