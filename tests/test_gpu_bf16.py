"""SAC_AcM(mlp_bf16=True) against the bf16-rounding oracle (oracle/bf16.py), layer by layer.

The other parity tests used to hold the bf16 kernel sets to the fp32 / float64 oracle, with tolerances wide
enough for the legitimate bf16 rounding (losses 3e-2, per-network gradient 6e-2): a truncating conversion, a
value rounded twice, a dropped bias, a relu mask on the wrong block all fit inside.  Here the reference rounds
where the kernels round, so each case is held to the bounds of bf16_cases.TABLE (max(fp32 figure, 4 x the
reference's own float32-vs-float64 distance): 2e-4 .. 2.7e-3 per tensor, 1e-4 on the losses), per layout
tensor of every network (weights and biases of every layer; relative norm and every-element), and the packed
weight images are checked bit-exactly after the update (check_images).

Each case is one ``ag.update`` with caller-supplied batch and eps.  Batch sizes (tiles of 32 samples):
  1, 31    one tile holding dead rows
  32       exactly one full tile (an odd tile count)
  33       two tiles, one live row in the second
  64       two full tiles
  65, 96   three tiles: odd count with a ragged / a full last tile
  512      ordinary
  8192     the first batch where the 256 x 256 bf16-operand weight gradients run k_dw_big16
           (finalize_dw: Bp >= 8192 and Bp % 64 == 0)
  8224     Bp % 64 == 32: the same jobs fall back to k_dw<true>, ragged 2048-sample slabs for the thin jobs
acm_critic=True / False (B = 33, 512) are two kernel sets (critics on [s | ACM(s, a)] / on [s | a]).  Both run the
one-tile critic phase of sac.hip: the two-tile critic phase of sac_bf.h (odd tile counts repeat a tile there) is an
A/B variant the default library does not contain (SPP_BF16_TWO_TILES = 0, common.h), so no test here reaches it;
the odd / even tile counts are kept so that a build with that variant enabled is exercised by the same cases.
norm_closs and custom_loss are run-time arguments of the same kernels: one case each.

The oracle's actor phase runs against the device's updated critic master (bf16_cases.oracle_update says why), and
that master is itself held to the oracle's own critic Adam step (|d| <= 2 lr; < 0.2 % beyond 1e-5 from B = 512).
The critic targets y cannot be read from the library and are covered through the critic losses.

Shown to bite on scratch builds with one value changed each (B = 32 .. 8192, both envs): truncation instead of RNE
in to_bf16x8 and in op_st / fm_st16, the ACM's fc2 bias dropped, the critics' fc2 input rounded twice with one
bf16 ulp of scale in between (a smaller scale rounds back to the same bf16: bit-identical results), the relu mask
of one D1 output block ignored, the last k-step of the Ant critic's ragged fc1 skipped.  All of them passed the
earlier 6e-2 / 3e-2 checks against the fp32 oracle, except that the last one failed those at B <= 33.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import spprl  # noqa: E402
import bf16_cases as bc  # noqa: E402
from test_gpu_bigbatch import SAC_NETS, snapshot  # noqa: E402
from test_gpu_multistep import check_images  # noqa: E402

DEV = torch.device("cuda:0")


def make_agent(env_name, B, acm_critic, custom_loss, norm_closs, seed=3):
    return spprl.SAC_AcM(env_name=env_name, acm_critic=acm_critic, custom_loss=custom_loss, norm_closs=norm_closs,
                         min_max_denormalize=True, denormalize_actor_out=True, gamma=0.99, max_batch=B,
                         buffer_size=128, device=DEV, seed=seed, mlp_bf16=True)


def bind_minmax(ag, lohi):
    rb = ag.replay_buffer
    rb.min_obs.copy_(torch.from_numpy(lohi[0]))
    rb.max_obs.copy_(torch.from_numpy(lohi[1]))
    rb._have_minmax = True


def run_case(env_name, B, acm_critic=True, custom_loss=0.2, norm_closs=False, steps=1):
    ob, ac = bc.ENVS[env_name]
    rng = np.random.RandomState(B % 1000 + ob)
    ag = make_agent(env_name, B, acm_critic, custom_loss, norm_closs)
    for step in range(1, steps + 1):
        # the oracle of step k starts from the device's fp32 master after step k - 1 (rounded at use, as the
        # library's images are): a later step's gradients are compared on the same weights
        params = snapshot(ag, SAC_NETS)
        before = {k: ag.params[net].clone() for k, net in SAC_NETS.items()}
        batch, e1, e2, lohi = bc.draw_inputs(rng, B, ob, ac)
        bind_minmax(ag, lohi)
        alpha = ag.current_alpha()
        ag.update(*batch, eps_next=e1, eps_cur=e2)
        torch.cuda.synchronize()
        if step < steps:  # an earlier step only has to leave the state behind; it is checked by its own case
            continue
        o = bc.make_oracle(ob, ac, params, lohi, acm_critic=acm_critic, custom_loss=custom_loss, norm_closs=norm_closs,
                           alpha=alpha)
        what = "%s B=%d acm_critic=%s closs=%g norm_closs=%s step %d:" % (env_name, B, acm_critic, custom_loss,
                                                                         norm_closs, step)
        bc.check_bf16_update(ag, SAC_NETS, o, batch, e1, e2, env_name, acm_critic, what, first_step=step == 1)
        assert check_images(ag, True, before) > 0
    return ag


@pytest.mark.parametrize("B", bc.SHAPES)
@pytest.mark.parametrize("env_name", list(bc.ENVS))
def test_bf16_update_matches_rounding_oracle_per_tensor(env_name, B):
    run_case(env_name, B)


@pytest.mark.parametrize("B", [33, 512])
@pytest.mark.parametrize("env_name", list(bc.ENVS))
def test_bf16_update_without_acm_critic_matches_rounding_oracle(env_name, B):
    run_case(env_name, B, acm_critic=False)


@pytest.mark.parametrize("custom_loss,norm_closs", [(0.2, True), (0.0, False)])
def test_bf16_update_loss_variants_match_rounding_oracle(custom_loss, norm_closs):
    run_case("Ant-v2", 96, custom_loss=custom_loss, norm_closs=norm_closs)


def test_bf16_second_update_on_repacked_images_matches_rounding_oracle():
    """Two consecutive updates at B = 96 (Ant): the second runs on images re-packed from the updated master and on
    non-zero Adam moments; its per-tensor gradients against the oracle's step from the same master."""
    ag = run_case("Ant-v2", 96, steps=2)
    assert float(ag.exp_avg[SAC_NETS["actor"]].abs().max()) > 0
