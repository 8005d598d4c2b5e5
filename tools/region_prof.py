"""Region timing of the SAC phase kernels (profiling build: python spp-rl_amd/build.py --prof).
Usage: SPPRL_LIB=spp-rl_amd/spprl/libspprl_prof.so python tools/region_prof.py"""
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "spp-rl_amd"), REPO]
import torch  # noqa: E402

import spprl  # noqa: E402
from spprl import _lib  # noqa: E402

# Kernel sets built with the register hand-over (SPP_GEN_INPUTS, csrc/common.h; the fp32 narrow-input sets) produce
# the critics' fc1 output and delta2 inside the consumer layer: the "L1" regions then hold only the first fragment
# request, the "delta staging" regions nothing, and their work is counted in the following L2 / W2T region.
# With the stage split (SPP_STAGE_SPLIT, csrc/sac.hip) the slots keep their stages and name the kernel that now runs them:
# T = k_sac_trunk_fwd, S = k_sac_squash_stage / k_sac_heads_stage (3 workgroups per CU: a slot's cycles are the
# wave's own, while two other waves share its SIMD), R = the rest kernels (k_sac_critic_phase<C, true>,
# k_sac_actor_phase<C, true, true>, k_sac_actor_trunk_bwd), whose "tile start" slots hold the hand-over read-backs.
NAMES = {0: "tile start (R: + SCA / SLP read-back)", 1: "actor L1 (T; SPP_ACTOR_GEN & 1: request only)", 2: "actor L2 (T; gen: + L1)", 3: "actor heads (T: -> THD)",
         4: "squash (S: + THD read-back)", 5: "ACM + target input (S: -> SCA / SLP)",
         6: "targ1 L1 (gen: request only)", 7: "targ1 L2 (gen: + L1)", 8: "targ2 L1 (gen: request only)",
         9: "targ2 L2 (gen: + L1)", 10: "y + critic input", 11: "critic L1 (gen: request only)",
         12: "critic L2 (gen: + L1)", 13: "delta2 staging (gen: fc3 gradient only)", 14: "critic W2T (gen: + delta2)",
         15: "tile end",
         20: "dense_lds prologue | A: delta staging (nodense; gen: none)",
         21: "dense_lds loop | A: W2T (nodense; gen: + delta2)",
         22: "dense_lds epilogue | A: W1Ta (nodense)",
         23: "dense prologue | A: ACM bwd input (nodense)", 24: "dense mfma | A: ACM W3T (nodense)",
         25: "dense epilogue | A: ACM W2T (nodense)",
         26: "A: tile start (R: + SCA / SLP read-back)", 27: "A: actor trunk (T: -> ADH, MASK)",
         28: "A: squash (S: + ADH read-back)", 29: "A: ACM fwd (S: -> SCA / SLP)", 19: "A: q min",
         30: "A: critics L1 (fwd; gen: request only)",
         31: "A: critics L2 (fwd; gen: + L1) | DCA read-back (S)", 16: "A: ACM bwd (S)",
         17: "A: heads bwd (S) | ADH read-back (R)", 18: "A: trunk bwd (R; SPP_ACTOR_GEN & 2: WhT under W2T)"}


def main():
    """argv[1]: hopper (default) | ant_bf16 (build with --prof --bf16-only)"""
    dev = torch.device("cuda", 0)
    E, B = 4096, 409600
    cfg = sys.argv[1] if len(sys.argv) > 1 else "hopper"
    env, ob, ac, bf = {"hopper": ("Hopper-v2", 11, 3, False), "ant_bf16": ("Ant-v2", 111, 8, True)}[cfg]
    ag = spprl.SAC_AcM(env_name=env, acm_critic=True, custom_loss=0.2, norm_closs=False,
                       min_max_denormalize=True, denormalize_actor_out=True, max_batch=B, buffer_size=200_000,
                       device=dev, seed=0, mlp_bf16=bf)
    rb = ag.replay_buffer
    n = 150_000
    slots = rb.add_obs_batch(torch.randn(n + 1, ob, device=dev))
    rb.add_timestep_batch(slots[:n], slots[1:], torch.randn(n, ob, device=dev), torch.randn(n, device=dev),
                          torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
                          torch.rand(n, ac, device=dev) * 2 - 1)
    rb.update_obs_mean_std()
    idx = torch.randint(0, n, (B,), device=dev)
    buf = (ctypes.c_ulonglong * 64)()
    for it in range(4):
        if it == 1:
            _lib.call("sppDebugReadProf", buf, 1)
        ag.update_from_replay_dp(idx, 1, it)
    torch.cuda.synchronize()
    _lib.call("sppDebugReadProf", buf, 0)
    t = np.array(buf[:32], np.float64)
    tiles = 3 * (B // 32)
    tot = t.sum()
    print("%s: both phases, cycles per tile (%d tiles per phase): total %.0f" % (cfg, tiles, tot / tiles))
    for k in [k for k in NAMES if t[k] > 0]:
        print("  %2d %-20s %9.0f  %5.1f%%" % (k, NAMES[k], t[k] / tiles, 100 * t[k] / tot))


if __name__ == "__main__":
    main()
