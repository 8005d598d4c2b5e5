#!/usr/bin/env python
"""Rate of vanilla PPO (spprl.PPO) at the reference cadence (train/vanilla_ppo_hcheetah.py): 1 env, batch_size =
2000 (whole 1000-frame episodes), ppo_batch_size = 512, max_ppo_epochs = 10, kl_div_threshold = 0.1, actor_lr =
3e-4, critic_lr = 1e-3, obs_norm_alpha = 0.95, gamma = 0.99, on SynthVecEnv, whole iterations.

    python tools/vanilla_ppo_rate.py [--iters 40] [--warmup 3] [--rounds 3]

The parent runs four variants as separate child processes, alternated ``rounds`` times each, prints every run's
line, then per variant the mean env-steps/s and the run-to-run spread (max - min) / mean:
  default         spprl.PPO as it comes: fused rollout act (sppOnpRolloutAct), actor minibatch steps one by one
                  (sppOnpActorGrads / Apply)
  epoch_kernel    default + SPP_PPO_EPOCH_KERNEL=1: one-launch actor epochs (sppOnpActorEpoch)
  baseline        SPP_PPO_FUSED_ACT=0: sppObsNormalize + sppRandNormal + sppOnpAct per frame, per-minibatch steps --
                  what the pieces before the fused act and the aout != ob epoch kernel cost
  unfused_epoch   baseline + SPP_PPO_EPOCH_KERNEL=1
A child (--child) warms up, then times ``iters`` whole iterations (collect_batch + update) with a host clock around
work that ends in a device synchronise, and the rollout / update split with HIP events on the stream; it prints
one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "spp-rl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

VARIANTS = {  # name: (SPP_PPO_FUSED_ACT, SPP_PPO_EPOCH_KERNEL)
    "default": ("1", "0"), "epoch_kernel": ("1", "1"), "baseline": ("0", "0"), "unfused_epoch": ("0", "1")}


def child(args):
    import torch

    import spprl

    dev = torch.device("cuda:0")
    ag = spprl.PPO(env_name="HalfCheetah-v2", gamma=0.99, actor_lr=3e-4, critic_lr=1e-3, batch_size=2000,
                   ppo_batch_size=512, kl_div_threshold=0.1, max_ppo_epochs=10, entropy_coef=0.0, obs_norm_alpha=0.95,
                   iterations=10 ** 9, n_envs=1, device=dev, seed=0, loop_seed=1000)
    assert ag.nets._epoch_kernel_ok(512) == (VARIANTS[args.variant][1] == "1")
    for _ in range(args.warmup):
        ag.update(ag.collect_batch())
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.iters)]
    frames0, epochs = ag.stats_logger.frames, 0
    t0 = time.perf_counter()
    for e in ev:
        e[0].record()
        mem = ag.collect_batch()
        e[1].record()
        ag.update(mem)
        e[2].record()
        epochs += ag.nets.last_epochs
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    frames = ag.stats_logger.frames - frames0
    roll = sum(e[0].elapsed_time(e[1]) for e in ev)
    upd = sum(e[1].elapsed_time(e[2]) for e in ev)
    print(json.dumps({
        "variant": args.variant, "env_steps_per_s": round(frames / elapsed, 1), "frames": frames,
        "iterations": args.iters, "elapsed_s": round(elapsed, 4),
        "rollout_ms_per_iter": round(roll / args.iters, 2), "update_ms_per_iter": round(upd / args.iters, 2),
        "rollout_us_per_frame": round(1e3 * roll / frames, 2), "actor_epochs_per_iter": round(epochs / args.iters, 2),
        "loss": {k: round(float(v), 6) for k, v in ag.loss.items()}}), flush=True)


def parent(args):
    runs = {v: [] for v in VARIANTS}
    for _ in range(args.rounds):
        for variant, (fused, epoch) in VARIANTS.items():  # alternated: drift of the machine shows in every variant
            env = dict(os.environ, SPP_PPO_FUSED_ACT=fused, SPP_PPO_EPOCH_KERNEL=epoch)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--variant", variant,
                                  "--iters", str(args.iters), "--warmup", str(args.warmup)], env=env,
                                 stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
            if out.returncode != 0:
                sys.exit("child (%s) exited %d" % (variant, out.returncode))
            line = out.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            runs[variant].append(json.loads(line))
    summary = {}
    for variant, rs in runs.items():
        v = [r["env_steps_per_s"] for r in rs]
        mean = sum(v) / len(v)
        summary[variant] = {"env_steps_per_s_mean": round(mean, 1), "runs": v,
                            "spread": round((max(v) - min(v)) / mean, 4),
                            "rollout_ms_per_iter": [r["rollout_ms_per_iter"] for r in rs],
                            "update_ms_per_iter": [r["update_ms_per_iter"] for r in rs]}
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)  # (80,000 frames: a window of 5-8 s)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--variant", choices=sorted(VARIANTS), default="default")
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.rounds < 2 and not a.child:
        ap.error("--rounds: at least 2")
    (child if a.child else parent)(a)
