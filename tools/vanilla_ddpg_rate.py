#!/usr/bin/env python
"""Rate of vanilla DDPG (spprl.DDPG) at the reference cadence: 1 env, B = 100, 50 grad steps every 50 frames
(train/vanilla_ddpg_hcheetah.py), on SynthVecEnv, past random_frames.

    python tools/vanilla_ddpg_rate.py [--frames 2000] [--warmup 200] [--rounds 2]

The parent runs the team (small-batch kernels, csrc/ddpg_team.h) and SPP_SAC_TEAM=0 (one-wave kernels) variants
as separate child processes, alternated ``rounds`` times each, and prints every run's line, then per variant the
mean env-steps/s and the run-to-run spread (max - min) / mean.  A child (--child) warms up, times ``frames``
frames one by one as bench.py's vanilla_sac_hcheetah step does (act -> env -> replay -> make_update, obs
statistics once per 1000 frames) ending in a device synchronise, and prints one JSON line with env-steps/s and
the per-phase kernel time per launch (HIP events around the launches, sppAgentSetTiming).
The replay ring is not prefilled (bench.py's lines sample a 990K-row ring): the gather's rows are cache-resident here.
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


def child(args):
    import torch

    import spprl
    from spprl import flops

    dev = torch.device("cuda:0")
    ag = spprl.DDPG(env_name="HalfCheetah-v2", gamma=0.99, actor_lr=1e-3, critic_lr=1e-3, update_batch_size=100,
                    update_freq=50, grad_steps=50, random_frames=100, batch_size=1000, iterations=10 ** 9,
                    buffer_size=1_000_000, max_batch=128, device=dev, seed=0, n_envs=1, loop_seed=1000)
    assert ag.schedule == "reference"
    ag._start_episodes()
    since_stats = [0]

    def step():  # one frame of DDPG.collect_batch_and_train (ddpg.py:192-223) with make_update
        end = ag._vector_step()
        ag.make_update()
        if bool(end[0]):
            ag._start_episodes()
        since_stats[0] += 1
        if since_stats[0] == 1000:  # perform_iteration's update_obs_mean_std, once per batch_size frames
            ag.update_obs_stats()
            since_stats[0] = 0

    while ag.stats_logger.frames < ag.random_frames + 101:  # past random_frames, the ring beyond one batch
        step()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ag.set_timing(True)
    ag.get_timing()  # clear
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.frames):
        step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    ms, cnt = ag.get_timing()
    names = ["critic_phase", "actor_phase", "dw_gemm", "adam"]
    mac = flops.ddpg_macs(17, 6, aout=6, acm_critic=False, with_acm=False)
    print(json.dumps({
        "variant": "one_wave" if os.environ.get("SPP_SAC_TEAM") == "0" else "team",
        "env_steps_per_s": round(args.frames / elapsed, 1), "frames": args.frames, "elapsed_s": round(elapsed, 4),
        "grad_steps": int(cnt[0]),
        "kernel_us_per_launch": {n: round(1e3 * ms[i] / max(cnt[i], 1), 2) for i, n in enumerate(names)},
        "launches": {n: int(cnt[i]) for i, n in enumerate(names)},
        "update_mflop_per_grad_step": round(2e-6 * mac["update"] * 100, 2),
        "loss": {k: round(v, 6) for k, v in ag.loss.items()}}), flush=True)


def parent(args):
    runs = {"team": [], "one_wave": []}
    for _ in range(args.rounds):
        for variant in ("team", "one_wave"):  # alternated: drift of the machine shows in both
            env = dict(os.environ, SPP_SAC_TEAM="0" if variant == "one_wave" else "1")
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--frames", str(args.frames),
                                  "--warmup", str(args.warmup)], env=env, stdout=subprocess.PIPE, text=True,
                                 timeout=args.child_timeout)
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
                            "kernel_us_per_launch": rs[-1]["kernel_us_per_launch"]}
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.frames < 2000 and not a.child:
        ap.error("--frames: at least 2000")
    (child if a.child else parent)(a)
