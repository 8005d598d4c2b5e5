#!/usr/bin/env python
"""Rate of vanilla A2C (spprl.A2C) on SynthVecEnv, whole iterations, at two cadences:
  reference   rltoolkit's A2C defaults (a2c.py:17-27, config.py): 1 env, batch_size = 200 (whole episodes), actor_lr =
              3e-3, critic_lr = 3e-4, 10 targets x 10 critic steps, obs_norm_alpha = 0.99, gamma = 0.95
  wide        4096 lockstep envs, one step per iteration (batch_size = 4096), the same update

    python tools/vanilla_a2c_rate.py [--iters N] [--warmup 5] [--rounds 3] [--cadence reference|wide|both]

The parent runs the two variants of the advantage as separate child processes, alternated ``rounds`` times each,
prints every run's line, then per cadence and variant the mean env-steps/s with the run-to-run spread
(max - min) / mean and the update tail's time:
  fused     spprl.A2C as it comes: sppOnpTdAdvantage (both critic passes, targets, advantages, moments: one launch
            and a one-workgroup finish)
  unfused   SPP_A2C_FUSED_ADV=0: two sppOnpValue launches, torch arithmetic, the moments by torch
A child (--child) warms up, then times ``iters`` whole iterations (collect_batch + update) with a host clock around
work that ends in a device synchronise; HIP events on the stream bracket the update tail -- from the critic targets
of calculate_advantage (after update_critic) to the actor's Adam step.  It prints one JSON line.
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

VARIANTS = {"fused": "1", "unfused": "0"}  # name: SPP_A2C_FUSED_ADV
CADENCES = {"reference": dict(n_envs=1, batch_size=200), "wide": dict(n_envs=4096, batch_size=4096)}
ITERS = {"reference": 60, "wide": 400}  # timed iterations: 60 whole 1000-frame episodes / 400 steps of 4096 envs


def child(args):
    import torch

    import spprl

    dev = torch.device("cuda:0")
    ag = spprl.A2C(env_name="HalfCheetah-v2", iterations=10 ** 9, device=dev, seed=0, loop_seed=1000,
                   **CADENCES[args.cadence])
    tail = []  # (start, end) events around td_advantage .. pg_actor_step of every update
    td, pg = ag.nets.td_advantage, ag.nets.pg_actor_step

    def td_timed(*a, **k):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        tail.append([e, None])
        return td(*a, **k)

    def pg_timed(*a, **k):
        out = pg(*a, **k)
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        tail[-1][1] = e
        return out

    ag.nets.td_advantage, ag.nets.pg_actor_step = td_timed, pg_timed
    for _ in range(args.warmup):
        ag.update(ag.collect_batch())
    torch.cuda.synchronize()
    del tail[:]
    frames0 = ag.stats_logger.frames
    t0 = time.perf_counter()
    for _ in range(args.iters):
        ag.update(ag.collect_batch())
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    frames = ag.stats_logger.frames - frames0
    tail_ms = sorted(a.elapsed_time(b) for a, b in tail)
    print(json.dumps({
        "cadence": args.cadence, "variant": args.variant, "env_steps_per_s": round(frames / elapsed, 1),
        "frames": frames, "iterations": args.iters, "elapsed_s": round(elapsed, 4),
        "iter_ms": round(1e3 * elapsed / args.iters, 3),
        "tail_us_mean": round(1e3 * sum(tail_ms) / len(tail_ms), 1),
        "tail_us_median": round(1e3 * tail_ms[len(tail_ms) // 2], 1),
        "loss": {k: round(float(v), 6) for k, v in ag.loss.items()}}), flush=True)


def parent(args):
    cadences = list(CADENCES) if args.cadence == "both" else [args.cadence]
    runs = {(c, v): [] for c in cadences for v in VARIANTS}
    for _ in range(args.rounds):
        for c in cadences:
            for variant, flag in VARIANTS.items():  # alternated: drift of the machine shows in every variant
                env = dict(os.environ, SPP_A2C_FUSED_ADV=flag)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--variant", variant, "--cadence", c,
                       "--iters", str(args.iters or ITERS[c]), "--warmup", str(args.warmup)]
                out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
                if out.returncode != 0:
                    sys.exit("child (%s, %s) exited %d" % (c, variant, out.returncode))
                line = out.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                runs[(c, variant)].append(json.loads(line))
    summary = {}
    for (c, variant), rs in runs.items():
        v = [r["env_steps_per_s"] for r in rs]
        mean = sum(v) / len(v)
        summary["%s/%s" % (c, variant)] = {
            "env_steps_per_s_mean": round(mean, 1), "runs": v, "spread": round((max(v) - min(v)) / mean, 4),
            "tail_us_median": [r["tail_us_median"] for r in rs], "tail_us_mean": [r["tail_us_mean"] for r in rs],
            "iter_ms": [r["iter_ms"] for r in rs]}
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=None, help="timed iterations (default: ITERS per cadence)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cadence", choices=sorted(CADENCES) + ["both"], default="both")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--variant", choices=sorted(VARIANTS), default="fused")
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.rounds < 2 and not a.child:
        ap.error("--rounds: at least 2")
    if a.child and a.cadence == "both":
        ap.error("--child needs one cadence")
    if a.child and a.iters is None:
        a.iters = ITERS[a.cadence]
    (child if a.child else parent)(a)
