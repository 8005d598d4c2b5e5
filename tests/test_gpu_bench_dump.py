"""bench.py's plain run and --dump-outputs on the GPU, at a small shape.

A plain run (no --full) prints the headline line only: no CPU baseline, no profiler children, no HBM-kernel
launches after the timed region.  --dump-outputs DIR writes what the last timed step left as float32 / float64
.npy files; the seeds are fixed, so a second run with the same arguments starts from the same inputs and (the
kernels being deterministic, as test_gpu_dp_rccl's checksum comparison already requires) writes the same arrays.
"""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--envs", "1024", "--buffer",
           "200000", "--dump-outputs", out_dir]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    arrays = {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(out_dir, "*.npy")))}
    return json.loads(lines[0]), arrays


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_steps_outputs(tmp_path):
    res, a = _bench(str(tmp_path / "a"))
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(1024 * 1e3 / res["ms_per_step"], rel=1e-3)
    for k in ("metric", "unit", "higher_is_better", "dtype", "losses", "param_checksum", "roofline"):
        assert k in res, k
    for k in ("cpu_baseline", "hbm_kernels", "pmc_bytes_per_launch"):
        assert k not in res, k
    assert "frac_rocprof" not in res["roofline"] and res["roofline"]["traffic"] is None

    nets = ["actor", "critic_1", "critic_2", "critic_1_targ", "critic_2_targ", "acm"]
    want = {"params_" + n for n in nets} | {"grads_" + n for n in ("actor", "critic_1", "critic_2", "acm")} | \
        {"loss_" + k for k in res["losses"]} | {"obs"}
    assert set(a) == want
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name, v in a.items():
        assert v.dtype in (np.float32, np.float64), name
        assert np.isfinite(v).all(), name
    assert a["obs"].shape == (1024, 11)
    assert a["params_critic_1"].shape == a["grads_critic_1"].shape and np.abs(a["grads_critic_1"]).max() > 0
    for k, v in res["losses"].items():  # the line prints the same losses, rounded to 5 decimals
        assert a["loss_" + k].shape == (1,) and abs(a["loss_" + k][0] - v) <= 0.5e-5 + 1e-12, k

    res_b, b = _bench(str(tmp_path / "b"))
    assert res_b["param_checksum"] == res["param_checksum"]
    assert set(b) == set(a)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
