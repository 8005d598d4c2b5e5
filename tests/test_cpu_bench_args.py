"""bench.py argument checks that need no GPU: --replicas is the configs[0] (vanilla SAC) layout on one GPU only,
and the parent process refuses other configs before touching the device."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_replicas_only_for_the_vanilla_config():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--config", "sac_hopper", "--replicas", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, r.stderr[-2000:]
    assert "--replicas is for --config vanilla_sac_hcheetah" in r.stderr


_DUMP = """
import os, sys
import numpy as np
import torch
import bench
d = sys.argv[1]
arrays = {"w": torch.arange(6, dtype=torch.float32).reshape(2, 3), "i": np.arange(4), "l": np.array([0.1]),
          "big": np.arange(5000, dtype=np.float32)}
bench.DUMP_BYTES = 4 * 1024  # a share of 1 KiB per array: "big" (20 KB) is sampled, the others are whole
for sub in ("a", "b"):
    bench.dump_outputs(os.path.join(d, sub), arrays)
got = {n: np.load(os.path.join(d, "a", n + ".npy")) for n in arrays}
assert got["w"].dtype == np.float32 and got["w"].shape == (2, 3) and (got["w"] == arrays["w"].numpy()).all()
assert got["i"].dtype == np.float32 and (got["i"] == np.arange(4)).all()
assert got["l"].dtype == np.float64 and got["l"][0] == 0.1
big = got["big"]
assert big.dtype == np.float32 and big.shape == (256,) and (np.diff(big) > 0).all()  # values = sorted indices
assert (big == np.load(os.path.join(d, "b", "big.npy"))).all()  # the same sample every time
assert sum(v.nbytes for v in got.values()) <= bench.DUMP_BYTES
print("ok")
"""


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path):
    """bench.dump_outputs (--dump-outputs): float64 stays, everything else becomes float32, an array over its
    share of the byte budget is cut to a fixed sample.  In a child process: importing bench sets the HIP queue
    count for its process."""
    r = subprocess.run([sys.executable, "-c", _DUMP, str(tmp_path)], cwd=REPO, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


def test_full_and_dump_outputs_are_options():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
