"""GPU parity of k_dw_thin (csrc/dw.hip), the LDS-staged kernel of the thin fp32 weight-gradient jobs (one side of
the gradient a single 32-block, two sample parts per item), against k_dw<false>, which ran those items before it and
still does under SPP_DW_THIN=0.

The claim is identical order, not a bound: every 32 x 32 block of every slab accumulates the same MFMA chain over the
same samples in the same order, the bias sums are formed by the same expression, the slabs and the reduce are
unchanged.  So every check is np.array_equal between the two routings, on float operands (Gaussians with ReLU-style
zeros: A a masked layer-output gradient, X a rectified layer input), and every case asserts that the thin kernel ran
in the one run and not in the other: sppDebugDwSet's thin flag for the direct cases, sppAgentDwThin for the agents.
(A workgroup of the kernel owns one sample part of an item, so "part 1 empty" below is a workgroup that runs no step
and stores an all-zero slab, and parts of unequal length are two workgroups with different trip counts.)

Direct cases (sppDebugDwSet, one job per call).  The planner gives a thin job items of 64 samples at Bp <= 256 and of
about Bp / 4 above (tests/dw_cases.unit_stats states the parts); with SPP_DW_THIN_MIN_BP=32 the batches reach
  B = 32      one item: part 0 one 32-sample step, part 1 empty
  B = 64      one item of 1 + 1 steps (no loop barrier beyond the first step's)
  B = 96, 160 items of 1 + 1 steps and a ragged last item of 1 + 0
  B = 512     items of 2 + 2 steps: both LDS buffers, no refill
  B = 704     items of 3 + 3 steps: the first refill; a last item of 2 + 2
  B = 2080    items of 9 + 9 steps, a last item of 6 + 5: parts of unequal length, each buffer refilled several times
and at the default threshold B = 8192 (32 + 32 steps) and 8224 (26 + 26 steps, a last item of 25 + 24).
Shapes: the wide side 256, 200 (a partial seventh block and a dead eighth) on either side, the narrow side 1 .. 23 rows
in one or two segments, and the head's two outputs (nrow2).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import dw_cases as dc  # noqa: E402
import test_gpu_dw_big8 as b8  # noqa: E402
import test_gpu_dw_direct as dd  # noqa: E402
from dw_cases import rup  # noqa: E402
from spprl import _lib  # noqa: E402

# (N, K0, K1, nrow2)
SHAPES = [(256, 11, 3, None), (256, 17, 6, None), (256, 11, 0, None), (200, 5, 0, None), (256, 1, 0, None),
          (22, 256, 0, 11), (17, 256, 0, None), (6, 256, 0, None), (1, 256, 0, None)]
# (SPP_DW_THIN_MIN_BP or None for the default, B, num_cu)
RUNS = ([(32, B, cu) for B in (32, 64, 96, 160, 2080) for cu in (1, 3)] + [(32, 512, 3), (32, 704, 3)] +
        [(None, 8192, 3), (None, 8224, 3)])
# parts (32-sample steps) of a full item and of the last item that the docstring states, checked against the plan
WANT_PARTS = {32: (1, [1, 0]), 64: (1, [1, 1]), 96: (1, [1, 0]), 160: (1, [1, 0]), 512: (2, [2, 2]), 704: (3, [2, 2]),
              2080: (9, [6, 5]), 8192: (32, [32, 32]), 8224: (26, [25, 24])}


def _fill_float(job, rng, B):
    Bp = rup(B, 32)
    A = rng.randn(job.N, Bp) * (rng.rand(job.N, Bp) < 0.5)
    A[:, B:] = 0
    X = np.maximum(rng.randn(job.K, Bp), 0)
    X[:, B:] = 0.25  # finite, not zero, in the dead columns
    job.A, job.X = A.astype(np.float32).astype(np.float64), X.astype(np.float32).astype(np.float64)


def _run_flagged(job, B, cu, monkeypatch):
    """dd.run of one job alone in its phase, and the thin flag that sppDebugDwSet left in its descriptor."""
    seen = []
    call = _lib.call

    def spy(name, descs, *a):
        r = call(name, descs, *a)
        seen.append(int(descs[0].thin))
        return r

    monkeypatch.setattr(_lib, "call", spy)
    try:
        (res,) = dd.run([job], B, cu)
    finally:
        monkeypatch.setattr(_lib, "call", call)
    assert len(seen) == 1
    return res, seen[0]


def _run(job, B, cu, thin, min_bp, monkeypatch):
    """(dW, db, plan, thin flag) of one job alone in its phase under SPP_DW_THIN = thin."""
    monkeypatch.setenv("SPP_DW_THIN", "1" if thin else "0")
    if min_bp is None:
        monkeypatch.delenv("SPP_DW_THIN_MIN_BP", raising=False)
    else:
        monkeypatch.setenv("SPP_DW_THIN_MIN_BP", str(min_bp))
    (dW, db, plan), seen = _run_flagged(job, B, cu, monkeypatch)
    assert seen == (1 if thin else 0), "SPP_DW_THIN=%d B %d: the thin flag is %s" % (thin, B, seen)
    return dW, db, plan


@pytest.mark.parametrize("db", [True, False], ids=["db", "nodb"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d+%d" % s[:3] for s in SHAPES])
def test_thin_equals_k_dw_bitwise(shape, db, monkeypatch):
    N, K0, K1, n2 = shape
    for min_bp, B, cu in RUNS:
        j = dd.Job(N, K0, K1, n2, db)
        _fill_float(j, np.random.RandomState(B + N + K0), B)
        rw, rb, rplan = _run(j, B, cu, 0, min_bp, monkeypatch)
        gw, gb, gplan = _run(j, B, cu, 1, min_bp, monkeypatch)
        tag = "%s db %d B %d num_cu %d plan %s" % (j.name(), db, B, cu, gplan)
        assert gplan == rplan and gplan[2] == 2, tag
        assert dc.unit_stats(gplan, rup(B, 32)) == WANT_PARTS[B], tag
        assert np.isfinite(rw).all() and np.abs(rw).max() > 0, tag
        assert np.array_equal(rw, gw), "dW %s: %d elements differ" % (tag, int(np.sum(rw != gw)))
        if db:
            assert np.abs(rb).max() > 0 and np.array_equal(rb, gb), "db %s: %d elements differ" % (
                tag, int(np.sum(rb != gb)))


@pytest.mark.parametrize("shape", [(256, 11, 3, None), (22, 256, 0, 11)], ids=["256x11+3", "22x256"])
def test_thin_exact_on_integers(shape, monkeypatch):
    """Integer operands against the float64 reference (every partial sum exact in fp32), B = 2080: parts of 9, 6, 5."""
    N, K0, K1, n2 = shape
    j = dd.Job(N, K0, K1, n2, True)
    dd.fill_int(j, np.random.RandomState(N), 2080)
    rw, rb, aw, ab = dd.reference(j, 2080)
    assert aw.max() < dd.LIMIT and ab.max() < dd.LIMIT
    gw, gb, _ = _run(j, 2080, 3, 1, 32, monkeypatch)
    np.testing.assert_array_equal(gw.astype(np.float64), rw)
    np.testing.assert_array_equal(gb.astype(np.float64), rb)


def test_below_the_threshold_stays_in_k_dw(monkeypatch):
    """Bp = 8160 at the default threshold: SPP_DW_THIN=1 leaves the job in k_dw."""
    j = dd.Job(256, 11, 3, None, True)
    _fill_float(j, np.random.RandomState(1), 8160)
    monkeypatch.setenv("SPP_DW_THIN", "1")
    monkeypatch.delenv("SPP_DW_THIN_MIN_BP", raising=False)
    assert _run_flagged(j, 8160, 3, monkeypatch)[1] == 0


# ------------------------------------------------------------------ agents
def _thin_of(ag):
    got = ctypes.c_int(-1)
    _lib.call("sppAgentDwThin", ag._h, ctypes.byref(got))
    return got.value


def _agent_states(name, sizes, thin, monkeypatch):
    monkeypatch.setenv("SPP_DW_THIN", "1" if thin else "0")  # read when the agent is made
    monkeypatch.delenv("SPP_DW_THIN_MIN_BP", raising=False)
    cls, env, _, _, kw = b8.SETS[name]
    ag = cls(env_name=env, max_batch=max(sizes), buffer_size=128, device=b8.bb.DEV, seed=3, **kw)
    states = []
    for B in sizes:
        b8._step(name, ag, b8._inputs(name, B))
        states.append(b8._state(ag))
        items = _thin_of(ag)
        assert (items > 0) == bool(thin and rup(B, 32) >= 8192), "SPP_DW_THIN=%d B %d: %d thin items" % (thin, B, items)
    return states


@pytest.mark.parametrize("name", ["sac_hopper", "ddpg_hcheetah"])
def test_agents_bitwise_over_shrinking_and_growing_batches(name, monkeypatch):
    sizes = [8192, 8256, 8192]
    ref = _agent_states(name, sizes, 0, monkeypatch)
    got = _agent_states(name, sizes, 1, monkeypatch)
    for i, (r, g) in enumerate(zip(ref, got)):
        for n in (_lib.SPP_NET_ACTOR, _lib.SPP_NET_CRITIC1):
            k = "grad %d" % n
            assert np.isfinite(r[k]).all() and np.abs(r[k]).max() > 0, k
        assert sorted(r) == sorted(g)
        for k in r:
            assert np.array_equal(r[k], g[k]), "update %d (B = %d) %s: %d elements differ" % (
                i, sizes[i], k, int(np.sum(r[k] != g[k])))


def test_small_batch_agent_reports_the_thin_kernel_off(monkeypatch):
    _agent_states("sac_hopper", [100], 1, monkeypatch)


def test_the_default_is_on(monkeypatch):
    """No SPP_DW_THIN in the environment: a B = 8,192 agent runs its thin items in k_dw_thin."""
    monkeypatch.delenv("SPP_DW_THIN", raising=False)
    monkeypatch.delenv("SPP_DW_THIN_MIN_BP", raising=False)
    cls, env, _, _, kw = b8.SETS["sac_hopper"]
    ag = cls(env_name=env, max_batch=8192, buffer_size=128, device=b8.bb.DEV, seed=3, **kw)
    b8._step("sac_hopper", ag, b8._inputs("sac_hopper", 8192))
    assert _thin_of(ag) > 0
