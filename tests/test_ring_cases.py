"""CPU: the collector schedules of tests/ring_cases.py reach the edges the GPU ring tests rely on.

Each case runs through the oracle ring alone (oracle/replay.py, add_obs_batch / add_step_batch: the reference's
single-step methods in env order).  The census below is the precondition of tests/test_gpu_ring_vector.py: a
schedule that never straddles the obs ring's end, or never wraps the timestep ring in mid-batch, would compare the
device ring with the oracle only where nothing can go wrong."""
import numpy as np
import pytest

import ring_cases as rc
from oracle.replay import OracleReplay


@pytest.mark.parametrize("name", list(rc.CASES))
def test_schedule_census(name):
    case = rc.CASES[name]
    assert case.reset_rate > 0 and case.E <= case.cap
    z = rc.census(case)  # (asserts on the way: no ts ring overflow, distinct timestep slots within a step)
    assert z["obs_wraps"] >= 3
    assert z["straddle_steps"], "no vector step with rows on both sides of the obs ring's end"
    assert z["q6_midbatch_steps"], "the Q6 rule never fired past env 0"
    assert z["q6_midbatch_steps"][0] >= 1, "no checkpoint before the first wrap"
    assert z["partial_before_q6"] and z["partial_before_straddle"], "no partial reset in the step before a wrap"
    assert z["flags"] == {(0, 0), (0, 1), (1, 0), (1, 1)}  # (done, end): each alone, both, neither
    assert z["state"][2] <= case.cap


def test_case_table():
    shapes = {(c.cap, c.E, c.ob, c.aout, c.ac) for c in rc.CASES.values()}
    assert shapes == {(97, 8, 5, 5, 2), (1000, 300, 11, 11, 3), (257, 64, 1, 1, 1), (600, 33, 111, 111, 8),
                      (400, 48, 17, 6, 6)}
    assert rc.CASES["straddle97"].steps >= 12  # the back-to-back test: three times the 4-deep metadata ring


@pytest.mark.parametrize("name", ["straddle97", "thin64"])
def test_payloads_are_distinct_and_deterministic(name):
    case = rc.CASES[name]
    a, b = list(rc.schedule(*case)), list(rc.schedule(*case))
    for x, y in zip(a[1:], b[1:]):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)
    steps = a[1:]
    fields = {"nobs": np.concatenate([s.nobs for s in steps]), "act": np.concatenate([s.act for s in steps]),
              "acm": np.concatenate([s.acm for s in steps]), "rew": np.concatenate([s.rew for s in steps])[:, None],
              "reset": np.concatenate([a[0]] + [s.reset_rows for s in steps])}
    for f, x in fields.items():
        assert x.dtype == np.float32
        assert len(np.unique(x[:, 0])) == len(x), f  # no two rows of a field agree in column 0
        assert rc.OFFSET[f] <= x.min() and x.max() < rc.OFFSET[f] + 1, f  # fields in disjoint intervals


def test_oracle_vector_driver_is_the_single_step_loop():
    """add_obs_batch / add_step_batch against the single-step calls written out (all E add_obs, then per env
    add_acm_action + add_timestep); acm=None stores zeros over what the records held."""
    case = rc.CASES["straddle97"]
    a = OracleReplay(case.cap, case.ob, case.aout, case.ac)
    b = OracleReplay(case.cap, case.ob, case.aout, case.ac)
    drv = rc.oracle_driver(a)
    it = rc.schedule(*case)
    rows = next(it)
    drv.start(rows)
    prev = np.array([b.add_obs(r) for r in rows])
    for t, s in enumerate(it):
        drv.with_acm = t < rc.ACM_NONE_FROM  # the last steps overwrite earlier records' ACM actions with zeros
        nxt, rs = drv.step(s)
        slots = np.array([b.add_obs(r) for r in s.nobs])
        np.testing.assert_array_equal(slots, nxt)
        for e in range(case.E):
            b.add_acm_action(s.acm[e] if t < rc.ACM_NONE_FROM else np.zeros(case.ac, np.float32))
            b.add_timestep(prev[e], slots[e], s.act[e], s.rew[e], s.done[e], s.end[e])
        prev = slots
        for e, r in zip(s.ended, s.reset_rows):
            prev[e] = b.add_obs(r)
        np.testing.assert_array_equal(prev, drv.prev)
        assert rc.state(a) == rc.state(b)
    idx = np.arange(len(a))
    for x, y in zip(a.gather(idx), b.gather(idx)):
        np.testing.assert_array_equal(x, y)
    assert (a._end == b._end).all()
    assert (a.gather(idx)[5] == 0).all(1).any() and (a.gather(idx)[5] != 0).all(1).any()
