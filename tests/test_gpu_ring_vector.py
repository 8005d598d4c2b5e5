"""GPU: the device replay ring under the vectorised collector's writes, against the oracle ring.

add_obs_batch / add_timestep_batch (sppReplayAddObs, sppReplayAddStep, k_replay_add_obs, k_replay_add_step) and
oracle/replay.py's OracleReplay run the same schedules (tests/ring_cases.py; tests/test_ring_cases.py asserts on
the CPU that every schedule straddles the obs ring's end, wraps the timestep ring in mid-batch (Q6), resets part
of the envs right before a wrap, and carries done and end alone and together).  The payloads are distinct per
(step, env, field), so a record that received another env's action, ACM action, reward or flags cannot compare
equal.  Everything is compared bit for bit: the ring stores what it is given and the gathers copy it.
"""
import numpy as np
import pytest
import torch

import ring_cases as rc
import spprl
from oracle.replay import OracleReplay
from spprl import _lib
from spprl._lib import SppError

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIELDS = ("obs", "next_obs", "action", "reward", "done", "acm_action")


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _rings(case, vanilla=False, n_envs=None):
    if vanilla:
        rb = spprl.ReplayBuffer(case.cap, case.ob, case.aout, device=DEV, n_envs=n_envs or case.E)
        orb = OracleReplay(case.cap, case.ob, case.aout, case.aout)
    else:
        rb = spprl.BufferAcMOffPolicy(case.cap, case.ob, case.aout, case.ac, device=DEV, n_envs=n_envs or case.E)
        orb = OracleReplay(case.cap, case.ob, case.aout, case.ac)
    return rb, orb


def _drivers(rb, orb, with_acm=True):
    return rc.Driver(rb.add_obs_batch, rb.add_timestep_batch, with_acm), rc.oracle_driver(orb, with_acm)


def _assert_rings_equal(rb, orb, tag=""):
    """State, then every live record's six fields (five for the vanilla ring) through rb.gather."""
    assert rc.state(rb) == rc.state(orb), tag
    n = len(orb)
    got = rb.gather(torch.arange(n))
    torch.cuda.synchronize()
    for name, g, w in zip(FIELDS, got, orb.gather(np.arange(n))):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg="%s %s" % (tag, name))


def _assert_gather_acm_equal(rb, orb, seed):
    n, ob, ac = len(orb), orb.ob, orb.ac
    rng = np.random.RandomState(seed)
    for B in (1, 63, 65, 257):  # either side of the 64-sample tile, several tiles with a ragged last one
        idx = rng.randint(0, n, B)
        x = torch.empty(B, 2 * ob, device=DEV)
        y = torch.empty(B, ac, device=DEV)
        _lib.call("sppReplayGatherAcm", rb._h, _lib.ptr(torch.from_numpy(idx).to(DEV)), B, _lib.ptr(x), _lib.ptr(y),
                  _lib.stream_handle())
        torch.cuda.synchronize()
        o, no, _, _, _, acm = orb.gather(idx)
        np.testing.assert_array_equal(_bits(x), _bits(np.concatenate([o, no], 1)), err_msg="B=%d" % B)
        np.testing.assert_array_equal(_bits(y), _bits(acm), err_msg="B=%d" % B)


def _lockstep(rb, orb, items, with_acm=True, checkpoints=()):
    """Both rings through the schedule `items`: slots and state equal after every step, the full gather equal after
    the steps in `checkpoints`."""
    dev, ora = _drivers(rb, orb, with_acm)
    np.testing.assert_array_equal(dev.start(items[0]), ora.start(items[0]))
    for t, s in enumerate(items[1:]):
        for got, want in zip(dev.step(s), ora.step(s)):
            np.testing.assert_array_equal(got, want, err_msg="slots, step %d" % t)
        assert rc.state(rb) == rc.state(orb), "step %d" % t
        if t in checkpoints:
            _assert_rings_equal(rb, orb, "after step %d" % t)
    return dev, ora


def _items(case, **change):
    """The schedule as a list: the start rows, then the Step tuples (read by both rings, never written)."""
    return list(rc.schedule(*case._replace(**change)))


@pytest.mark.parametrize("name", list(rc.CASES))
def test_vector_writes_match_oracle(name):
    """Slots and (obs_idx, ts_idx, len) after every step; all six fields of every live record before the first
    wrap, right after the first mid-batch Q6 wrap and at the end; then the ACM gather at four batch sizes."""
    case = rc.CASES[name]
    z = rc.census(case)
    first_mid = z["q6_midbatch_steps"][0]
    before_wrap = min(z["q6_steps"][0], z["straddle_steps"][0]) - 1
    assert before_wrap >= 0
    rb, orb = _rings(case)
    _lockstep(rb, orb, _items(case), checkpoints=(before_wrap, first_mid))
    assert rc.state(orb) == z["state"]
    _assert_rings_equal(rb, orb, "end")
    _assert_gather_acm_equal(rb, orb, seed=case.seed)


def _to_device(items):
    """The schedule's payloads as device tensors (ended stays on the host): the writes then need no upload."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    out = [t(items[0])]
    for s in items[1:]:
        out.append(s._replace(nobs=t(s.nobs), act=t(s.act), acm=t(s.acm), rew=t(s.rew), done=t(s.done), end=t(s.end),
                              reset_rows=t(s.reset_rows)))
    torch.cuda.synchronize()
    return out


def test_back_to_back_steps_without_synchronisation():
    """48 vector steps enqueued back to back from device-resident payloads (twelve times the 4-deep pinned metadata
    ring): nothing waits for the device between the steps, the comparison comes only at the end."""
    case = rc.CASES["straddle97"]
    assert case.steps >= 12
    items = _items(case)
    rb, orb = _rings(case)
    dev, ora = _drivers(rb, orb)
    ditems = _to_device(items)
    dev.start(ditems[0])
    for s in ditems[1:]:
        dev.step(s)
    ora.start(items[0])
    for s in items[1:]:
        ora.step(s)
    np.testing.assert_array_equal(dev.prev, ora.prev)
    _assert_rings_equal(rb, orb)


def test_metadata_ring_grows_between_unsynchronised_writes():
    """A ring built for one env takes five E = 1 steps and then, with those still in flight, E = 300 steps: the
    pinned metadata ring is reallocated (ring_reserve) under the queued uploads of the earlier steps."""
    small = rc.Case(1000, 1, 11, 11, 3, 5, 0.4, 11)
    big = rc.Case(1000, 300, 11, 11, 3, 2, 0.1, 12)
    rb, orb = _rings(small, n_envs=1)
    dev, ora = _drivers(rb, orb)
    parts = [list(rc.schedule(*small)), list(rc.schedule(*big))]
    dparts = [_to_device(p) for p in parts]
    for p in dparts:
        dev.start(p[0])
        for s in p[1:]:
            dev.step(s)
    for p in parts:
        ora.start(p[0])
        for s in p[1:]:
            ora.step(s)
    np.testing.assert_array_equal(dev.prev, ora.prev)
    _assert_rings_equal(rb, orb)
    _assert_gather_acm_equal(rb, orb, seed=3)


def test_acm_action_none_overwrites_with_zeros_after_a_wrap():
    """Steps without an ACM action after the timestep ring has wrapped: the records they overwrite held non-zero
    ACM actions and must read zeros; the records they leave alone keep theirs."""
    case = rc.CASES["straddle97"]
    k = rc.ACM_NONE_FROM
    assert rc.census(case)["q6_steps"][-1] < k
    items = _items(case)
    rb, orb = _rings(case)
    dev, ora = _drivers(rb, orb)
    dev.start(items[0]), ora.start(items[0])
    for s in items[1:1 + k]:
        dev.step(s), ora.step(s)
    n = len(orb)
    before = rb.gather(torch.arange(n))[5].cpu().numpy()
    assert (before != 0).all()
    dev.with_acm = ora.with_acm = False
    for s in items[1 + k:]:
        dev.step(s), ora.step(s)
    assert len(orb) == n
    _assert_rings_equal(rb, orb)
    after = rb.gather(torch.arange(n))[5].cpu().numpy()
    zero = (after == 0).all(1)
    assert zero.sum() == (case.steps - k) * case.E  # exactly the records of the steps without an ACM action
    np.testing.assert_array_equal(after[~zero], before[~zero])


def test_vanilla_replay_buffer_sample_batch():
    """spprl.ReplayBuffer (no ACM action) through the 17 / 6 / 6 schedule; sample_batch's five fields on the
    indices numpy's global stream draws (replay_buffer.py:234)."""
    case = rc.CASES["vanilla48"]
    rb, orb = _rings(case, vanilla=True)
    _lockstep(rb, orb, _items(case), with_acm=False)
    _assert_rings_equal(rb, orb)
    B = 257
    np.random.seed(77)
    got = rb.sample_batch(B)
    torch.cuda.synchronize()
    np.random.seed(77)
    idx = np.random.randint(0, len(orb), B)
    assert len(got) == 5
    for name, g, w in zip(FIELDS, got, orb.gather(idx)):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=name)


def test_refused_writes_leave_no_trace():
    """An add_timestep_batch whose LAST env has an out-of-range slot and an add_obs_batch of more rows than the
    ring holds are refused by host argument checks (no launch).  The ring's state must be what it was, the next
    valid step must land where the oracle (which never saw the refused calls) puts it, and the records must match."""
    case = rc.CASES["straddle97"]
    z = rc.census(case)
    items = _items(case)
    rb, orb = _rings(case)
    dev, ora = _drivers(rb, orb)
    dev.start(items[0]), ora.start(items[0])
    # refuse once in the open ring and once in the step whose batch wraps the timestep ring
    for t, s in enumerate(items[1:]):
        if t in (3, z["q6_midbatch_steps"][1]):
            st = rc.state(rb)
            nxt_bad = (dev.prev + 1) % case.cap
            for bad in (case.cap, -1):
                nxt_bad[-1] = bad
                with pytest.raises(SppError, match="slot out of range"):
                    rb.add_timestep_batch(dev.prev, nxt_bad, s.act, s.rew, s.done, s.end, s.acm)
                assert rc.state(rb) == st
            prev_bad = dev.prev.copy()
            prev_bad[-1] = case.cap
            with pytest.raises(SppError, match="slot out of range"):
                rb.add_timestep_batch(prev_bad, (dev.prev + 1) % case.cap, s.act, s.rew, s.done, s.end, s.acm)
            assert rc.state(rb) == st
            with pytest.raises(SppError):
                rb.add_obs_batch(np.zeros((case.cap + 1, case.ob), np.float32))
            assert rc.state(rb) == st
        for got, want in zip(dev.step(s), ora.step(s)):
            np.testing.assert_array_equal(got, want, err_msg="slots, step %d" % t)
        assert rc.state(rb) == rc.state(orb), "step %d" % t
    _assert_rings_equal(rb, orb)


def test_q6_rule_at_its_boundary():
    """add_timestep's wrap rule is next_obs_idx < ts_idx, strictly (replay_buffer.py:65-75).  The collector never
    presents next == ts_idx (its obs ring leads), so the boundary is driven by hand: next == ts_idx must not wrap,
    next == ts_idx - 1 must, both in the middle of a batch."""
    cap, ob, aout, ac = 50, 3, 2, 1
    rb = spprl.BufferAcMOffPolicy(cap, ob, aout, ac, device=DEV, n_envs=4)
    orb = OracleReplay(cap, ob, aout, ac)
    rng = np.random.RandomState(0)
    rows = rng.rand(20, ob).astype(np.float32)
    np.testing.assert_array_equal(rb.add_obs_batch(rows), orb.add_obs_batch(rows))
    # (prev, next) per batch; ts_idx runs 0 1 2 3 | 4 5 -> 0 1 | 2 3 -> 0 1
    batches = [([0, 1, 2, 3], [4, 5, 6, 7]),   # next > ts_idx throughout
               ([4, 5, 6, 7], [4, 4, 0, 9]),   # 4 == 4: no wrap; 4 < 5: wrap; 0 == 0: no wrap
               ([8, 9, 10, 11], [2, 2, 0, 1])]  # 2 == 2: no wrap; 2 < 3: wrap; 0 == 0, 1 == 1: no wrap
    want_state = [(20, 4, 4), (20, 2, 6), (20, 2, 4)]  # (a wrap sets len = ts_idx + 1, even downwards)
    for (prev, nxt), want in zip(batches, want_state):
        pay = (rng.rand(4, aout).astype(np.float32) + 4, rng.rand(4).astype(np.float32) + 8,
               rng.rand(4) < 0.5, rng.rand(4) < 0.5, rng.rand(4, ac).astype(np.float32) + 6)
        rb.add_timestep_batch(np.array(prev), np.array(nxt), *pay)
        orb.add_step_batch(prev, nxt, *pay)
        assert rc.state(orb) == want
        assert rc.state(rb) == want
    _assert_rings_equal(rb, orb)


def test_reset_idx_then_a_fresh_schedule():
    """reset_idx (replay_buffer.py:32-35) rewinds the three cursors and keeps the storage; a second schedule on top
    of the first one's leftovers must match an oracle reset the same way."""
    case = rc.CASES["thin64"]
    rb, orb = _rings(case)
    _lockstep(rb, orb, _items(case))
    rb.reset_idx()
    rc.oracle_reset(orb)
    assert rc.state(rb) == (0, 0, 0)
    z = rc.census(case._replace(seed=case.seed + 100))
    _lockstep(rb, orb, _items(case, seed=case.seed + 100), checkpoints=(0, z["q6_midbatch_steps"][0]))
    _assert_rings_equal(rb, orb, "end")
    _assert_gather_acm_equal(rb, orb, seed=9)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_record_heads_match_oracle(name):
    """The record heads as the ring holds them, read through the ring view: obs slot, next-obs slot, reward bits,
    done (bit 0) and end (bit 8).  rb.gather returns no end flag, so env e's end byte is checked here."""
    case = rc.CASES[name]
    rb, orb = _rings(case)
    _lockstep(rb, orb, _items(case))
    n = len(orb)
    h = rc.record_heads(rb, n)
    np.testing.assert_array_equal(h[:, 0], orb._obs_idx[:n])
    np.testing.assert_array_equal(h[:, 1], orb._next_obs_idx[:n])
    np.testing.assert_array_equal(h[:, 2], orb._rewards[:n].view(np.uint32))
    np.testing.assert_array_equal(h[:, 3] & 1, orb._done[:n])
    np.testing.assert_array_equal(h[:, 3] >> 8, orb._end[:n])
    assert orb._end[:n].any() and (orb._end[:n] != orb._done[:n]).any()
