"""sppReplayObsStats on its side stream (SPP_STATS_OVERLAP=1, csrc/api_replay.hip) against the same
calls on the caller's stream (SPP_STATS_OVERLAP=0) and against numpy on the same rows the way tests/test_gpu_stats.py
compares: percentiles bit-exact, mean / std within fp32 rounding of the fp64 result (rtol 2e-7), running max / min.
The two modes must agree bit for bit after every call, the outputs must change at the call's place in the caller's
stream (not before), the rows must be read before a later writer overwrites them, and every call the library
cannot prove independent must be counted as serial (sppReplayStatsOverlapCounts: a silent fallback cannot pass)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import spprl
from spprl import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@contextlib.contextmanager
def _mode(overlap):
    """SPP_STATS_OVERLAP is read when a replay handle is made."""
    old = os.environ.get("SPP_STATS_OVERLAP")
    os.environ["SPP_STATS_OVERLAP"] = str(overlap)
    try:
        yield
    finally:
        if old is None:
            del os.environ["SPP_STATS_OVERLAP"]
        else:
            os.environ["SPP_STATS_OVERLAP"] = old


def _buffer(overlap, size, ob, ac=3):
    with _mode(overlap):
        rb = spprl.BufferAcMOffPolicy(size, ob, ob, ac, device=DEV)
    assert _lib.load().sppReplayStatsOverlap(rb._h) == overlap
    rb._last = rb.add_obs_batch(torch.zeros(1, ob))[-1:]
    return rb


def _counts(rb):
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    _lib.call("sppReplayStatsOverlapCounts", rb._h, ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def _push(rb, rows):
    """rows [n, ob] as n transitions chained to the last observation written (in batches the ring can take)."""
    ob = rows.shape[1]
    step = min(8192, rb.size)
    for i in range(0, rows.shape[0], step):
        part = rows[i:i + step]
        E = part.shape[0]
        slots = rb.add_obs_batch(torch.from_numpy(part))
        prevs = np.concatenate([rb._last, slots[:-1]])
        z = np.zeros(E, bool)
        rb.add_timestep_batch(prevs, slots, torch.zeros(E, ob), np.zeros(E, np.float32), z, z, torch.zeros(E, 3))
        rb._last = slots[-1:]


def _live(rb):
    """The live rows obs[obs_idx[t]] (the bit-exact gather)."""
    return rb.gather(torch.arange(len(rb)))[0].cpu().numpy()


def _arrays(rb):
    return [t.cpu().numpy() for t in (rb.obs_mean, rb.obs_std, rb.max_obs, rb.min_obs)]


def _expect(got, x, prev=None):
    x = x.astype(np.float64)
    p99, p1 = np.percentile(x, 99, axis=0).astype(np.float32), np.percentile(x, 1, axis=0).astype(np.float32)
    if prev is not None:
        p99, p1 = np.maximum(p99, prev[2]), np.minimum(p1, prev[3])
    np.testing.assert_array_equal(got[2], p99)
    np.testing.assert_array_equal(got[3], p1)
    np.testing.assert_allclose(got[0], x.mean(0).astype(np.float32), rtol=2e-7, atol=1e-30)
    np.testing.assert_allclose(got[1], x.std(0).astype(np.float32), rtol=2e-7, atol=1e-30)


def _same(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def _rows(rng, n, ob, scale=1.0, shift=0.0):
    return (rng.standard_t(3, size=(n, ob)) * rng.uniform(0.1, 5, ob) * scale + rng.randn(ob) + shift).astype(
        np.float32)


# (live rows at the first calls, ring slots, transitions pushed first, transitions pushed over old rows)
SIZES = {11: (19, 11, 16), 1000: (1008, 1000, 500), 20000: (20000, 24000, 5000), 70000: (70008, 70000, 30000)}


@pytest.mark.parametrize("ob", [3, 11, 17, 111])
@pytest.mark.parametrize("live", [11, 1000, 20000, 70000])
def test_overlap_equals_serial_and_numpy(live, ob):
    size, first, more = SIZES[live]
    rng = np.random.RandomState(live % 991 + ob)
    a, b = _rows(rng, first, ob), _rows(rng, more, ob, 3.0, 2.0)
    pair = [_buffer(0, size, ob), _buffer(1, size, ob)]
    for rb in pair:
        _push(rb, a)
        assert len(rb) == live
    x = _live(pair[0])
    np.testing.assert_array_equal(x, _live(pair[1]))
    prev = None
    for call in range(4):
        if call == 3:  # rows that overwrite old ones (the obs ring wraps)
            for rb in pair:
                _push(rb, b)
            x = _live(pair[0])
            np.testing.assert_array_equal(x, _live(pair[1]))
        for rb in pair:
            rb.update_obs_mean_std()
        got = [_arrays(rb) for rb in pair]
        _same(got[0], got[1])
        _expect(got[1], x, prev)
        prev = got[1]
    assert _counts(pair[0]) == (0, 4)
    assert _counts(pair[1]) == (3, 1)  # the first call on a handle (first_update) is serial


def test_outputs_change_at_the_call_not_before():
    """A copy of the outputs queued BEFORE the call, behind a few ms of matmul the statistics kernels overlap,
    still holds the old values; a copy queued after the call holds the new ones."""
    rng = np.random.RandomState(3)
    ob = 11
    rb = _buffer(1, 40_000, ob)
    _push(rb, _rows(rng, 20_000, ob))
    rb.update_obs_mean_std()
    old = _arrays(rb)
    _push(rb, _rows(rng, 10_000, ob, 4.0, 7.0))
    x = _live(rb)
    m = torch.randn(4096, 4096, device=DEV)
    torch.cuda.synchronize()
    for _ in range(6):
        m = torch.mm(m, m) * 1e-3
    before = [t.clone() for t in (rb.obs_mean, rb.obs_std, rb.max_obs, rb.min_obs)]
    rb.update_obs_mean_std()
    after = [t.clone() for t in (rb.obs_mean, rb.obs_std, rb.max_obs, rb.min_obs)]
    torch.cuda.synchronize()
    assert _counts(rb) == (1, 1)
    _same([t.cpu().numpy() for t in before], old)
    new = [t.cpu().numpy() for t in after]
    _expect(new, x, old)
    assert not np.array_equal(new[0], old[0]) and not np.array_equal(new[2], old[2])
    _same(_arrays(rb), new)


def test_rows_are_read_before_a_later_writer_overwrites_them():
    rng = np.random.RandomState(4)
    ob, size = 17, 4096
    rb = _buffer(1, size, ob)
    _push(rb, _rows(rng, size + 100, ob))  # wrapped: every obs slot is live
    assert len(rb) == size
    rb.update_obs_mean_std()
    old = _arrays(rb)
    _push(rb, _rows(rng, 100, ob, 2.0))
    x = _live(rb)
    other = torch.from_numpy(_rows(rng, size, ob, 50.0, -300.0)).to(DEV)
    torch.cuda.synchronize()
    rb.update_obs_mean_std()
    rb.add_obs_batch(other)  # the same slots, other values, at once
    torch.cuda.synchronize()
    assert _counts(rb) == (1, 1)
    _expect(_arrays(rb), x, old)
    assert not np.array_equal(_live(rb), x)


def test_calls_the_library_cannot_prove_independent_are_serial():
    rng = np.random.RandomState(5)
    ob, n = 11, 5000
    pair = [_buffer(0, 3 * n, ob), _buffer(1, 3 * n, ob)]
    rows = _rows(rng, n, ob)
    for rb in pair:
        _push(rb, rows)
        rb.update_obs_mean_std()
        rb.update_obs_mean_std()
    assert _counts(pair[1]) == (1, 1)
    _same(_arrays(pair[0]), _arrays(pair[1]))

    def step(change, want):
        more = _rows(rng, 500, ob, 2.0, 1.0)
        for rb in pair:
            _push(rb, more)
            change(rb)
            rb.update_obs_mean_std()
        assert _counts(pair[1]) == want
        got = [_arrays(rb) for rb in pair]
        _same(got[0], got[1])
        return got[1]

    prev = _arrays(pair[1])
    got = step(lambda rb: rb.view(), (1, 2))  # the caller may write the rows through the view
    _expect(got, _live(pair[1]), prev)
    prev = got
    got = step(lambda rb: None, (2, 2))  # rows written through the library again: the side stream
    _expect(got, _live(pair[1]), prev)
    prev = got
    got = step(lambda rb: _lib.call("sppReplayObsStatsInvalidate", rb._h), (2, 3))
    _expect(got, _live(pair[1]), prev)
    prev = got

    def other_tensors(rb):
        rb.obs_mean, rb.obs_std = rb.obs_mean.clone(), rb.obs_std.clone()
        rb.max_obs, rb.min_obs = rb.max_obs.clone(), rb.min_obs.clone()

    got = step(other_tensors, (2, 4))
    _expect(got, _live(pair[1]), prev)
    prev = got
    got = step(lambda rb: None, (3, 4))
    _expect(got, _live(pair[1]), prev)


def test_two_caller_streams_in_turn():
    rng = np.random.RandomState(6)
    ob, n = 11, 30_000
    pair = [_buffer(0, 3 * n, ob), _buffer(1, 3 * n, ob)]
    first, more, last = _rows(rng, n, ob), _rows(rng, n // 2, ob, 3.0, 5.0), _rows(rng, n // 2, ob, 6.0, -9.0)
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    ref = []
    for rb in pair:
        _push(rb, first)
        rb.update_obs_mean_std()
        s1.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s1):
            rb.update_obs_mean_std()
        s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            _push(rb, more)
            rb.update_obs_mean_std()
        s1.wait_stream(s2)
        with torch.cuda.stream(s1):
            rb.update_obs_mean_std()
            _push(rb, last)
        s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            rb.update_obs_mean_std()
        torch.cuda.synchronize()
        ref.append(_arrays(rb))
    assert _counts(pair[0]) == (0, 5)
    assert _counts(pair[1]) == (4, 1)
    _same(ref[0], ref[1])
    x = _live(pair[1]).astype(np.float64)
    # (the running extremes of the earlier calls only widen the percentiles of the last rows)
    assert np.all(ref[1][2] >= np.percentile(x, 99, axis=0).astype(np.float32))
    assert np.all(ref[1][3] <= np.percentile(x, 1, axis=0).astype(np.float32))
    np.testing.assert_allclose(ref[1][0], x.mean(0).astype(np.float32), rtol=2e-7, atol=1e-30)
    np.testing.assert_allclose(ref[1][1], x.std(0).astype(np.float32), rtol=2e-7, atol=1e-30)


AGENT = dict(gamma=0.99, actor_lr=1e-3, critic_lr=1e-3, alpha_lr=1e-3, alpha=0.2, acm_lr=1e-3, acm_critic=True,
             custom_loss=0.2, norm_closs=False, min_max_denormalize=True, denormalize_actor_out=True,
             update_batch_size=100, update_freq=50, grad_steps=50, acm_update_freq=1000, acm_update_batches=100,
             acm_batch_size=100)


def _agent_run(overlap, calls_per_step):
    E, cap, ob, ac = 64, 4096, 11, 3
    with _mode(overlap):
        ag = spprl.SAC_AcM(env_name="Hopper-v2", buffer_size=cap, max_batch=100 * E, device=DEV, seed=0, n_envs=E,
                           schedule="fused", random_frames=0, batch_size=1000, iterations=10 ** 9, loop_seed=1000,
                           acm_epochs=1, **AGENT)
    rb = ag.replay_buffer
    assert _lib.load().sppReplayStatsOverlap(rb._h) == overlap
    g = torch.Generator(device="cpu").manual_seed(7)
    fill = cap - 2 * E
    prev = rb.add_obs_batch(torch.randn(1, ob, generator=g))
    slots = rb.add_obs_batch(torch.randn(fill, ob, generator=g))
    z = torch.zeros(fill, dtype=torch.uint8)
    rb.add_timestep_batch(np.concatenate([prev[-1:], slots[:-1]]), slots, torch.randn(fill, ob, generator=g),
                          torch.randn(fill, generator=g), z, z, torch.rand(fill, ac, generator=g) * 2 - 1)
    ag.update_obs_stats()
    ag.iteration = 1
    ag.stats_logger.frames = fill
    for _ in range(6):
        ag.collect_batch_and_train(E)
        for _ in range(calls_per_step):
            ag.update_obs_stats()
    torch.cuda.synchronize()
    out = {"param_%s" % k: v.detach().cpu().numpy().copy() for k, v in ag.params.items()}
    out.update(zip(("mean", "std", "max", "min"), _arrays(rb)))
    return out, _counts(rb)


@pytest.mark.parametrize("calls_per_step", [1, 4])
def test_agent_steps_equal_in_both_modes(calls_per_step):
    serial, cs = _agent_run(0, calls_per_step)
    side, co = _agent_run(1, calls_per_step)
    assert cs == (0, 1 + 6 * calls_per_step)
    assert co == (6 * calls_per_step, 1)
    assert sorted(serial) == sorted(side)
    for k in serial:
        np.testing.assert_array_equal(serial[k], side[k], err_msg=k)
