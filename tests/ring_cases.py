"""Collector schedules for the replay ring: what OffPolicyLoop._vector_step writes, step by step, as data.

One vector step of E lockstep envs is (spprl/trainer.py:_vector_step)
    nxt = add_obs_batch(next obs [E, ob])
    add_timestep_batch(prev, nxt, action, reward, done, end, acm action)
    prev = nxt;  prev[ended] = add_obs_batch(reset obs of the envs that ended)
so the obs ring advances by E + (number of ended envs) rows per step and leads the timestep ring, whose Q6 wrap
(replay_buffer.py:65-75: next_obs_idx < ts_idx) then fires in the middle of a batch whenever the E rows of a step
straddle the obs ring's end.

``schedule`` generates the payloads, ``Driver`` applies them to any ring with the two batched methods (the device
ring and oracle/replay.py's), ``census`` runs a schedule through the oracle alone and reports which of those edges
it reaches.  tests/test_ring_cases.py asserts the census for every case in CASES without a GPU;
tests/test_gpu_ring_vector.py then compares the device ring with the oracle on the same schedules.

Payloads are distinct by construction: field f of record k (k counts rows of that field in write order) has
column 0 = OFFSET[f] + (k + u) / 8192 with u uniform in [0, 1), the other columns OFFSET[f] + u.  The fields live
in the disjoint intervals [OFFSET[f], OFFSET[f] + 1), and column 0 differs between any two rows of a field, so a
row or a field that lands in another's place cannot compare equal."""
from collections import namedtuple

import numpy as np

from oracle.replay import OracleReplay

Case = namedtuple("Case", "cap E ob aout ac steps reset_rate seed")
Step = namedtuple("Step", "nobs act acm rew done end ended reset_rows")

OFFSET = {"nobs": 0.0, "reset": 2.0, "act": 4.0, "acm": 6.0, "rew": 8.0}

CASES = {
    "straddle97": Case(97, 8, 5, 5, 2, 48, 0.2, 1),      # cap no multiple of E: rows straddle the ring end mid-batch
    "blocks300": Case(1000, 300, 11, 11, 3, 14, 0.1, 2),  # E > 256: every section of k_replay_add_step crosses blocks
    "thin64": Case(257, 64, 1, 1, 1, 16, 0.1, 3),        # minimal widths, the head section starts at element 128
    "ant33": Case(600, 33, 111, 111, 8, 64, 0.1, 4),     # Ant record width
    "vanilla48": Case(400, 48, 17, 6, 6, 30, 0.1, 5),    # aout != ob (the vanilla ring's shape)
}
# straddle97 with acm_action=None from this step on: the timestep ring last wraps at step 40, so the 48 records of
# steps 42..47 overwrite records that held ACM actions, and the rest of the ring keeps non-zero ones
ACM_NONE_FROM = 42


def _rows(rng, field, k0, n, w):
    """n rows of width w of `field`, numbered k0, k0 + 1, ... (see the module docstring)."""
    assert k0 + n <= 8192
    x = rng.random_sample((n, w))
    x[:, 0] = (k0 + np.arange(n) + x[:, 0]) / 8192.0
    return (OFFSET[field] + x).astype(np.float32)


def schedule(cap, E, ob, aout, ac, steps, reset_rate, seed):
    """Generator: first the E reset observations [E, ob] every env starts from, then `steps` Step tuples --
    nobs [E, ob], act [E, aout], acm [E, ac], rew [E] (fp32), done / end [E] (uint8), ended (the env numbers with
    end set) and reset_rows [len(ended), ob], the observations those envs restart from.  end ~ Bernoulli(reset_rate)
    per env and step; done is set on half of the ends and, alone, on a further reset_rate / 4 of the rows."""
    rng = np.random.RandomState(seed)
    n_reset = E
    yield _rows(rng, "reset", 0, E, ob)
    for t in range(steps):
        k = t * E
        u = rng.random_sample(E)
        end = u < reset_rate
        done = (u < reset_rate / 2) | (u > 1.0 - reset_rate / 4)
        ended = np.flatnonzero(end)
        rew = _rows(rng, "rew", k, E, 1)[:, 0]
        st = Step(_rows(rng, "nobs", k, E, ob), _rows(rng, "act", k, E, aout), _rows(rng, "acm", k, E, ac), rew,
                  done.astype(np.uint8), end.astype(np.uint8), ended, _rows(rng, "reset", n_reset, len(ended), ob))
        n_reset += len(ended)
        yield st


class Driver:
    """Applies a schedule to a ring through add_obs(rows) -> slots and add_step(prev, nxt, act, rew, done, end, acm),
    keeping the collector's prev slots (patched after a partial reset, as _vector_step does)."""

    def __init__(self, add_obs, add_step, with_acm=True):
        self.add_obs, self.add_step, self.with_acm = add_obs, add_step, with_acm
        self.prev = None

    def start(self, rows):
        self.prev = np.array(self.add_obs(rows), np.int64)
        return self.prev

    def step(self, s):
        """-> (slots of the next observations, slots of the reset rows or None)"""
        nxt = np.array(self.add_obs(s.nobs), np.int64)
        self.add_step(self.prev, nxt, s.act, s.rew, s.done, s.end, s.acm if self.with_acm else None)
        self.prev = nxt.copy()
        rs = None
        if len(s.ended):
            rs = np.array(self.add_obs(s.reset_rows), np.int64)
            self.prev[s.ended] = rs
        return nxt, rs


def oracle_driver(orb, with_acm=True):
    return Driver(orb.add_obs_batch, orb.add_step_batch, with_acm)


def oracle_reset(orb):
    """MetaReplayBuffer.reset_idx (replay_buffer.py:32-35): the three cursors, nothing else."""
    orb.obs_idx = orb.ts_idx = orb.current_len = 0


def state(ring):
    return ring.obs_idx, ring.ts_idx, len(ring)


def record_heads(rb, n):
    """The first n record heads of a device ring as uint32 [n, 4] -- obs slot, next-obs slot, reward bits, flags
    (done in bit 0, end in bit 8: k_replay_add_step) -- read through the ring view (sppReplayGetView)."""
    import torch

    v = rb.view()
    rw = v.rec_words

    class _Records:  # the record array aliased as int32 [n * rw]
        __cuda_array_interface__ = {"shape": (n * rw,), "typestr": "<i4", "data": (v.rec, False), "version": 2}

    torch.cuda.synchronize()
    rec = torch.as_tensor(_Records(), device=rb.device).cpu().numpy().view(np.uint32)
    return rec.reshape(n, rw)[:, :4]


class _Watch(OracleReplay):
    """The oracle ring, logging per add_timestep (ts_idx before the call, whether the Q6 rule fired)."""

    def __init__(self, *a):
        super().__init__(*a)
        self.log = []

    def add_timestep(self, obs_idx, next_obs_idx, *rest):
        t = self.ts_idx
        assert t < self.size, "ts ring overflow: the obs ring must lead (reset_rate > 0)"
        super().add_timestep(obs_idx, next_obs_idx, *rest)
        self.log.append((t, next_obs_idx < t))


def census(case):
    """Runs `case` through the oracle and counts the edges it reaches.  Per step t: straddle[t] (the E next-obs
    rows lie on both sides of the obs ring's end), q6_env[t] (the env numbers at which the timestep ring wrapped),
    partial[t] (some but not all envs ended)."""
    cap, E = case.cap, case.E
    orb = _Watch(cap, case.ob, case.aout, case.ac)
    drv = oracle_driver(orb)
    it = schedule(*case)
    drv.start(next(it))
    rows, straddle, q6_env, partial, flags = E, [], [], [], set()
    for s in it:
        base = orb.obs_idx
        straddle.append(base + E > cap)
        n0 = len(orb.log)
        drv.step(s)
        ts = [t for t, _ in orb.log[n0:]]
        assert len(set(ts)) == E, "two envs of one step share a timestep slot: the write order would matter"
        q6_env.append([e for e, (_, fired) in enumerate(orb.log[n0:]) if fired])
        partial.append(0 < len(s.ended) < E)
        rows += E + len(s.ended)
        flags |= set(zip(s.done.tolist(), s.end.tolist()))
    q6_steps = [t for t, f in enumerate(q6_env) if f]
    mid = [t for t, f in enumerate(q6_env) if any(e > 0 for e in f)]
    return {
        "obs_wraps": rows // cap,
        "straddle_steps": [t for t, f in enumerate(straddle) if f],
        "q6_steps": q6_steps,
        "q6_midbatch_steps": mid,
        "partial_before_q6": [t for t in q6_steps if t > 0 and partial[t - 1]],
        "partial_before_straddle": [t for t, f in enumerate(straddle) if f and t > 0 and partial[t - 1]],
        "flags": flags,
        "state": state(orb),
    }
