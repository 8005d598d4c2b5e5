"""The CPU references of the optimizer tests (oracle/adam.py), checked against each other.

tests/test_gpu_optim.py holds the device Adam to (a) bit equality with adam_steps_f32 and (b) a float64 bound
of 4 x the normalised error of adam_steps_f32 against adam_steps_f64.  These tests keep those two
restatements honest without a GPU:
  - adam_steps_f64 is OracleAdam (the restated torch.optim.Adam every other oracle steps with) run on float64
    tensors, from a resumed state too: normalised error <= 1e-14 (the same dozen float64 operations of 1.1e-16
    each, in another association inside lerp_ / addcdiv_; normalised, since m cancels where g ~ -9 m);
  - adam_steps_f32 stays within 1e-6 (normalised, scales of oracle.adam.adam_scales) of adam_steps_f64 over
    8 steps of n = 1e5 elements with gradient magnitudes log-uniform in [1e-6, 1e2], resumed at steps 0, 1, 9,
    999 and 1e5, with and without the polyak target.  Measured when written: p 5.7e-7, m 1.2e-7, v 5.1e-7,
    target 6.5e-7 at most (a float32 rounding is 6e-8; v takes two roundings per step of a sum that decays by
    0.999, p one of a term lr-sized against a scale of at least 8 lr);
  - an OracleAdam resumed from (m, v, t) continues bit for bit like the one it was copied from.
"""
import numpy as np
import pytest
import torch

import optim_cases as oc
from oracle.adam import (OracleAdam, adam_scales, adam_steps_f32, adam_steps_f64, designed_gradient,
                         designed_state)

LR, TAU = 1e-3, 0.005


def _case(seed, n, K, huge=0):
    rng = np.random.RandomState(seed)
    p0, m0, v0 = designed_state(rng, n)
    tg0 = rng.uniform(-1, 1, n).astype(np.float32)
    grads = [designed_gradient(rng, n, huge=huge) for _ in range(K)]
    return p0, m0, v0, tg0, grads


def normalised_errors(p0, m0, v0, t0, grads, lr, tg0=None, tau=None):
    """Largest normalised error of the float32 restatement against float64: (p, m, v, target)."""
    r64 = adam_steps_f64(p0, m0, v0, t0, grads, lr, tg0, tau)
    r32 = adam_steps_f32(p0, m0, v0, t0, grads, lr, tg0, tau)
    s_p, s_m, s_v = adam_scales(p0, m0, grads, lr, r64[2])
    e = [float(np.max(np.abs(r32[i].astype(np.float64) - r64[i]) / s)) for i, s in enumerate((s_p, s_m, s_v))]
    if tg0 is not None:
        s_t = np.maximum(np.abs(np.asarray(tg0, np.float64)), s_p)
        e.append(float(np.max(np.abs(r32[3].astype(np.float64) - r64[3]) / s_t)))
    return e


@pytest.mark.parametrize("t0", [0, 1, 9, 999, 100000])
def test_f32_restatement_within_1e6_of_float64(t0):
    p0, m0, v0, tg0, grads = _case(100 + t0 % 97, 100000, 8)
    e = normalised_errors(p0, m0, v0, t0, grads, LR, tg0, TAU)
    print("t0 %d: normalised error of the fp32 restatement: p %.2e m %.2e v %.2e target %.2e" % (t0, *e))
    assert max(e) <= 1e-6, e


def test_f32_restatement_with_huge_and_zero_gradients_is_finite_and_exact_where_nothing_moves():
    """+-1e18 entries stay finite (g^2 = 1e36 < 3.4e38); where g = m0 = v0 = 0 the step leaves p bit-unchanged
    and the moments exact zeros; the normalised bound holds there too."""
    n = 4096
    p0, m0, v0, tg0, grads = _case(7, n, 3, huge=4)
    assert sum(int(np.sum(np.abs(g) == np.float32(1e18))) for g in grads) == 12
    p, m, v, tg, t = adam_steps_f32(p0, m0, v0, 9, grads, LR, tg0, TAU)
    assert t == 12 and all(np.isfinite(x).all() for x in (p, m, v, tg))
    z = slice(n // 8, n // 4)
    assert (p[z].view(np.int32) == p0[z].view(np.int32)).all() and not m[z].any() and not v[z].any()
    assert (p[:n // 8] != p0[:n // 8]).all()  # zero gradient over live moments still moves p
    assert max(normalised_errors(p0, m0, v0, 9, grads, LR, tg0, TAU)) <= 1e-6


@pytest.mark.parametrize("t0", [0, 9, 100000])
def test_f64_restatement_is_oracle_adam(t0):
    p0, m0, v0, _, grads = _case(3 + t0 % 89, 5000, 4)
    lrs = [LR, LR, 2.5e-4, 2.5e-4]
    p, m, v, _, t = adam_steps_f64(p0, m0, v0, t0, grads, lrs)
    tp = torch.from_numpy(p0.astype(np.float64))
    o = OracleAdam([tp], LR, m=[m0], v=[v0], t=t0)
    assert o.m[0].dtype == torch.float64
    for g, a in zip(grads, lrs):
        o.lr = float(np.float32(a))
        o.step([torch.from_numpy(g.astype(np.float64))])
    assert o.t == t == t0 + 4
    s_p, s_m, s_v = adam_scales(p0, m0, grads, lrs, v)
    for got, want, s in ((tp.numpy(), p, s_p), (o.m[0].numpy(), m, s_m), (o.v[0].numpy(), v, s_v)):
        assert np.max(np.abs(got - want) / s) <= 1e-14


def test_oracle_adam_resumes_bit_for_bit():
    rng = np.random.RandomState(5)
    shapes = [(7, 3), (5,)]
    grads = [[torch.from_numpy(rng.randn(*s).astype(np.float32)) for s in shapes] for _ in range(5)]
    pa = [torch.from_numpy(rng.randn(*s).astype(np.float32)) for s in shapes]
    a = OracleAdam(pa, LR)
    for g in grads[:3]:
        a.step(g)
    pb = [p.clone() for p in pa]
    b = OracleAdam(pb, LR, m=[x.numpy().copy() for x in a.m], v=[x.reshape(-1).clone() for x in a.v], t=a.t)
    for g in grads[3:]:
        a.step(g)
        b.step(g)
    assert a.t == b.t == 5
    for x, y in zip(pa + a.m + a.v, pb + b.m + b.v):
        assert torch.equal(x, y)
    # the resumed copy owns its moments
    assert b.m[0].data_ptr() != a.m[0].data_ptr()


def test_acm_trainer_oracle_dtype_and_resume():
    """OracleAcmTrainer(dtype=float64) follows the float32 one to float32 rounding, and resumes from moments."""
    from oracle import nets as onets
    from oracle.acm import OracleAcmTrainer
    from weights import fill_params

    params = fill_params(onets.acm_layout(22, 3), 4)
    rng = np.random.RandomState(1)
    xs = [(rng.randn(40, 22)).astype(np.float32) for _ in range(4)]
    ys = [rng.uniform(-1, 1, (40, 3)).astype(np.float32) for _ in range(4)]
    o32 = OracleAcmTrainer(22, 3, lr=LR, params=params)
    o64 = OracleAcmTrainer(22, 3, lr=LR, params=params, dtype=torch.float64)
    for x, y in zip(xs[:2], ys[:2]):
        l32, l64 = o32.batch_update(x, y), o64.batch_update(x, y)
        assert l32 == pytest.approx(l64, rel=1e-5)
    assert o64.flat().dtype == np.float64 and o64.last_grad.dtype == np.float64
    m, v = o64.moments()
    np.testing.assert_allclose(o32.moments()[0], m, rtol=0, atol=1e-5 * np.abs(m).max())
    state = {n: t.detach().numpy().copy() for n, t in o64.p.items()}
    r = OracleAcmTrainer(22, 3, lr=LR, params=state, dtype=torch.float64, m=m.copy(), v=v.copy(), t=o64.opt.t)
    for x, y in zip(xs[2:], ys[2:]):
        assert r.batch_update(x, y) == o64.batch_update(x, y)
    assert r.opt.t == 4 and np.array_equal(r.flat(), o64.flat())
    assert all(np.array_equal(a, b) for a, b in zip(r.moments(), o64.moments()))


@pytest.mark.parametrize("name", list(oc.CASES))
def test_persistent_case_tolerance_inputs_still_hold(name):
    """tests/test_gpu_optim.py holds every moment of a persistent-kernel case to tau x rms(its layer), tau =
    max(2e-4, optim_cases.TAU_F32[name]), the latter recorded as 8 x the deviation of the float32 oracle from the
    float64 oracle.  Re-measured here (summation order may move it a little: 1.5 x the record allowed); the
    probes' oracle gradient is exactly zero (asserted inside run_oracle)."""
    case = oc.make_case(name)
    r64, r32 = oc.run_oracle(case, torch.float64), oc.run_oracle(case, torch.float32)
    dev = max(oc.layer_deviation(a[i], b[i], case["layout"]) for a, b in zip(r32, r64) for i in (1, 2))
    print("%s: 8 x float32-oracle deviation %.2e (recorded %.2e)" % (name, 8 * dev, oc.TAU_F32[name]))
    assert 8 * dev <= 1.5 * oc.TAU_F32[name]
    assert len(case["probes"]) > 0 and case["m0"][case["probes"]].all() and case["v0"][case["probes"]].all()
    if case["kind"] != "critic":  # the flat buffer's last element is a probe: the last shard has one
        assert case["probes"][-1] == len(case["p0"]) - 1
    ref = oc.probe_reference(case)
    assert ref[-1][3] == sum(len(s["steps"]) for s in case["segs"])
