"""The reference side of the edge design (tests/edge_cases.py), on the CPU: the GPU cases of tests/test_gpu_edge.py
cannot hide behind a badly chosen input.

Census.  For every case of edge_cases.CASES: the always-clamped columns are always clamped (raw log_std 2.7 .. 3.3
and -25.4 .. -24.7), the in-range columns never are, the straddling columns (raw 0.6 .. 3.0) have 15 % .. 38 % of
their samples above 2 per case (single columns 0 % .. 92 %), pre-tanh u spans -73 .. +76: samples with
10 < |u| <= 44.4, with |u| > 44.4 and with 1 - t * t == 0 in fp32 exist in every case beside columns that never
saturate, and every oracle output is finite.

Conditioning.  The float32 oracle against the float64 oracle on the same inputs, the largest over the cases
(OMP_NUM_THREADS = 4):
  losses (alpha_loss among them)                      1.8e-7 relative (critic losses 1.5e4 .. 6.3e6; DDPG 2.3e3 .. 3.6e3)
  layout tensors, relative norm / every-element       3.4e-7 / 5.9e-7   (SAC)
                                                      6.0e-7 / 7.0e-7   (DDPG)
  rows of fc_prob.weight / fc_scale.weight            1.5e-6 / 9.3e-7   (Ant row 91 / row 104; every row's norm is
                                                                         above 1e-2 of the tensor's largest)
  rows of the DDPG actors' fc3.weight                 2.7e-5 (|u| ~ 4; 5e-7 at u ~ 0), 8.9e-6 as a share of a bound
                                                      that is 2e-4 with the absolute term; the |u| ~ 12 rows are 0 in
                                                      float32 and 1e-10 of the largest row in float64: 5e-3 of the
                                                      absolute term ROW_FLOOR x largest (edge_cases docstring)
  single elements of fc_prob.bias                     up to 5.2e-5 (a sum of B terms of either sign): held per
                                                      tensor, not per element
  rows that are exactly zero in float64 (always-clamped fc_scale rows: 5 of 11, 8 of 17, 45 of 111, 3 of 6; the
  DDPG actors' |u| ~ 50 rows) are exactly zero in float32
So by the rule of bf16_cases.fp32_elem_tol (the fp32 figure or 4 x the reference's own float32-vs-float64 distance,
whichever is larger) every GPU bound is the existing fp32 figure: losses 1e-4 relative + 1e-6, gradients 2e-4.  The
test holds every distance under a quarter of its bound (5e-5; losses 2.5e-5), so that the rule cannot silently
start to widen a bound.

Teeth.  Three plausible defects of the head math, put into the oracle's actor here (not in oracle/), on Hopper
B = 100, against the oracle without the defect.  The figure is the actor gradient's relative error over the whole
network, which every parity test of the init design asserts, as a multiple of its bound 2e-4:
  defect                                              init design (the other tests')  edge design
  clamp passes gradient outside [-20, 2]              0 (exactly)                     7.4e3; the zero rows are not zero
  log(1 - tanh^2 + 1e-6) for the softplus form        0.55                            4.1e3; loss sac 1.05e4 bounds
  softplus without its threshold (fp32 exp)           0.0015                          not finite
The test asserts < 1 on the init design (the losses too) and >= 10 on the edge design.  On the init design the log
form's largest per-tensor figure is fc_scale.bias's every-element one at 1.01 bounds (on these inputs; 0.55 over the
network), and the per-row figure, which only the edge files compute, 1.38 bounds: seen marginally if at all.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_cases as bc
import edge_cases as ec
from oracle import nets as onets

_RUNS = {}


def _run(name, dtype, edge=True):
    """(oracle, losses) after one update, computed once per (case, precision, design)."""
    key = (name, dtype, edge)
    if key not in _RUNS:
        _RUNS[key] = ec.run_oracle(name, dtype, edge)
    return _RUNS[key]


def test_init_params_restates_the_sac_acm_draw():
    """edge_cases.init_params against bf16_cases.draw_params, which tests/test_gpu_bf16.py holds to the agent."""
    want = bc.draw_params(11, 3, True, 3)
    got = ec.init_params("sac_acm-hopper-33")
    assert set(got) == set(want)
    for k in want:
        for n in want[k]:
            assert np.array_equal(got[k][n], want[k][n]), (k, n)


def test_edge_changes_what_it_says_and_nothing_else():
    p0 = ec.init_params("sac_acm-hcheetah-33")
    p1 = ec.apply_edge(p0)
    a0, a1 = p0["actor"], p1["actor"]
    for n in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc_prob.weight"):
        assert np.array_equal(a0[n], a1[n]), n
    assert a1["fc_scale.bias"][:6].tolist() == [3.0, -25.0, 0.0, np.float32(1.9), -1.0, 3.0]
    assert a1["fc_prob.bias"][:8].tolist() == [0.0, 4.0, -4.0, 12.0, -12.0, 50.0, -50.0, 0.0]
    assert np.array_equal(a1["fc_scale.weight"][3], 4 * a0["fc_scale.weight"][3])
    assert np.array_equal(a1["fc_scale.weight"][4], a0["fc_scale.weight"][4])
    assert np.array_equal(p1["critic_1"]["fc3.weight"], 40 * p0["critic_1"]["fc3.weight"])
    assert p1["critic_2"]["fc3.bias"].tolist() == [100.0]
    for k in ("critic_1", "critic_2"):  # the targets differ from their online nets in every tensor
        for n in p1[k]:
            assert not np.array_equal(p1[k][n], p1[k + "_targ"][n]), (k, n)
    assert np.array_equal(p0["acm"]["fc1.weight"], p1["acm"]["fc1.weight"])
    d = ec.apply_edge(ec.init_params("ddpg-hcheetah-team-33"))
    assert d["actor"]["fc3.bias"].tolist() == [0.0, 4.0, -4.0, 12.0, -12.0, 50.0]
    assert not np.array_equal(d["actor"]["fc3.weight"], d["actor_targ"]["fc3.weight"])
    e = ec.draw_inputs("sac_acm-hopper-33")[1]
    assert not e[:, [1, 6]].any() and e[:, [0, 2, 3, 4, 5]].all()


# ------------------------------------------------------------------ census
@pytest.mark.parametrize("name", list(ec.CASES))
def test_census_every_regime_is_populated(name):
    c = ec.census(name)
    print(name, {k: np.round(v, 2) if v.size <= 17 else (round(float(v.min()), 2), round(float(v.max()), 2))
                 for k, v in c.items()})
    ec.assert_census(name, c)
    o, losses = _run(name, torch.float64)
    for k, v in losses.items():
        assert np.isfinite(v), (name, k)
    for net, g in o.last["grads"].items():
        assert np.isfinite(g).all() and np.abs(g).max() > 0, (name, net)
    assert torch.isfinite(o.last["y"]).all()
    if ec.is_sac(ec.CASES[name][0]):
        assert torch.isfinite(o.last["logp"]).all() and np.isfinite(o.alpha)


def test_init_design_populates_none_of_them():
    """What the other parity tests run on: no clamp, no saturation."""
    c = ec.census("sac_acm-hopper-100", edge=False)
    assert c["above"].max() == 0 and c["below"].max() == 0 and c["u10"].max() == 0 and c["sat"].max() == 0
    assert max(-c["umin"].min(), c["umax"].max()) < 6


# ------------------------------------------------------------------ conditioning
def _distances(name, o, losses, o_ref, l_ref, rows=True):
    """edge_cases.figures of an oracle run against the reference run."""
    alpha = o.alpha if ec.is_sac(ec.CASES[name][0]) else None
    return ec.figures(name, o.last["grads"], losses, alpha, o_ref, l_ref, rows)


@pytest.mark.parametrize("name", list(ec.CASES))
def test_float32_oracle_is_within_a_quarter_of_every_bound(name):
    o64, l64 = _run(name, torch.float64)
    o32, l32 = _run(name, torch.float32)
    d = _distances(name, o32, l32, o64, l64)
    for what in ("loss", "rel", "elem", "row"):
        sel = [x for x in d if what in x[2].split()]
        if sel:
            print(name, what, "max %.1e: %s" % max(sel)[::2])
    for fig, bound, label in d:
        assert fig <= bound / 4, "%s %s: float32 vs float64 %.2e, a quarter of the bound is %.1e" % (
            name, label, fig, bound / 4)
    kind = ec.CASES[name][0]
    rows = ec.head_row_errors(o32.last["grads"]["actor"], o64.last["grads"]["actor"], o64.layouts["actor"],
                              ec.heads_of(kind))
    nzero = sum(int(z.sum()) for _, _, z in rows.values())
    assert nzero > 0, name  # the case has rows that must be exactly zero
    if ec.is_sac(kind):  # no row is small enough to hide: the plain relative error means something for each
        lay = dict(o64.layouts["actor"])
        for t, sl in bc.layout_slices(o64.layouts["actor"]):
            if t in ("fc_prob.weight", "fc_scale.weight"):
                rn = np.linalg.norm(o64.last["grads"]["actor"][sl].reshape(lay[t][0], -1), axis=1)
                assert rn[rn > 0].min() > 1e-2 * rn.max(), (name, t, rn)


# ------------------------------------------------------------------ teeth
def _mutated_actor(defect):
    """oracle.nets.sac_actor (fp32 path) with one defect of the head math."""

    def sac_actor(p, x, lim, eps=None, bf16=False):
        assert not bf16
        h = torch.relu(onets.lin(x, p, "fc1"))
        h = torch.relu(onets.lin(h, p, "fc2"))
        mu = onets.lin(h, p, "fc_prob")
        raw = onets.lin(h, p, "fc_scale")
        ls = torch.clamp(raw, -20, 2)
        if defect == "gate":  # the clamp's value, the identity's gradient
            ls = raw + (ls - raw).detach()
        scale = torch.exp(ls)
        u = mu if eps is None else mu + eps * scale
        var = scale ** 2
        lp = (-((u - mu) ** 2) / (2 * var) - scale.log() - onets.LOG_SQRT_2PI).sum(axis=-1)
        if defect == "log1mt2":
            corr = torch.log(1 - torch.tanh(u) ** 2 + 1e-6).sum(axis=1)
        elif defect == "no_threshold":  # log1p(exp(x)) with the kernels' fp32 exp
            sp = torch.log1p(torch.exp((-2 * u).float())).to(u.dtype)
            corr = 2 * (onets.LOG2 - u - sp).sum(axis=1)
        else:
            corr = 2 * (onets.LOG2 - u - F.softplus(-2 * u)).sum(axis=1)
        return torch.tanh(u) * lim, lp - corr, u

    return sac_actor


TEETH_CASE = "sac_acm-hopper-100"


def _moved(defect, edge, monkeypatch):
    """{label: figure / bound} of the oracle with the defect against the oracle without it."""
    ref = _run(TEETH_CASE, torch.float64, edge)
    with monkeypatch.context() as m:
        m.setattr(onets, "sac_actor", _mutated_actor(defect))
        o, losses = ec.run_oracle(TEETH_CASE, torch.float64, edge)
    return {label: fig / bound for fig, bound, label in _distances(TEETH_CASE, o, losses, *ref)}


def _actor_gradient(moved):
    """The actor gradient's relative error as a multiple of its bound (infinite if the gradient is not finite)."""
    return moved.get("actor not finite", moved.get("actor <net> rel"))


def test_the_restated_actor_is_the_oracles(monkeypatch):
    for edge in (False, True):
        assert max(_moved(None, edge, monkeypatch).values()) == 0.0


@pytest.mark.parametrize("defect", ["gate", "log1mt2", "no_threshold"])
def test_defect_passes_the_init_design_and_misses_the_edge_design(defect, monkeypatch):
    """The figure is the actor gradient's relative error, ||g - g_ref|| / ||g_ref|| over the whole network, which
    every parity test of the init design asserts; every other checked figure is printed with it."""
    init, edge = _moved(defect, False, monkeypatch), _moved(defect, True, monkeypatch)
    for what, m in (("init", init), ("edge", edge)):
        rows = {k: v for k, v in m.items() if " row " in k} or {"no finite row": np.inf}
        rest = {k: v for k, v in m.items() if " row " not in k}
        print("%s, %s design: actor gradient %.3g bounds; worst of the losses and tensors %.3g (%s); worst row %.3g (%s)"
              % (defect, what, _actor_gradient(m), max(rest.values()), max(rest, key=rest.get), max(rows.values()),
                 max(rows, key=rows.get)))
    assert _actor_gradient(init) < 1.0, (defect, _actor_gradient(init))
    assert max(v for k, v in init.items() if k.startswith("loss ")) < 1.0, defect
    assert _actor_gradient(edge) >= 10.0, (defect, _actor_gradient(edge))
