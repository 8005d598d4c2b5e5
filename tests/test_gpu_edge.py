"""GPU parity of the actor-head math where it saturates (tests/edge_cases.py: the design and why; tests/test_edge_ref.py:
the reference's own census, conditioning and teeth on the CPU).

Every other parity test runs on freshly initialised networks, where clamp(log_std, -20, 2) and its gradient gate,
the softplus(-2u) threshold, expf(2u) = inf in sigmoid(-2u) and 1 - t * t == 0 are never reached, Q is O(1) and the
target nets equal the online ones.  The cases here run one update on the edge parameters and inputs through every
hand-typed copy of that math: the narrow heads (heads_backward), the wide Ant heads (k_sac_actor_heads), the team
kernels (sac_team.h), squash_write, k_policy_act and the DDPG actors (ddpg.hip, ddpg_team.h).

Against the float64 oracle, with the fp32 bounds of tests/test_gpu_bigbatch.py unchanged (the reference's own
float32-vs-float64 distance in this regime is at most 1.5e-6, tests/test_edge_ref.py): losses (alpha_loss among them)
1e-4 relative + 1e-6, gradients 2e-4 per network, per layout tensor (norm and every element) and per row of the head
weights; rows whose reference is exactly zero (always-clamped log_std columns, DDPG columns saturated in float64)
exactly 0.0; alpha after the step to 1e-5.  DDPG rows get the absolute term of edge_cases.ROW_FLOOR, and the
fc3 rows of the columns with |u| > 10 on every sample must be exactly zero (fp32 tanh is 1.0 there).

Bit for bit between kernel forms on the edge parameters: SPP_MINQ_SPLIT 0 / 1, SPP_STAGE_SPLIT 0 / 7,
SPP_CRITIC_PAIRS 0 / 3, each asserted through sppAgentStageSplit / sppAgentCriticPairs to have run as asked.

Rollout action (sppPolicyAct), sampled and deterministic, on the edge actor: against oracle.nets with the tolerance of
tests/test_gpu_parity.py::test_policy_act_matches_oracle; columns with |u| > 10 come out at exactly +-lim
(denormalised); nothing is NaN.

-s prints every figure and, per case, the figure nearest its bound.  Measured on an MI355X: no case is nearer than
0.009 of a bound for SAC (row 3 of fc_scale.weight, the straddling column, 1.9e-6 at Hopper B = 100; network gradients
6e-8 .. 6e-7, losses to 7 digits) and 0.054 for DDPG (an fc3.weight row at |u| ~ 4, 1.1e-5); sppPolicyAct within
3.7e-6.  A scratch build without the clamp gate in heads_backward (csrc/sac.hip) fails the seven cases that run that
copy (actor gradient 0.8 .. 1.5 relative) and passes the Ant, team-kernel and DDPG cases.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import spprl  # noqa: E402
import bf16_cases as bc  # noqa: E402
import edge_cases as ec  # noqa: E402
import test_gpu_bigbatch as bb  # noqa: E402
import test_gpu_critic_pairs as cp  # noqa: E402
import test_gpu_gen_inputs as gi  # noqa: E402
import test_gpu_stage_split as ss  # noqa: E402
from ddpg_ref import noise_action  # noqa: E402
from oracle import nets as onets  # noqa: E402
from spprl import _lib  # noqa: E402

DEV = bb.DEV
F64 = torch.float64
DDPG_VANILLA_NETS = {"actor": _lib.SPP_NET_ACTOR, "critic": _lib.SPP_NET_CRITIC1,
                     "actor_targ": _lib.SPP_NET_ACTOR_TARG, "critic_targ": _lib.SPP_NET_CRITIC1_TARG}
CLASSES = {"sac_acm": (spprl.SAC_AcM, bb.SAC_NETS), "sac": (spprl.SAC, gi.VANILLA_NETS),
           "ddpg_acm": (spprl.DDPG_AcM, bb.DDPG_NETS), "ddpg": (spprl.DDPG, DDPG_VANILLA_NETS)}


def _load_edge(ag, nets):
    """Reshape the agent's own parameters by the edge design; returns them."""
    edge = ec.apply_edge(bb.snapshot(ag, nets))
    for k, net in nets.items():
        ag.load_net(net, edge[k])
    return edge


def _set_minmax(ag, lohi):
    rb = ag.replay_buffer
    rb.min_obs.copy_(torch.from_numpy(lohi[0]))
    rb.max_obs.copy_(torch.from_numpy(lohi[1]))
    rb._have_minmax = True


def _edge_agent(name, monkeypatch, max_batch=None):
    """The case's agent on the edge parameters: (agent, its net ids, the parameters, the inputs)."""
    kind, env, _, B, _, sw = ec.CASES[name]
    if sw.get("team") is None:
        monkeypatch.delenv("SPP_SAC_TEAM", raising=False)  # read when the agent is made
    else:
        monkeypatch.setenv("SPP_SAC_TEAM", sw["team"])
    cls, nets = CLASSES[kind]
    ag = cls(env_name=env, max_batch=max_batch or B, buffer_size=128, device=DEV, **ec.agent_kwargs(name))
    init = ec.init_params(name)  # the CPU checks of tests/test_edge_ref.py ran on these
    own = bb.snapshot(ag, nets)
    for k in init:
        for n in init[k]:
            assert np.array_equal(own[k][n], init[k][n]), (name, k, n)
    params = _load_edge(ag, nets)
    inp = ec.draw_inputs(name)
    if kind in ("sac_acm", "ddpg_acm"):
        _set_minmax(ag, inp[3])
    return ag, nets, params, inp


def _report(name, figs):
    fig, bound, label = max(figs, key=lambda f: f[0] / f[1])
    print("%s: nearest its bound: %s %.2e = %.3f of %.0e" % (name, label, fig, fig / bound, bound))
    for fig, bound, label in figs:
        assert fig < bound, "%s %s: %.3e, bound %.1e" % (name, label, fig, bound)


# ------------------------------------------------------------------ SAC_AcM and vanilla SAC against the oracle
@pytest.mark.parametrize("name", ec.SAC_CASES)
def test_sac_update_matches_oracle(name, monkeypatch):
    kind = ec.CASES[name][0]
    ag, nets, params, (batch, e1, e2, lohi) = _edge_agent(name, monkeypatch)
    if kind == "sac":
        ag.update(*batch[:5], eps_next=e1, eps_cur=e2)
    else:
        ag.update(*batch, eps_next=e1, eps_cur=e2)
    torch.cuda.synchronize()
    o = ec.make_oracle(name, params, lohi, F64)
    ol = ec.oracle_update(name, o, batch, e1, e2)
    raw = ag._losses.detach().cpu().numpy()
    losses = dict(ag.loss, alpha_loss=float(raw[5]))
    grads = {k: ag.grads[nets[k]].cpu().numpy() for k in ec.trained_nets(kind)}
    assert all(np.isfinite(g).all() for g in grads.values()) and np.isfinite(raw).all()
    rows = ec.head_row_errors(grads["actor"], o.last["grads"]["actor"], o.layouts["actor"], ec.SAC_HEADS)
    print(name, "head rows", ec.fmt_rows(rows), "alpha_loss", (losses["alpha_loss"], ol["alpha_loss"]), "alpha",
          (ag.current_alpha(), o.alpha))
    bb.check_sac(ag, o, ol, grad_tol=ec.GRAD_TOL, loss_tol=ec.LOSS_TOL, params_check=False)
    ec.assert_head_rows(grads["actor"], o.last["grads"]["actor"], o.layouts["actor"], ec.SAC_HEADS, ec.GRAD_TOL, name)
    assert abs(losses["alpha_loss"] - ol["alpha_loss"]) <= ec.LOSS_TOL * abs(ol["alpha_loss"]) + 1e-6
    assert ag.current_alpha() == pytest.approx(o.alpha, rel=1e-5)
    assert float(raw[6]) == pytest.approx(o.alpha, rel=1e-5)  # the loss vector's alpha entry
    _report(name, ec.figures(name, grads, losses, ag.current_alpha(), o, ol))


# ------------------------------------------------------------------ DDPG_AcM and vanilla DDPG against their oracles
@pytest.mark.parametrize("name", ec.DDPG_CASES)
def test_ddpg_update_matches_oracle(name, monkeypatch):
    kind, _, _, B, _, _ = ec.CASES[name]
    ag, nets, params, (batch, e1, e2, lohi) = _edge_agent(name, monkeypatch)
    ag.update(*(batch if kind == "ddpg_acm" else batch[:5]))
    torch.cuda.synchronize()
    o = ec.make_oracle(name, params, lohi, F64)
    ol = ec.oracle_update(name, o, batch, e1, e2)
    gl = ag.loss
    assert set(gl) == set(ol)
    grads = {k: ag.grads[nets[k]].cpu().numpy() for k in ("critic", "actor")}
    assert all(np.isfinite(g).all() for g in grads.values())
    rows = ec.head_row_errors(grads["actor"], o.last["grads"]["actor"], o.layouts["actor"], ec.DDPG_HEADS, ec.ROW_FLOOR)
    print(name, "head rows", ec.fmt_rows(rows), "losses", {k: (round(gl[k], 6), round(ol[k], 6)) for k in gl})
    for k in ("critic", "actor"):
        e = bb.relerr(grads[k], o.last["grads"][k])
        print(name, k, "grad rel err %.2e" % e)
        assert e < ec.GRAD_TOL, (k, e)
        bc.assert_tensor_grads(grads[k], o.last["grads"][k], o.layouts[k], ec.GRAD_TOL, k, bc.fp32_elem_tol(B))
    for k in ol:
        assert abs(gl[k] - ol[k]) <= ec.LOSS_TOL * abs(ol[k]) + 1e-6, (k, gl[k], ol[k])
    ec.assert_head_rows(grads["actor"], o.last["grads"]["actor"], o.layouts["actor"], ec.DDPG_HEADS, ec.GRAD_TOL, name,
                        ec.ROW_FLOOR)
    # columns saturated on every sample of the actor's forward on obs: fp32 tanh is exactly 1.0, the row exactly zero
    u = ec.pre_tanh(name, params)[1][0]
    sat, live = np.all(np.abs(u) > 10, axis=0), np.all(np.abs(u) < 9, axis=0)
    assert sat.any() and live.any()
    lay = dict(o.layouts["actor"])
    for t, sl in bc.layout_slices(o.layouts["actor"]):
        if t in ec.DDPG_HEADS:
            g = grads["actor"][sl].reshape(lay[t][0], -1)
            assert not g[sat].any(), "%s %s: a saturated column's row is not exactly zero" % (name, t)
            assert g[live].any(axis=1).all(), (name, t)
    _report(name, ec.figures(name, grads, gl, None, o, ol))


# ------------------------------------------------------------------ bit for bit between kernel forms
def _forms(switch, set_name, B, monkeypatch):
    """The two agents of a switch on the same seed: [(asked-for value, agent)]."""
    out = []
    if switch == "stage":
        monkeypatch.delenv("SPP_MINQ_SPLIT", raising=False)
        monkeypatch.delenv("SPP_CRITIC_PAIRS", raising=False)
        return [(bits, ss._make(set_name, B, bits, monkeypatch)) for bits in (0, 7)]  # asserts sppAgentStageSplit
    if switch == "pairs":
        monkeypatch.delenv("SPP_MINQ_SPLIT", raising=False)
        return [(bits, cp._make(set_name, B, bits, monkeypatch)) for bits in (0, 3)]  # asserts sppAgentCriticPairs
    cls, env, ob, aout, ac, kw = ss.SETS[set_name]
    monkeypatch.delenv("SPP_SAC_TEAM", raising=False)
    monkeypatch.delenv("SPP_STAGE_SPLIT", raising=False)
    monkeypatch.delenv("SPP_CRITIC_PAIRS", raising=False)
    for split in (0, 1):
        monkeypatch.setenv("SPP_MINQ_SPLIT", str(split))  # read when the agent is made
        ag = cls(env_name=env, max_batch=B, buffer_size=128, device=DEV, seed=3, **kw)
        # the stage cuts are cuts of the split phase: they run only where the min-critic split does
        cuts = ctypes.c_int(-1)
        _lib.call("sppAgentStageSplit", ag._h, ctypes.byref(cuts))
        assert cuts.value == (7 if split else 0), "SPP_MINQ_SPLIT=%d: the agent runs cuts %d" % (split, cuts.value)
        out.append((split, ag))
    return out


@pytest.mark.parametrize("B", [33, 100])
@pytest.mark.parametrize("set_name", ["hopper", "hcheetah"])
@pytest.mark.parametrize("switch", ["minq", "stage", "pairs"])
def test_kernel_forms_agree_bitwise_on_the_edge_parameters(switch, set_name, B, monkeypatch):
    _, _, ob, aout, ac, _ = ss.SETS[set_name]
    batch, e1, e2, (lo, hi) = ec.draw_inputs_for(B, ob, aout, ac)
    states = []
    for _, ag in _forms(switch, set_name, B, monkeypatch):
        _load_edge(ag, bb.SAC_NETS)
        ss._step(set_name, ag, (lo, hi, batch, e1, e2))
        states.append(ss._state(set_name, ag))
    ref, got = states
    for k in ("grad critic_1", "grad critic_2", "grad actor", "losses"):
        assert np.isfinite(ref[k]).all() and np.abs(ref[k]).max() > 0, k
    assert ref["losses"][0] > 1000  # the edge regime: Q ~ 100
    for k in ref:
        assert np.array_equal(ref[k], got[k]), "%s: %d elements differ" % (k, int(np.sum(ref[k] != got[k])))


# ------------------------------------------------------------------ rollout action
def _saturated(u):
    """Entries whose fp32 tanh is exactly +-1 with margin (1 - tanh(10) = 4e-9, under half an ulp of 1)."""
    sat = np.abs(u) > 10
    assert sat.any() and not sat.all()
    return sat


def test_sac_acm_policy_act_on_the_edge_actor(monkeypatch):
    name = "sac_acm-hopper-33"
    _, _, (ob, aout, ac), E, _, _ = ec.CASES[name]
    ag, nets, params, (_, _, _, lohi) = _edge_agent(name, monkeypatch)
    rng = np.random.RandomState(5)
    obs = (rng.randn(E, ob) * 1.3).astype(np.float32)
    eps = ec.draw_eps(rng, E, aout)
    P = {k: {n: torch.from_numpy(v) for n, v in params[k].items()} for k in ("actor", "acm")}
    P64 = {n: v.to(F64) for n, v in P["actor"].items()}
    norm = onets.Norm(True, torch.from_numpy(lohi[0]), torch.from_numpy(lohi[1]))
    lim = torch.ones(aout)
    one = norm.denormalize(torch.ones(E, aout)).numpy()
    mone = norm.denormalize(-torch.ones(E, aout)).numpy()
    for what, e in (("sampled", eps), ("deterministic", None)):
        tgt, env = ag.act(torch.from_numpy(obs), eps=None if e is None else torch.from_numpy(e).to(DEV), noise=None,
                          mode=1 if e is not None else 2, act_noise=0.0)
        torch.cuda.synchronize()
        tgt, env = tgt.cpu().numpy(), env.cpu().numpy()
        with torch.no_grad():
            et = None if e is None else torch.from_numpy(e)
            a, _, _ = onets.sac_actor(P["actor"], torch.from_numpy(obs), lim, et)
            ad = norm.denormalize(torch.clamp(a, -1.1 * lim, 1.1 * lim))
            c = onets.acm(P["acm"], torch.cat([torch.from_numpy(obs), ad], 1), torch.ones(ac))
            u = onets.sac_actor(P64, torch.from_numpy(obs).to(F64), lim.to(F64), None if e is None else et.to(F64))[2]
        assert np.isfinite(tgt).all() and np.isfinite(env).all(), what
        print(what, "target max |d| %.2e, env max |d| %.2e" % (np.abs(tgt - ad.numpy()).max(),
                                                               np.abs(env - c.numpy()).max()))
        np.testing.assert_allclose(tgt, ad.numpy(), rtol=1e-4, atol=1e-5, err_msg=what)
        np.testing.assert_allclose(env, c.numpy(), rtol=1e-4, atol=1e-5, err_msg=what)
        u = u.numpy()
        sat = _saturated(u)
        assert np.array_equal(tgt[sat], np.where(u > 0, one, mone)[sat]), what  # exactly denormalize(+-lim)


def test_ddpg_policy_act_on_the_edge_actor(monkeypatch):
    name = "ddpg-hcheetah-team-33"
    _, _, (ob, aout, ac), E, _, _ = ec.CASES[name]
    ag, nets, params, _ = _edge_agent(name, monkeypatch)
    rng = np.random.RandomState(6)
    obs = (rng.randn(E, ob) * 1.3).astype(np.float32)
    noise = rng.randn(E, ac).astype(np.float32)
    t = lambda z: torch.from_numpy(z).to(DEV)  # noqa: E731
    p64 = {n: torch.from_numpy(v).to(F64) for n, v in params["actor"].items()}
    h = torch.relu(onets.lin(torch.from_numpy(obs).to(F64), p64, "fc1"))
    u = onets.lin(torch.relu(onets.lin(h, p64, "fc2")), p64, "fc3").numpy()
    sat = _saturated(u)
    tgt, env = ag.act(t(obs), noise=t(noise), mode=1)  # noise_action with the agent's act_noise
    torch.cuda.synchronize()
    want = noise_action(params["actor"], obs, 1.0, noise, ag.act_noise)
    assert np.isfinite(env.cpu().numpy()).all() and np.abs(env.cpu().numpy()).max() <= 1.0
    np.testing.assert_allclose(env.cpu().numpy(), want, rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(tgt.cpu().numpy(), env.cpu().numpy())
    tgt, env = ag.act(t(obs), mode=2, act_noise=0.0)  # deterministic
    torch.cuda.synchronize()
    got = env.cpu().numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, noise_action(params["actor"], obs, 1.0, None, 0.0), rtol=1e-4, atol=1e-5)
    assert np.array_equal(got[sat], np.sign(u)[sat].astype(np.float32))  # exactly +-lim
    np.testing.assert_array_equal(tgt.cpu().numpy(), got)
