"""The edge design of the actor-head parity tests (tests/test_edge_ref.py on the CPU, tests/test_gpu_edge.py on
the GPU), importable without a GPU.

Every other parity test updates freshly initialised networks on randn inputs, where the per-sample head math
(clamp(log_std, -20, 2) and its gradient gate, tanh, 1 - t^2, softplus(-2u) with its threshold at 20,
sigmoid(-2u) through expf(2u)) never leaves its easy region and target nets equal the online ones.  This module
reshapes the seeded init parameters so that one update covers the regimes a trained policy lives in:

  actor fc_scale.bias[j]   LS_BIAS[j % 5] = 3, -25, 0, 1.9, -1; fc_scale.weight rows j % 5 == 3 times 4: a column always
                           above the upper clamp, one always below the lower, two in range, one straddling 2
  actor fc_prob.bias[j]    MU_BIAS[j % 7] = 0, 4, -4, 12, -12, 50, -50 (DDPG actors: the same on fc3.bias): |u| > 10 (the
                           softplus threshold branch), |u| > 44.4 (expf(2u) is inf), 1 - t * t == 0 in fp32
  eps, both draws          0 in the columns j % 5 == 1: at log_std = -20 the reference's own fp32 (u - mu)^2 / (2 var)
                           is chaotic (u - mu is 0 or one ulp of mu), so no reference exists for eps != 0; with
                           u == mu the lower gate is still observable: d loss / d log_std is -g_lp if it leaks, else 0
  critics, target critics  fc3.weight times 40, fc3.bias = 100: Q ~ 100, critic losses in the thousands
  every target net         each parameter times 1 + 0.1 randn (own seeded generator): targets differ from online nets
  batch                    done with probability 0.3, rewards 5 randn; alpha and gamma away from their defaults

init_params restates the agents' seeded draws on the CPU (the GPU test asserts that it equals the agent's own
parameters), so that the CPU test checks the reference on exactly the GPU test's inputs.

Per-row check of the head tensors (head_row_errors).  A wrong column of the head math is one row of fc_prob.weight /
fc_scale.weight (fc3.weight for DDPG); inside the tensor's norm a small row hides.  Every row gets
||g - g_ref|| / ||g_ref|| < tol, and rows whose reference is all zero (an always-clamped log_std column; a DDPG
column whose tanh is 1.0 in float64 too) must be exactly 0.0.
DDPG only: a row of fc3.weight is all (1 - t * t), and fp32 tanh has spacing 2^-24 below 1, so the fp32 1 - t * t is
a multiple of ~2^-23: its absolute error is 2^-23 of an unsaturated column's value whatever its own size (|u| ~ 12:
1.5e-10 in float64, exactly 0 in fp32; |u| ~ 4: 1.3e-3 +- 6e-8).  Such a row's bound is tol ||g_ref|| + ROW_FLOOR x
the tensor's largest row norm, ROW_FLOOR = 2^-23.  The SAC rows carry the log-prob's O(1) term and get no absolute
term: there the rule is the plain relative error.
"""
import numpy as np
import torch

import bf16_cases as bc
from oracle import nets as onets
from oracle.ddpg_acm import OracleDdpgAcm
from oracle.sac import OracleSac
from oracle.sac_acm import OracleSacAcm

LS_BIAS = (3.0, -25.0, 0.0, 1.9, -1.0)
MU_BIAS = (0.0, 4.0, -4.0, 12.0, -12.0, 50.0, -50.0)
STRADDLE_GAIN = 4.0
Q_GAIN, Q_BIAS = 40.0, 100.0
TARGET_JITTER = 0.1
ROW_FLOOR = 2.0 ** -23
GRAD_TOL, LOSS_TOL = bc.FP32_GRAD_TOL, bc.FP32_LOSS_TOL
ALPHA, GAMMA_SAC, GAMMA_DDPG = 0.7, 0.97, 0.9

# name: kind, env, (ob, aout, ac), B, agent seed, switches.  team: SPP_SAC_TEAM for the vanilla agents (None: unset)
CASES = {
    "sac_acm-hopper-33": ("sac_acm", "Hopper-v2", (11, 11, 3), 33, 3, dict(acm_critic=True, norm_closs=False)),
    "sac_acm-hopper-100": ("sac_acm", "Hopper-v2", (11, 11, 3), 100, 3, dict(acm_critic=True, norm_closs=False)),
    "sac_acm-hopper-acmc0-33": ("sac_acm", "Hopper-v2", (11, 11, 3), 33, 3, dict(acm_critic=False, norm_closs=False)),
    "sac_acm-hopper-acmc0-100": ("sac_acm", "Hopper-v2", (11, 11, 3), 100, 3, dict(acm_critic=False, norm_closs=False)),
    "sac_acm-hcheetah-33": ("sac_acm", "HalfCheetah-v2", (17, 17, 6), 33, 3, dict(acm_critic=True, norm_closs=False)),
    "sac_acm-ant-64": ("sac_acm", "Ant-v2", (111, 111, 8), 64, 3, dict(acm_critic=True, norm_closs=False)),
    "sac_acm-hopper-normcloss-33": ("sac_acm", "Hopper-v2", (11, 11, 3), 33, 3, dict(acm_critic=True, norm_closs=True)),
    "sac-hcheetah-team-33": ("sac", "HalfCheetah-v2", (17, 6, 6), 33, 5, dict(team=None)),
    "sac-hcheetah-onewave-100": ("sac", "HalfCheetah-v2", (17, 6, 6), 100, 5, dict(team="0")),
    "ddpg_acm-hopper-33": ("ddpg_acm", "Hopper-v2", (11, 11, 3), 33, 4, dict()),
    "ddpg_acm-hcheetah-33": ("ddpg_acm", "HalfCheetah-v2", (17, 17, 6), 33, 4, dict()),
    "ddpg-hcheetah-team-33": ("ddpg", "HalfCheetah-v2", (17, 6, 6), 33, 5, dict(team=None)),
    "ddpg-hcheetah-onewave-100": ("ddpg", "HalfCheetah-v2", (17, 6, 6), 100, 5, dict(team="0")),
}
SAC_CASES = [k for k, v in CASES.items() if v[0] in ("sac_acm", "sac")]
DDPG_CASES = [k for k, v in CASES.items() if v[0] in ("ddpg_acm", "ddpg")]
SAC_HEADS = ("fc_prob.weight", "fc_prob.bias", "fc_scale.weight", "fc_scale.bias")
DDPG_HEADS = ("fc3.weight", "fc3.bias")


def is_sac(kind):
    return kind in ("sac_acm", "sac")


def agent_kwargs(name):
    """The constructor keywords of the case's agent (env_name, max_batch, buffer_size and device are the caller's)."""
    kind, _, _, _, seed, sw = CASES[name]
    if kind == "sac_acm":
        return dict(acm_critic=sw["acm_critic"], custom_loss=0.2, norm_closs=sw["norm_closs"], min_max_denormalize=True,
                    denormalize_actor_out=True, gamma=GAMMA_SAC, alpha=ALPHA, seed=seed)
    if kind == "sac":
        return dict(gamma=GAMMA_SAC, actor_lr=1e-3, critic_lr=1e-3, alpha_lr=1e-3, alpha=ALPHA, seed=seed)
    if kind == "ddpg_acm":
        return dict(gamma=GAMMA_DDPG, actor_lr=5e-4, critic_lr=5e-4, acm_critic=True, custom_loss=1.0, norm_closs=False,
                    min_max_denormalize=True, denormalize_actor_out=True, seed=seed)
    return dict(gamma=GAMMA_DDPG, actor_lr=1e-3, critic_lr=1e-3, seed=seed)


# ------------------------------------------------------------------ parameters
def net_layouts(kind, ob, aout, ac, acm_critic=True):
    """[(net, layout)] in the order the agent's constructor draws them."""
    from spprl import nets as snets

    if is_sac(kind):
        cin = ob + (ac if (acm_critic and kind == "sac_acm") else aout)
        return [("actor", snets.sac_actor_layout(ob, aout)), ("critic_1", snets.critic_layout(cin)),
                ("critic_2", snets.critic_layout(cin)), ("critic_1_targ", snets.critic_layout(cin)),
                ("critic_2_targ", snets.critic_layout(cin)), ("acm", snets.acm_layout(2 * ob, ac))]
    cin = ob + (ac if kind == "ddpg_acm" else aout)
    lays = [("actor", snets.ddpg_actor_layout(ob, aout)), ("actor_targ", snets.ddpg_actor_layout(ob, aout)),
            ("critic", snets.critic_layout(cin)), ("critic_targ", snets.critic_layout(cin))]
    if kind == "ddpg_acm":
        lays.append(("acm", snets.basic_acm_layout(2 * ob, ac)))
    return lays


def init_params(name):
    """{net: {tensor: float32 array}}: the default-initialised parameters of the case's agent, drawn as its
    constructor draws them (one seeded generator through spprl.nets.linear_init_, targets copied)."""
    from spprl import nets as snets

    kind, _, (ob, aout, ac), _, seed, sw = CASES[name]
    lays = net_layouts(kind, ob, aout, ac, sw.get("acm_critic", True))
    gen = torch.Generator().manual_seed(seed)
    flat = {k: snets.linear_init_(torch.empty(snets.numel(lay)), lay, gen) for k, lay in lays}
    for k in flat:
        if k.endswith("_targ"):
            flat[k].copy_(flat[k[:-5]])
    out = {k: {n: v.numpy().copy() for n, v in snets.state_dict(flat[k], lay).items()} for k, lay in lays}
    if kind == "sac":
        del out["acm"]  # drawn (it moves nothing after it), never used
    return out


def apply_edge(params, seed=0):
    """The edge design over a {net: {tensor: array}} dict; returns a new dict of float32 arrays."""
    out = {k: {n: np.array(v, np.float32) for n, v in p.items()} for k, p in params.items()}
    for k, p in out.items():
        if k.startswith("actor"):
            head = "fc_prob.bias" if "fc_prob.bias" in p else "fc3.bias"
            j = np.arange(p[head].shape[0])
            p[head][:] = np.asarray(MU_BIAS, np.float32)[j % 7]
            if "fc_scale.bias" in p:
                p["fc_scale.bias"][:] = np.asarray(LS_BIAS, np.float32)[j % 5]
                p["fc_scale.weight"][j % 5 == 3] *= np.float32(STRADDLE_GAIN)
        if k.startswith("critic"):
            p["fc3.weight"] *= np.float32(Q_GAIN)
            p["fc3.bias"][:] = Q_BIAS
    for i, k in enumerate(sorted(out)):
        if k.endswith("_targ"):
            rng = np.random.RandomState(1000 * seed + 17 + i)
            for n, v in out[k].items():
                v *= (1 + TARGET_JITTER * rng.randn(*v.shape)).astype(np.float32)
    return out


# ------------------------------------------------------------------ inputs
def draw_inputs(name, edge=True):
    """(batch6, eps_next, eps_cur, (lo, hi)) of the case.  edge=False: the init regime of the other parity tests
    (tests/test_gpu_bigbatch.py random_batch: rewards randn, done with probability 0.05, dense eps)."""
    kind, _, (ob, aout, ac), B, _, _ = CASES[name]
    return draw_inputs_for(B, ob, aout, ac, edge)


def draw_inputs_for(B, ob, aout, ac, edge=True):
    rng = np.random.RandomState(B % 1000 + ob + 7 * aout)
    lo = -rng.uniform(0.5, 2, ob).astype(np.float32)
    hi = rng.uniform(0.5, 2, ob).astype(np.float32)
    batch = (rng.randn(B, ob).astype(np.float32), rng.randn(B, ob).astype(np.float32),
             rng.uniform(-1, 1, (B, aout)).astype(np.float32),
             ((5.0 if edge else 1.0) * rng.randn(B)).astype(np.float32),
             (rng.rand(B) < (0.3 if edge else 0.05)).astype(np.int8), rng.uniform(-1, 1, (B, ac)).astype(np.float32))
    e1, e2 = draw_eps(rng, B, aout, edge), draw_eps(rng, B, aout, edge)
    return batch, e1, e2, (lo, hi)


def draw_eps(rng, B, aout, edge=True):
    e = rng.randn(B, aout).astype(np.float32)
    if edge:
        e[:, np.arange(aout) % 5 == 1] = 0.0
    return e


# ------------------------------------------------------------------ oracles
def make_oracle(name, params, lohi, dtype=torch.float64, edge=True):
    """The case's oracle on params.  edge=False: alpha at its default 0.2 (the init regime)."""
    kind, _, (ob, aout, ac), _, _, sw = CASES[name]
    norm = onets.Norm(True, torch.from_numpy(lohi[0]).to(dtype), torch.from_numpy(lohi[1]).to(dtype))
    alpha = ALPHA if edge else 0.2
    if kind == "sac_acm":
        return OracleSacAcm(ob, aout, ac, acm_critic=sw["acm_critic"], custom_loss=0.2, norm_closs=sw["norm_closs"],
                            norm=norm, actor_lim=1.0, acm_lim=np.ones(ac, np.float32), gamma=GAMMA_SAC, alpha=alpha,
                            params=params, dtype=dtype)
    if kind == "sac":
        return OracleSac(ob, ac, gamma=GAMMA_SAC, alpha=alpha, params=params, dtype=dtype)
    if kind == "ddpg_acm":
        return OracleDdpgAcm(ob, aout, ac, norm=norm, actor_lim=1.0, gamma=GAMMA_DDPG, tau=0.005, params=params,
                             dtype=dtype)
    from ddpg_ref import DdpgRef

    return DdpgRef(ob, ac, gamma=GAMMA_DDPG, params=params, dtype=dtype)


def oracle_update(name, o, batch, e1, e2):
    """One update of the case's oracle; returns its losses (SAC: alpha_loss among them)."""
    kind = CASES[name][0]
    if kind == "sac_acm":
        return o.update(*batch, e1, e2)
    if kind == "sac":
        return o.update(*batch[:5], e1, e2)
    if kind == "ddpg_acm":
        return o.update(*batch)
    return o.update(*batch[:5])


def run_oracle(name, dtype=torch.float64, edge=True, params=None):
    """(oracle after one update, its losses) of the case on the edge (or the init) design."""
    if params is None:
        params = init_params(name)
        params = apply_edge(params) if edge else params
    batch, e1, e2, lohi = draw_inputs(name, edge)
    o = make_oracle(name, params, lohi, dtype, edge)
    return o, oracle_update(name, o, batch, e1, e2)


def trained_nets(kind):
    return ("critic_1", "critic_2", "actor") if is_sac(kind) else ("critic", "actor")


def heads_of(kind):
    return SAC_HEADS if is_sac(kind) else DDPG_HEADS


# ------------------------------------------------------------------ per-row comparison of the head tensors
def head_row_errors(g, g_ref, layout, tensors, floor=0.0):
    """{tensor: (err [rows], extra [rows], zero [rows] bool)} of a flat actor gradient against its reference.  A bias
    is a tensor of one-element rows.  err is ||g - g_ref|| / ||g_ref|| of the row; for a zero row (the reference is
    all zero) 0.0 if the row is exactly zero, inf otherwise.  extra = floor x (the tensor's largest row norm) /
    ||g_ref||: what the row's bound grows by under the absolute term (module docstring; 0 for SAC)."""
    g, g_ref = np.asarray(g, np.float64).ravel(), np.asarray(g_ref, np.float64).ravel()
    shapes = dict(layout)
    out = {}
    for t, sl in bc.layout_slices(layout):
        if t not in tensors:
            continue
        rows = shapes[t][0]
        a, r = g[sl].reshape(rows, -1), g_ref[sl].reshape(rows, -1)
        rn = np.linalg.norm(r, axis=1)
        dn = np.linalg.norm(a - r, axis=1)
        zero = ~r.any(axis=1)
        err = dn / np.maximum(rn, 1e-300)
        err[zero] = np.where(a[zero].any(axis=1), np.inf, 0.0)
        extra = floor * rn.max() / np.maximum(rn, 1e-300)
        extra[zero] = 0.0
        out[t] = (err, extra, zero)
    return out


def assert_head_rows(g, g_ref, layout, tensors, tol, what="", floor=0.0):
    """The reference's zero rows exactly 0.0 in every tensor; every row of the weight tensors within tol (+ the
    absolute term).  The biases' elements are sums of B terms of either sign (one measured 5e-5 between the float32
    and the float64 oracle): they are held by the per-tensor check, not one by one.  Returns the errors."""
    errs = head_row_errors(g, g_ref, layout, tensors, floor)
    for t, (err, extra, zero) in errs.items():
        for j in np.nonzero(zero)[0]:
            assert err[j] == 0.0, "%s %s row %d: the reference is exactly zero, the row is not" % (what, t, j)
        if t.endswith(".weight"):
            j = int(np.argmax(err / (tol + extra)))
            assert err[j] < tol + extra[j], "%s %s row %d: ||g - g_ref|| / ||g_ref|| = %.3e, bound %.1e" % (
                what, t, j, err[j], tol + extra[j])
    return errs


def figures(name, grads, losses, alpha, o_ref, l_ref, rows=True):
    """[(figure, bound, label)]: every figure the GPU test checks, of one update's results (grads {net: flat
    gradient}, losses {key: value} for the keys of l_ref that are there, alpha after the step or None) against the
    reference oracle after its update.  A figure whose bound has an absolute part is scaled so that figure / bound
    says how near the bound it is; a zero row's figure is 0.0 or inf.  rows=False: without the per-row figures,
    i.e. what the parity tests of the init design check."""
    kind = CASES[name][0]
    out = []
    for k, want in l_ref.items():
        if k in losses:
            d = abs(losses[k] - want) if np.isfinite(losses[k]) else np.inf
            out.append((d / (LOSS_TOL * abs(want) + 1e-6) * LOSS_TOL, LOSS_TOL, "loss " + k))
    for net in trained_nets(kind):
        g, r = np.asarray(grads[net]), o_ref.last["grads"][net]
        if not np.isfinite(g).all():
            out.append((np.inf, GRAD_TOL, net + " not finite"))
            continue
        for t, (rel, elem) in bc.tensor_errors(g, r, o_ref.layouts[net]).items():
            out.append((rel, GRAD_TOL, "%s %s rel" % (net, t)))
            out.append((elem, GRAD_TOL, "%s %s elem" % (net, t)))
    g, r = np.asarray(grads["actor"]), o_ref.last["grads"]["actor"]
    if rows and np.isfinite(g).all():
        errs = head_row_errors(g, r, o_ref.layouts["actor"], heads_of(kind), 0.0 if is_sac(kind) else ROW_FLOOR)
        for t, (err, extra, zero) in errs.items():
            for j in range(len(err)):
                if zero[j]:
                    out.append((err[j], GRAD_TOL, "actor %s zero row %d" % (t, j)))
                elif t.endswith(".weight"):
                    out.append((err[j] / (GRAD_TOL + extra[j]) * GRAD_TOL, GRAD_TOL, "actor %s row %d" % (t, j)))
    if alpha is not None:
        out.append((abs(alpha - o_ref.alpha) / o_ref.alpha / 1e-5 * LOSS_TOL, LOSS_TOL, "alpha"))
    return out


def fmt_rows(errs):
    return {t: "max %.1e (row %d), %d zero" % (e.max(), int(np.argmax(e)), int(z.sum())) for t, (e, x, z) in errs.items()}


# ------------------------------------------------------------------ regime census
def pre_tanh(name, params=None, edge=True):
    """[(u, raw log_std or None)] (float64 arrays [B][aout]) of the update's two actor forwards: SAC: next_obs with
    eps_next, then obs with eps_cur; DDPG: the target actor on next_obs, then the actor on obs."""
    kind = CASES[name][0]
    if params is None:
        params = init_params(name)
        params = apply_edge(params) if edge else params
    batch, e1, e2, _ = draw_inputs(name, edge)
    t64 = lambda a: torch.as_tensor(np.asarray(a)).to(torch.float64)  # noqa: E731
    passes = ((batch[1], e1, "actor"), (batch[0], e2, "actor")) if is_sac(kind) else (
        (batch[1], None, "actor_targ"), (batch[0], None, "actor"))
    out = []
    for x, e, net in passes:
        p = {n: t64(v) for n, v in params[net].items()}
        h = torch.relu(onets.lin(t64(x), p, "fc1"))
        h = torch.relu(onets.lin(h, p, "fc2"))
        if is_sac(kind):
            raw = onets.lin(h, p, "fc_scale")
            u = onets.lin(h, p, "fc_prob") + t64(e) * torch.exp(torch.clamp(raw, -20, 2))
            out.append((u.numpy(), raw.numpy()))
        else:
            out.append((onets.lin(h, p, "fc3").numpy(), None))
    return out


def census(name, params=None, edge=True):
    """Per actor-output column, the fraction of samples (of both forwards of pre_tanh) in each regime.  Keys (arrays
    [aout]): above / below (raw log_std > 2 / < -20, SAC only), u10 (10 < |u| <= 44.4: softplus(-2u) takes its
    threshold branch or underflows), u44 (|u| > 44.4: expf(2u) overflows), sat (1 - t * t == 0 with the fp32 tanh);
    plus the ranges umin / umax and rawmin / rawmax."""
    fw = pre_tanh(name, params, edge)
    u = np.concatenate([f[0] for f in fw])
    t32 = np.tanh(u.astype(np.float32))
    out = {"u10": np.mean((np.abs(u) > 10) & (np.abs(u) <= 44.4), axis=0), "u44": np.mean(np.abs(u) > 44.4, axis=0),
           "sat": np.mean(np.float32(1) - t32 * t32 == 0, axis=0), "umin": u.min(axis=0), "umax": u.max(axis=0)}
    if fw[0][1] is not None:
        raw = np.concatenate([f[1] for f in fw])
        out.update(above=np.mean(raw > 2, axis=0), below=np.mean(raw < -20, axis=0), rawmin=raw.min(axis=0),
                   rawmax=raw.max(axis=0))
    return out


def assert_census(name, c):
    """Every regime of the design is populated in this case (asserted per shape: a GPU case cannot hide behind a
    badly chosen input).  The straddling columns are weighed together: 1.9 + 4 w.h is a random column each, and
    with a dozen of them (Ant) one or two stay on one side; over all of them at least 10 % of the samples lie
    on each side of 2, and at least one column has 10 % on each side by itself."""
    kind, _, (ob, aout, ac), B, _, _ = CASES[name]
    j = np.arange(aout)
    assert c["u10"].max() > 0 and c["u44"].max() > 0 and c["sat"].max() > 0, name
    assert c["sat"].min() == 0, name  # and some column never saturates
    assert c["umax"].max() > 44.4, name
    if aout > 6:
        assert c["umin"].min() < -44.4, name  # (MU_BIAS[6]; the 6-dim vanilla actors end at +50)
    if is_sac(kind):
        assert np.all(c["above"][j % 5 == 0] == 1), name
        assert np.all(c["below"][j % 5 == 1] == 1), name
        mid = (j % 5 == 2) | (j % 5 == 4)
        assert np.all(c["above"][mid] == 0) and np.all(c["below"][mid] == 0), name
        st = c["above"][j % 5 == 3]
        assert st.size and 0.1 <= st.mean() <= 0.9, (name, st)
        assert np.any((st >= 0.1) & (st <= 0.9)), (name, st)
