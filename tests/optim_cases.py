"""Inputs and CPU oracles of the persistent-kernel optimizer-state tests (tests/test_gpu_optim.py section 3),
importable without a GPU so that the tolerance inputs can be measured on the CPU (tests/test_adam_ref.py).

A case is a sequence of Adam steps on one network, cut into three segments that the GPU test runs as
K1 per-step steps, ONE persistent launch, K3 per-step steps:
  acm      AcM(22 -> 64 -> 32 -> 3) regression (Hopper dims), sppAcmSgd / sppAcmSgdEpoch; the learning rate
           changes between the first and the second segment
  critic   on-policy critic (17 -> 64 -> 64 -> 1), sppOnpCriticSteps: the launch's steps share their rows
  actor    on-policy PPO actor (17 -> 64 -> 64 -> 17), sppOnpActorEpoch: one launch is one epoch over the pool's
           N rows, so its step count is ceil(N / mb), not K2
Two input columns are zero in every row, and the last output's limit is 0 (AcM, actor): the gradient of those
fc1.weight columns, of the last fc3.weight row and of the last fc3.bias entry (the tail of the flat buffer)
is exactly +-0 in every implementation.  Those entries ("probes") start from non-zero moments; every other
moment starts at zero.
"""
import numpy as np
import torch

from oracle import nets as onets
from oracle import onpolicy as oo
from oracle.acm import OracleAcmTrainer
from oracle.adam import adam_steps_f32, adam_steps_f64
from weights import fill_params

K1, K2, K3 = 3, 4, 2
ZERO_COLS = (3, 9)
OB = 17          # on-policy nets (HalfCheetah)
ACM_OB, ACM_AC = 11, 3  # AcM (Hopper)
ENT = 0.01

# name: (kind, rows per step, rows of the persistent launch's last step or None, pool rows (actor))
CASES = {
    "acm_sgd_bs64": ("acm", 64, None, None),        # one workgroup
    "acm_sgd_bs129": ("acm", 129, None, None),      # 3 workgroups
    "acm_sgd_bs321": ("acm", 321, None, None),      # 6 workgroups
    "acm_epoch_bs129_last2": ("acm", 129, 2, None),  # sppAcmSgdEpoch, ragged last batch of 2 rows
    "critic_n50": ("critic", 50, None, None),
    "critic_n300": ("critic", 300, None, None),
    "actor_n300_mb64": ("actor", 64, None, 300),    # 5 steps, the last of 44 rows
    "actor_n300_mb129": ("actor", 129, None, 300),  # 3 steps, the last of 42 rows
}


def layout_of(kind):
    return {"acm": onets.acm_layout(2 * ACM_OB, ACM_AC), "critic": oo.critic_layout(OB),
            "actor": oo.actor_layout(OB, OB)}[kind]


def layer_slices(layout):
    out, o = [], 0
    for name, shape in layout:
        n = int(np.prod(shape))
        out.append((name, slice(o, o + n)))
        o += n
    return out


def probe_index(kind):
    """Flat indices whose gradient is exactly zero in every step of the case."""
    idx = []
    for name, sl in layer_slices(layout_of(kind)):
        shape = dict(layout_of(kind))[name]
        base = np.arange(sl.start, sl.stop).reshape(shape)
        if name == "fc1.weight":
            idx += list(base[:, list(ZERO_COLS)].reshape(-1))
        if kind != "critic" and name == "fc3.weight":
            idx += list(base[-1])
        if kind != "critic" and name == "fc3.bias":
            idx += [base[-1]]
    return np.array(sorted(idx), np.int64)


def limits(kind):
    lim = np.ones(ACM_AC if kind == "acm" else OB, np.float32)
    lim[-1] = 0.0
    return lim


def _rows(rng, kind, n, a0=None):
    if kind == "acm":
        x = (rng.randn(n, 2 * ACM_OB) * 1.2).astype(np.float32)
        x[:, list(ZERO_COLS)] = 0
        return dict(x=x, y=rng.uniform(-1, 1, (n, ACM_AC)).astype(np.float32))
    x = (rng.randn(n, OB) * 1.3).astype(np.float32)
    x[:, list(ZERO_COLS)] = 0
    if kind == "critic":
        return dict(x=x, q=(rng.randn(n) * 0.7).astype(np.float32))
    act = rng.uniform(-1.1, 1.1, (n, OB)).astype(np.float32)
    with torch.no_grad():
        lp = oo.actor_dist(oo._params(a0, oo.actor_layout(OB, OB)), torch.from_numpy(x),
                           torch.from_numpy(limits("actor"))).log_prob(torch.from_numpy(act)).numpy()
    return dict(x=x, act=act, lp_old=(lp + 0.2 * rng.randn(n)).astype(np.float32),
                adv=rng.randn(n).astype(np.float32), nxt=rng.randn(n, OB).astype(np.float32))


def make_case(name):
    """Everything both sides need: initial (p0, m0, v0), the probes, and per segment the list of steps, each
    a dict of row arrays plus its learning rate.  The persistent segment also carries its launch arguments:
    ``pool`` (the arrays handed to the launch) and, for the actor, ``perm``."""
    kind, bs, last, pool_n = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    lay = layout_of(kind)
    n = sum(int(np.prod(s)) for _, s in lay)
    if kind == "acm":
        p0 = onets.flatten({k: torch.from_numpy(v) for k, v in fill_params(lay, 17).items()}).numpy()
        lrs = (1e-3, 5e-4, 5e-4)  # sppAgentSetLr between the first and the second segment
    else:
        p0 = oo.init_flat(lay, 31)
        if kind == "actor":
            p0[:OB] += rng.uniform(-0.3, 0.3, OB).astype(np.float32)
        lrs = (3e-4,) * 3
    probes = probe_index(kind)
    m0, v0 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    m0[probes] = (rng.uniform(0.5e-2, 2e-2, len(probes)) * rng.choice([-1.0, 1.0], len(probes))).astype(np.float32)
    v0[probes] = (2 * m0[probes]) ** 2
    segs = []
    fresh = lambda: _rows(rng, kind, bs, p0)  # noqa: E731
    segs.append(dict(steps=[fresh() for _ in range(K1)], lr=lrs[0]))
    if kind == "acm":
        sizes = [bs] * K2 if last is None else [bs] * (K2 - 1) + [last]
        pool = _rows(rng, kind, sum(sizes))
        cuts = np.cumsum([0] + sizes)
        steps = [{k: v[a:b] for k, v in pool.items()} for a, b in zip(cuts[:-1], cuts[1:])]
        segs.append(dict(steps=steps, lr=lrs[1], pool=pool, nrows=int(cuts[-1]), epoch=last is not None))
    elif kind == "critic":
        pool = fresh()
        segs.append(dict(steps=[pool] * K2, lr=lrs[1], pool=pool))
    else:
        pool = _rows(rng, kind, pool_n, p0)
        perm = rng.permutation(pool_n)
        steps = [{k: v[perm[s:s + bs]] for k, v in pool.items()} for s in range(0, pool_n, bs)]
        segs.append(dict(steps=steps, lr=lrs[1], pool=pool, perm=perm))
    segs.append(dict(steps=[fresh() for _ in range(K3)], lr=lrs[2]))
    return dict(name=name, kind=kind, bs=bs, layout=lay, p0=p0, m0=m0, v0=v0, probes=probes, segs=segs,
                lim=limits(kind))


def gradient(case, flat, rows, dtype):
    """The oracle's gradient of one step at the parameters ``flat``."""
    if case["kind"] == "critic":
        return oo.critic_step(flat, OB, rows["x"], rows["q"], dtype=dtype)[1]
    return oo.actor_step(flat, OB, OB, case["lim"], rows["x"], rows["act"], rows["lp_old"], rows["adv"],
                         entropy_coef=ENT, next_obs=rows["nxt"], dtype=dtype)[1]


def run_oracle(case, dtype=torch.float64):
    """(p, m, v) after each segment, from the oracle in ``dtype`` (float32: torch / numpy float32 throughout)."""
    f64 = dtype == torch.float64
    out = []
    if case["kind"] == "acm":
        params = {k: v.numpy() for k, v in onets.unflatten(case["p0"], case["layout"]).items()}
        o = OracleAcmTrainer(2 * ACM_OB, ACM_AC, lr=1e-3, ac_lim=case["lim"], params=params, dtype=dtype,
                             m=case["m0"], v=case["v0"], t=0)
        for seg in case["segs"]:
            o.opt.lr = float(np.float32(seg["lr"]))
            for rows in seg["steps"]:
                o.batch_update(rows["x"], rows["y"])
                assert not o.last_grad[case["probes"]].any()  # the probes' gradient is exactly zero
            out.append((o.flat().copy(),) + tuple(x.copy() for x in o.moments()))
        return out
    step = adam_steps_f64 if f64 else adam_steps_f32
    p, m, v = (np.array(x, np.float64 if f64 else np.float32) for x in (case["p0"], case["m0"], case["v0"]))
    t = 0
    for seg in case["segs"]:
        for rows in seg["steps"]:
            g = gradient(case, p, rows, dtype)
            assert not g[case["probes"]].any()
            p, m, v, _, t = step(p, m, v, t, [g], seg["lr"])
        out.append((p.copy(), m.copy(), v.copy()))
    return out


def probe_reference(case):
    """(p, m, v) of the probes after each segment: the float32 restatement with a zero gradient."""
    ix = case["probes"]
    p, m, v, t = case["p0"][ix], case["m0"][ix], case["v0"][ix], 0
    z, out = np.zeros(len(ix), np.float32), []
    for seg in case["segs"]:
        p, m, v, _, t = adam_steps_f32(p, m, v, t, [z] * len(seg["steps"]), seg["lr"])
        out.append((p, m, v, t))
    return out


def layer_deviation(a, ref, layout):
    """max over elements of |a - ref| / rms(ref over the element's layer tensor)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    worst = 0.0
    for _, sl in layer_slices(layout):
        rms = np.sqrt(np.mean(ref[sl] ** 2))
        worst = max(worst, float(np.max(np.abs(a[sl] - ref[sl])) / rms))
    return worst


# 8 x the largest layer_deviation of the float32 oracle's m and v from the float64 oracle's over the three
# segments of each case, measured on the CPU (tests/test_adam_ref.py asserts that they still cover it)
TAU_F32 = {
    "acm_sgd_bs64": 2.4e-5, "acm_sgd_bs129": 3.6e-5, "acm_sgd_bs321": 5.2e-5, "acm_epoch_bs129_last2": 2.2e-5,
    "critic_n50": 2.1e-5, "critic_n300": 4.5e-5,
    # (the PPO actor's float32 moments sit ~3e-5 of a layer's rms from float64's, ten times the regressions')
    "actor_n300_mb64": 3.8e-4, "actor_n300_mb129": 5.2e-4,
}
GRAD_TOL = 2e-4  # the project's gradient tolerance


def tau(name):
    return max(GRAD_TOL, TAU_F32[name])
