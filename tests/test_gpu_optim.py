"""Optimizer state on the GPU: what *Apply and the persistent kernels do with a gradient.

Adam exists three times in the library: k_adam (optim.hip, behind every *Apply), the in-register Adam of the
persistent kernels (sgd_mlp.hip: sppAcmSgd, sppAcmSgdEpoch, sppOnpCriticSteps, sppOnpActorEpoch; sharded over
workgroups, beta^t carried as running products from step0) and the float64 temperature step k_alpha_step.
Data-parallel ranks all-reduce the gradient buckets between *Grads and *Apply and rely on Apply being a pure,
deterministic function of (p, m, v, g, step, lr); these tests pin that function down.

1. k_adam, isolated by injecting the gradient (test_apply_*).  *Grads runs on the smallest legal batch
   (B = 32); the caller-owned gradient bucket is then overwritten with a designed gradient, exp_avg / exp_avg_sq
   and the step counters are preset, *Apply runs, and EVERY element of p, m, v and the polyak target is compared.
   Three consecutive Apply calls with a fresh gradient each, sppAgentSetLr(x 0.25, -1 for the other rates) before
   the last, resumed at steps 0, 1, 9, 999 and 100,000 (every counter of a handle starts at another of them).
   Designed gradients (oracle.adam.designed_gradient / designed_state, fixed seeds): magnitudes log-uniform
   in [1e-6, 1e2] with random signs, a block of exact zeros over live moments, a block of zeros over zero
   moments (p must stay bit-unchanged), four entries of +-1e18.  Every intermediate stays in the normal float32
   range: non-zero |g| >= 1e-6 (>= 1e-15 required), non-zero v0 >= 1e-12 (>= 1e-30 required), g^2 <= 1e36.
     (a) bit equality with the float32 restatement oracle.adam.adam_steps_f32 (one rounding per operation, the
         kernel's stated order; torch.optim.Adam on the CPU is NOT that reference: it differs in tens of thousands
         of m / v entries of 200,000 by step 2);
     (b) |gpu - float64| / scale <= 4 x the largest such error of the float32 restatement on the same inputs,
         computed here on the CPU (<= 6.5e-7 at 1e5 elements, tests/test_adam_ref.py), scales s_p = max(|p0|, K lr),
         s_m = max(|m0|, max_k |g_k|), s_v = max(s_m^2, v_ref), target: max(|target0|, s_p);
     (c) sppAgentGetSteps advanced by exactly one per Apply on the right counter(s);
     (d) every network, moment and target outside the applied bucket bit-unchanged.
   Handles: SAC_AcM Hopper fp32 and mlp_bf16 (critic bucket = two jobs with polyak, actor, ACM; every packed image
   afterwards = the new parameters, RNE bf16 of them for the bf16 agent), DDPG_AcM HalfCheetah (critic with polyak,
   actor with polyak of the ACTOR target, BasicAcM), vanilla SAC HalfCheetah, OnPolicyNets critic and actor (no
   step setter: the step is reached by running Apply with a zero gradient over zero moments, which moves nothing).
   Bit equality (a) held everywhere when written.
   The reference fixture's own moments (sac_hopper_paper: m_actor, v_actor, m_critic_1, v_critic_1 after two
   updates) are compared with the GPU's exp_avg / exp_avg_sq: |d| <= tau x rms(layer tensor), tau = 2e-4 (8 x
   the float32 oracle's deviation from the float64 oracle on that case is 7.3e-5, below the gradient tolerance).
2. The temperature step (test_alpha_*): alpha_state = {log_alpha, m, v, alpha} and the alpha step counter
   preset, the bound alpha-gradient scalar overwritten with c after sppSacAcmActorGrads (what a data-parallel
   caller's all-reduce does), against Python float64: log_alpha, m, v, alpha rel 1e-12 (a dozen float64
   operations with libm pow / exp / sqrt at a few ulp: ~1e-14), alpha_f32 and losses[6] within one float32
   ulp of float32(exp(log_alpha_gpu)), losses[5] = float32(exp(log_alpha) c).
3. The persistent kernels (test_persistent_*): K1 = 3 per-step steps, ONE persistent launch (K2 = 4 steps; an
   actor epoch over N = 300 rows is ceil(N / mb) = 5 or 3 steps), K3 = 2 per-step steps on one handle, the AcM
   with sppAgentSetLr between the first and second segment, against the float64 oracle over the same steps
   (tests/optim_cases.py).  After EACH segment:
     - exact probes: two input columns are zero in every row and the last output's limit is 0, so the gradient
       of those fc1.weight columns, the last fc3.weight row and the flat buffer's last element is exactly +-0;
       they start from non-zero moments.  m and v there are bit-equal to the float32 restatement through all the
       steps; p within (steps so far) ulp (the kernel carries beta^t as products: each of its two scalars may
       differ from pow's by one float32 ulp);
     - every element: |m - m_ref| <= tau x rms(m_ref over its layer tensor), likewise v: no share left out, so a
       slot no shard owns, or moments not stored back, fail.  tau = max(2e-4 (the gradient tolerance), 8 x the
       float32 oracle's largest such deviation from the float64 oracle), measured on the CPU
       (optim_cases.TAU_F32): 2.4e-5 / 3.6e-5 / 5.2e-5 / 2.2e-5 (AcM bs 64 / 129 / 321 / epoch), 2.1e-5 / 4.5e-5
       (critic N 50 / 300), 3.8e-4 / 5.2e-4 (actor mb 64 / 129), so tau = 2e-4 except for the two actor cases;
     - parameters: |d| <= 2 lr per step, mean |d| <= 0.01 lr (near-zero gradient coordinates may flip);
     - hand-off: the moments read right after the persistent launch satisfy the bound (stored back, not only
       consumed by the next launch); the AcM step counter ends at K1 + K2 + K3; the timeout flag stays clear;
     - same state, two paths: a second handle reaches the launch's start (p, m, v, step) by the same per-step
       steps (bit-identical: two handles on the same inputs agree exactly) and runs the launch's steps per-step;
       m and v of the two paths agree within tau per element.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import spprl  # noqa: E402
from spprl import _lib  # noqa: E402
from spprl.onpolicy import OnPolicyNets  # noqa: E402
import optim_cases as oc  # noqa: E402
from golden_cases import sac_case  # noqa: E402
from oracle.adam import adam_scales, adam_steps_f32, adam_steps_f64, designed_gradient, designed_state  # noqa: E402
from test_gpu_bigbatch import DDPG_NETS, SAC_NETS, random_batch, set_minmax  # noqa: E402
from test_gpu_multistep import check_images  # noqa: E402

DEV = torch.device("cuda:0")
T0S = [0, 1, 9, 999, 100000]
B = 32  # the smallest legal batch: one 32-row tile
ST = _lib.stream_handle
A, C1, C2, C1T, C2T, ACM, AT = (_lib.SPP_NET_ACTOR, _lib.SPP_NET_CRITIC1, _lib.SPP_NET_CRITIC2,
                                _lib.SPP_NET_CRITIC1_TARG, _lib.SPP_NET_CRITIC2_TARG, _lib.SPP_NET_ACM,
                                _lib.SPP_NET_ACTOR_TARG)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def host(t):
    return t.detach().cpu().numpy().copy()


def put(t, a):
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))


def get_steps(h):
    s = np.zeros(4, np.int64)
    _lib.call("sppAgentGetSteps", h, s.ctypes.data_as(ctypes.c_void_p))
    return [int(x) for x in s]


# ------------------------------------------------------------------ 1. k_adam behind *Apply
class Job:
    """One Adam job of a bucket: parameter / gradient / moment tensors, the polyak target (or None), and the
    reference state it started from with the gradients and rates applied so far."""

    def __init__(self, name, p, g, m, v, targ, tau):
        self.name, self.p, self.g, self.m, self.v, self.targ, self.tau = name, p, g, m, v, targ, tau

    def preset(self, rng, t0):
        n = self.p.numel()
        _, m0, v0 = designed_state(rng, n)
        put(self.m, m0)
        put(self.v, v0)
        self.n, self.t0, self.grads, self.lrs = n, t0, [], []
        self.p0, self.m0, self.v0 = host(self.p), m0, v0
        self.tg0 = None if self.targ is None else host(self.targ)

    def inject(self, rng, lr):
        g = designed_gradient(rng, self.n)
        put(self.g, g)
        self.grads.append(g)
        self.lrs.append(lr)

    def check(self):
        tau = None if self.targ is None else self.tau
        r32 = adam_steps_f32(self.p0, self.m0, self.v0, self.t0, self.grads, self.lrs, self.tg0, tau)
        r64 = adam_steps_f64(self.p0, self.m0, self.v0, self.t0, self.grads, self.lrs, self.tg0, tau)
        got = [host(self.p), host(self.m), host(self.v), None if self.targ is None else host(self.targ)]
        s_p, s_m, s_v = adam_scales(self.p0, self.m0, self.grads, self.lrs, r64[2])
        scales = [s_p, s_m, s_v, None if self.targ is None else np.maximum(np.abs(self.tg0.astype(np.float64)), s_p)]
        K = len(self.grads)
        for what, x, a32, a64, s in zip(("p", "m", "v", "target"), got, r32, r64, scales):
            if x is None:
                continue
            assert np.isfinite(x).all(), (self.name, what, K)
            # (b) float64 bound from the float32 restatement's own error, never from the GPU output
            bound = 4 * float(np.max(np.abs(a32.astype(np.float64) - a64) / s))
            err = float(np.max(np.abs(x.astype(np.float64) - a64) / s))
            # (a) bit equality with the float32 restatement
            bad = np.flatnonzero(bits(x) != bits(a32))
            print("%s %s after %d steps from t0 %d: %d of %d differ from the fp32 restatement; normalised error "
                  "to float64 %.2e (bound %.2e)" % (self.name, what, K, self.t0, len(bad), len(x), err, bound))
            assert err <= bound, (self.name, what, K, err, bound)
            assert len(bad) == 0, "%s %s step %d: %d of %d elements differ from the fp32 restatement, first %d: " \
                "gpu %r ref %r" % (self.name, what, K, len(bad), len(x), bad[0], x[bad[0]], a32[bad[0]])
        z = slice(self.n // 8, self.n // 4)  # g = m0 = v0 = 0: nothing may move
        assert (bits(got[0][z]) == bits(self.p0[z])).all() and not got[1][z].any() and not got[2][z].any(), self.name


def frozen(tensors, skip):
    return {k: t.clone() for k, t in tensors.items() if not any(t.data_ptr() == s.data_ptr() for s in skip)}


def assert_frozen(tensors, snap, who):
    for k, t in snap.items():
        assert torch.equal(tensors[k].view(torch.int32), t.view(torch.int32)), "%s changed %s" % (who, k)


def run_buckets(h, buckets, everything, i_t0, lr0, set_steps=True):
    """buckets: [dict(name, jobs, ctr (counters that advance), slot (sppAgentSetLr argument), grads(), apply())].
    everything: {name: tensor} of all parameters, targets and moments of the handle.
    Counter k starts at T0S[(i_t0 + k) % 5]: every bucket meets every resume step over the five cases, and a
    bucket stepping with another's counter shows."""
    rng = np.random.RandomState(4000 + i_t0)
    start = [T0S[(i_t0 + k) % 5] for k in range(4)]
    _lib.call("sppAgentSetSteps", h, *start)
    _lib.call("sppAgentSetLr", h, *[float(x) for x in lr0])
    lr = list(lr0)
    for b in buckets:
        for j in b["jobs"]:
            j.preset(rng, start[b["ctr"][0]])
    for r in range(3):
        for b in buckets:
            if r == 2:  # a rate change before the last Apply; -1 keeps the other rates
                lr[b["slot"]] = lr0[b["slot"]] * 0.25
                _lib.call("sppAgentSetLr", h, *[lr[b["slot"]] if k == b["slot"] else -1.0 for k in range(4)])
            b["grads"]()  # the library's own gradients of a B = 32 batch ...
            for j in b["jobs"]:
                j.inject(rng, lr[b["slot"]])  # ... replaced, as a caller's all-reduce does in place
            mine = [t for j in b["jobs"] for t in (j.p, j.m, j.v, j.targ) if t is not None]
            snap = frozen(everything, mine)
            s0 = get_steps(h)
            b["apply"]()
            torch.cuda.synchronize()
            want = [s + (1 if k in b["ctr"] else 0) for k, s in enumerate(s0)]
            assert get_steps(h) == want, (b["name"], s0, get_steps(h))  # (c)
            assert_frozen(everything, snap, b["name"])  # (d)
            for j in b["jobs"]:
                j.check()
    assert get_steps(h) == [s + 3 * sum(k in b["ctr"] for b in buckets) for k, s in enumerate(start)]


def agent_tensors(ag):
    out = {"p%d" % k: t for k, t in ag.params.items()}
    out.update({"m%d" % k: t for k, t in ag.exp_avg.items()})
    out.update({"v%d" % k: t for k, t in ag.exp_avg_sq.items()})
    return out


def job(ag, name, net, targ=None, tau=None):
    return Job(name, ag.params[net], ag.grads[net], ag.exp_avg[net], ag.exp_avg_sq[net],
               None if targ is None else ag.params[targ], tau)


def acm_bucket(ag, rng, ob, ac):
    keep = {}

    def grads():
        keep["x"] = torch.from_numpy((rng.randn(B, 2 * ob) * 1.2).astype(np.float32)).to(DEV)
        keep["y"] = torch.from_numpy(rng.uniform(-1, 1, (B, ac)).astype(np.float32)).to(DEV)
        keep["l"] = torch.zeros(1, device=DEV)
        _lib.call("sppAcmRegressGrads", ag._h, _lib.ptr(keep["x"]), _lib.ptr(keep["y"]), B, _lib.ptr(keep["l"]), ST())

    return dict(name="acm", jobs=[job(ag, "acm", ACM)], ctr=[3], slot=3, grads=grads,
                apply=lambda: _lib.call("sppAcmRegressApply", ag._h, ST()))


def sac_buckets(ag, ob, aout, ac, vanilla=False):
    rng = np.random.RandomState(77)
    keep = {}

    def critic_grads():
        batch = random_batch(rng, B, ob, aout, ac)
        if vanilla:  # SAC.update: the env action is the critics' action input
            batch = batch[:5] + (batch[2],)
        b, keep["batch"] = ag._batch(*batch)
        keep["e1"], keep["e2"] = torch.randn(B, aout, device=DEV), torch.randn(B, aout, device=DEV)
        _lib.call("sppSacAcmCriticGrads", ag._h, ctypes.byref(b), _lib.ptr(keep["e1"]), _lib.ptr(ag._losses), ST())

    def actor_grads():
        _lib.call("sppSacAcmActorGrads", ag._h, _lib.ptr(keep["e2"]), _lib.ptr(ag._losses), ST())
        ag.alpha_grad.fill_(0.25)  # (the temperature step has its own test; kept finite here)

    tau = ag.tau
    out = [dict(name="critic", jobs=[job(ag, "critic_1", C1, C1T, tau), job(ag, "critic_2", C2, C2T, tau)], ctr=[1],
                slot=1, grads=critic_grads, apply=lambda: _lib.call("sppSacAcmCriticApply", ag._h, ST())),
           dict(name="actor", jobs=[job(ag, "actor", A)], ctr=[0, 2], slot=0, grads=actor_grads,
                apply=lambda: _lib.call("sppSacAcmActorApply", ag._h, _lib.ptr(ag._losses), ST()))]
    if not vanilla:
        out.append(acm_bucket(ag, rng, ob, ac))
    return out, critic_grads


_AGENTS = {}


def sac_agent(kind):
    """One handle per kind for the five resume-step cases: Apply is a pure function of the preset state."""
    if kind not in _AGENTS:
        if kind == "vanilla":
            ag = spprl.SAC(env_name="HalfCheetah-v2", max_batch=B, buffer_size=64, device=DEV, seed=3)
        else:
            ag = spprl.SAC_AcM(env_name="Hopper-v2", acm_critic=True, custom_loss=0.2, norm_closs=False,
                               min_max_denormalize=True, denormalize_actor_out=True, gamma=0.99, max_batch=B,
                               buffer_size=64, device=DEV, seed=5, mlp_bf16=kind == "bf16")
            set_minmax(ag, np.random.RandomState(1), 11)
        _AGENTS[kind] = ag
    return _AGENTS[kind]


@pytest.mark.parametrize("i_t0", range(5))
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_apply_sac_acm_hopper(kind, i_t0):
    ag = sac_agent(kind)
    buckets, critic_grads = sac_buckets(ag, 11, 11, 3)
    run_buckets(ag._h, buckets, agent_tensors(ag), i_t0, (1e-3, 5e-4, 3e-4, 2e-3))
    # every packed image = the NEW parameters (bf16 agents: RNE bf16 of them): the next update's first phase packs
    # them all from the fp32 master weights
    critic_grads()
    torch.cuda.synchronize()
    assert check_images(ag, kind == "bf16", {k: ag.params[net] for k, net in SAC_NETS.items()}) > 0


@pytest.mark.parametrize("i_t0", range(5))
def test_apply_vanilla_sac_hcheetah(i_t0):
    ag = sac_agent("vanilla")
    buckets, _ = sac_buckets(ag, 17, 6, 6, vanilla=True)
    run_buckets(ag._h, buckets, agent_tensors(ag), i_t0, (1e-3, 5e-4, 3e-4, 2e-3))


@pytest.mark.parametrize("i_t0", range(5))
def test_apply_ddpg_acm_hcheetah_polyak_of_both_targets(i_t0):
    if "ddpg" not in _AGENTS:
        ag = spprl.DDPG_AcM(env_name="HalfCheetah-v2", gamma=0.99, actor_lr=5e-4, critic_lr=1e-3, tau=0.02,
                            acm_critic=True, custom_loss=1.0, norm_closs=False, min_max_denormalize=True,
                            denormalize_actor_out=True, max_batch=B, buffer_size=64, device=DEV, seed=9)
        set_minmax(ag, np.random.RandomState(2), 17)
        _AGENTS["ddpg"] = ag
    ag = _AGENTS["ddpg"]
    ob, ac = 17, 6
    rng = np.random.RandomState(78)
    keep = {}

    def critic_grads():
        keep["t"] = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in random_batch(rng, B, ob, ob, ac)]
        b = _lib.Batch(B, *[_lib.ptr(x) for x in keep["t"]])
        _lib.call("sppDdpgAcmCriticGrads", ag._h, ctypes.byref(b), _lib.ptr(ag._losses), ST())

    buckets = [dict(name="critic", jobs=[job(ag, "critic", C1, C1T, ag.tau)], ctr=[1], slot=1, grads=critic_grads,
                    apply=lambda: _lib.call("sppDdpgAcmCriticApply", ag._h, ST())),
               dict(name="actor", jobs=[job(ag, "actor", A, AT, ag.tau)], ctr=[0], slot=0,
                    grads=lambda: _lib.call("sppDdpgAcmActorGrads", ag._h, _lib.ptr(ag._losses), ST()),
                    apply=lambda: _lib.call("sppDdpgAcmActorApply", ag._h, ST())),
               acm_bucket(ag, rng, ob, ac)]
    assert set(DDPG_NETS.values()) == set(ag.params)
    run_buckets(ag._h, buckets, agent_tensors(ag), i_t0, (5e-4, 1e-3, 0.0, 2e-3))


@pytest.mark.parametrize("t0", T0S)
@pytest.mark.parametrize("net", [1, 0], ids=["critic", "actor"])
def test_apply_onpolicy_nets(net, t0):
    """sppOnpCriticGrads / Apply and sppOnpActorGrads / Apply (ob 17).  The handle has no step setter: t0 Apply calls
    with a zero gradient over zero moments reach the step (0 / (0 + eps) = 0: the parameters must not move)."""
    lrs = (3e-3, 3e-4)  # actor, critic
    n = OnPolicyNets(17, 17, ac_lim=1.0, actor_lr=lrs[0], critic_lr=lrs[1], entropy_coef=0.01, max_batch=B,
                     device=DEV, seed=11)
    rng = np.random.RandomState(500 + net)
    keep = {}

    def grads():
        x = torch.from_numpy((rng.randn(B, 17) * 1.2).astype(np.float32)).to(DEV)
        if net == 1:
            keep["t"] = (x, torch.from_numpy(rng.randn(B).astype(np.float32)).to(DEV), torch.zeros(1, device=DEV))
            _lib.call("sppOnpCriticGrads", n._h, _lib.ptr(x), _lib.ptr(keep["t"][1]), B, _lib.ptr(keep["t"][2]), ST())
        else:
            act = torch.from_numpy(rng.uniform(-1, 1, (B, 17)).astype(np.float32)).to(DEV)
            lp = torch.from_numpy((rng.randn(B) - 10).astype(np.float32)).to(DEV)
            adv = torch.from_numpy(rng.randn(B).astype(np.float32)).to(DEV)
            keep["t"] = (x, act, lp, adv, torch.empty(4, device=DEV))
            _lib.call("sppOnpActorGrads", n._h, _lib.ptr(x), _lib.ptr(act), _lib.ptr(lp), _lib.ptr(adv), None, B,
                      _lib.ptr(keep["t"][4]), ST())

    apply = "sppOnpCriticApply" if net == 1 else "sppOnpActorApply"
    grads()
    n.grads[net].zero_()
    p_start = n.params[net].clone()
    st = ST()
    for _ in range(t0):
        _lib.call(apply, n._h, st)
    torch.cuda.synchronize()
    assert torch.equal(n.params[net].view(torch.int32), p_start.view(torch.int32))
    assert not n.m[net].any() and not n.v[net].any()
    j = Job("onp_" + ("critic" if net == 1 else "actor"), n.params[net], n.grads[net], n.m[net], n.v[net], None, None)
    j.preset(rng, t0)
    other = 1 - net
    snap = [t.clone() for t in (n.params[other], n.m[other], n.v[other])]
    for _ in range(3):
        grads()
        j.inject(rng, lrs[net])
        _lib.call(apply, n._h, ST())
        torch.cuda.synchronize()
        j.check()
    for a, b in zip(snap, (n.params[other], n.m[other], n.v[other])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_fixture_moments_match_gpu_exp_avg():
    """The reference's own Adam moments after the sac_hopper_paper fixture's two updates against the GPU's."""
    from test_gpu_parity import build_agent

    cfg, fx, params, layouts, norm, steps = sac_case("sac_hopper_paper")
    assert "m_actor" in fx and "v_critic_1" in fx
    ag, names = build_agent(cfg, fx, params, norm, int(fx["dims"][3]))
    for batch, e1, e2 in steps:
        ag.update(*batch, eps_next=e1, eps_cur=e2)
    torch.cuda.synchronize()
    assert get_steps(ag._h)[:3] == [len(steps)] * 3
    tau = 2e-4
    for k in ("actor", "critic_1"):
        for mv, t in (("m", ag.exp_avg), ("v", ag.exp_avg_sq)):
            d = oc.layer_deviation(host(t[names[k]]), fx["%s_%s" % (mv, k)], layouts[k])
            print("%s_%s: max |d| / rms(layer) %.2e" % (mv, k, d))
            assert d <= tau, (k, mv, d)


# ------------------------------------------------------------------ 2. the temperature step
def alpha_ref(la, m, v, t, c, lr):
    g = math.exp(la) * c
    m = m + (1.0 - 0.9) * (g - m)
    v = v * 0.999 + (1.0 - 0.999) * g * g
    bc1, bc2s = 1.0 - 0.9 ** t, math.sqrt(1.0 - 0.999 ** t)
    nla = la - (lr / bc1) * (m / (math.sqrt(v) / bc2s + 1e-8))
    return nla, m, v, math.exp(nla), g


@pytest.mark.parametrize("t0", [0, 9, 100000])
def test_alpha_step_matches_float64(t0):
    ag = sac_agent("fp32")
    _, critic_grads = sac_buckets(ag, 11, 11, 3)
    e2 = torch.randn(B, 11, device=DEV)
    cases = [(0.37, math.log(0.2), 0.0, 0.0, 3e-4), (-1.9, math.log(0.2), 0.0, 0.0, 3e-4), (0.0, -0.7, 0.0, 0.0, 3e-4),
             (0.0, -0.7, 0.03, 0.002, 3e-4), (2.5, 0.4, -0.2, 0.09, 1e-3), (-0.011, -2.3, 0.004, 1e-5, 1e-3)]
    for c, la, m, v, lr in cases:
        c = float(np.float32(c))
        ag.alpha_state.copy_(torch.tensor([la, m, v, math.exp(la)], dtype=torch.float64))
        ag.set_steps(actor=5, critic=6, alpha=t0, acm=7)
        _lib.call("sppAgentSetLr", ag._h, -1.0, -1.0, lr, -1.0)
        critic_grads()
        _lib.call("sppSacAcmActorGrads", ag._h, _lib.ptr(e2), _lib.ptr(ag._losses), ST())
        ag.alpha_grad.fill_(c)  # the all-reduced operand
        _lib.call("sppSacAcmActorApply", ag._h, _lib.ptr(ag._losses), ST())
        torch.cuda.synchronize()
        assert get_steps(ag._h) == [6, 6, t0 + 1, 7]
        got = ag.alpha_state.cpu().numpy()
        want = alpha_ref(la, m, v, t0 + 1, c, float(np.float32(lr)))
        for name, x, w in zip(("log_alpha", "m", "v", "alpha"), got, want):
            assert abs(x - w) <= 1e-12 * abs(w), (name, t0, c, x, w)
        if c == 0.0 and m == 0.0:
            assert got[0] == la and got[1] == 0.0 and got[2] == 0.0
        a32 = np.float32(math.exp(got[0]))
        losses = host(ag._losses)
        for x in (host(ag.alpha_f32)[0], losses[6]):
            assert abs(float(x) - float(a32)) <= float(np.spacing(a32)), (t0, c, x, a32)
        assert losses[5] == np.float32(want[4]), (t0, c, losses[5], want[4])


# ------------------------------------------------------------------ 3. the persistent kernels
class AcmHandle:
    def __init__(self, case):
        self.ag = spprl.SAC_AcM(env_name="Hopper-v2", acm_lr=case["segs"][0]["lr"], max_batch=512, buffer_size=64,
                                device=DEV, seed=1)
        a_lim = np.ones(oc.ACM_OB, np.float32)
        _lib.call("sppAgentSetLimits", self.ag._h, a_lim.ctypes.data_as(ctypes.c_void_p),
                  case["lim"].ctypes.data_as(ctypes.c_void_p))
        self.p, self.m, self.v = self.ag.params[ACM], self.ag.exp_avg[ACM], self.ag.exp_avg_sq[ACM]
        self.keep = []

    def set_lr(self, lr):
        _lib.call("sppAgentSetLr", self.ag._h, -1.0, -1.0, -1.0, float(lr))

    def step(self, rows):
        x, y = (torch.from_numpy(np.ascontiguousarray(rows[k])).to(DEV) for k in ("x", "y"))
        loss = torch.zeros(1, device=DEV)
        self.keep.append((x, y, loss))
        _lib.call("sppAcmRegressGrads", self.ag._h, _lib.ptr(x), _lib.ptr(y), x.shape[0], _lib.ptr(loss), ST())
        _lib.call("sppAcmRegressApply", self.ag._h, ST())

    def launch(self, case, seg):
        x, y = (torch.from_numpy(seg["pool"][k]).to(DEV) for k in ("x", "y"))
        loss = torch.zeros(1, device=DEV)
        self.keep.append((x, y, loss))
        if seg["epoch"]:
            _lib.call("sppAcmSgdEpoch", self.ag._h, _lib.ptr(x), _lib.ptr(y), seg["nrows"], case["bs"], _lib.ptr(loss),
                      ST())
        else:
            _lib.call("sppAcmSgd", self.ag._h, _lib.ptr(x), _lib.ptr(y), len(seg["steps"]), case["bs"], _lib.ptr(loss),
                      ST())

    def finish(self, nsteps):
        assert get_steps(self.ag._h)[3] == nsteps
        flag = np.ones(1, np.int32)
        _lib.call("sppAcmSgdStatus", self.ag._h, flag.ctypes.data)
        assert flag[0] == 0


class OnpHandle:
    def __init__(self, case):
        lr = case["segs"][0]["lr"]
        self.net = 1 if case["kind"] == "critic" else 0
        self.n = OnPolicyNets(oc.OB, oc.OB, ac_lim=case["lim"], actor_lr=lr, critic_lr=lr, entropy_coef=oc.ENT,
                              max_batch=512, device=DEV, seed=2)
        self.p, self.m, self.v = self.n.params[self.net], self.n.m[self.net], self.n.v[self.net]
        self.keep = []

    def set_lr(self, lr):
        pass  # (one rate throughout: the handle has no setter)

    def step(self, rows):
        if self.net == 1:
            self.n.critic_step(rows["x"], rows["q"])
        else:
            self.n.actor_step(rows["x"], rows["act"], rows["lp_old"], rows["adv"], rows["nxt"])

    def launch(self, case, seg):
        n, pool = self.n, {k: torch.from_numpy(v).to(DEV) for k, v in seg["pool"].items()}
        N = pool["x"].shape[0]
        if self.net == 1:
            out = torch.zeros(1, device=DEV)
            _lib.call("sppOnpCriticSteps", n._h, _lib.ptr(pool["x"]), _lib.ptr(pool["q"]), N, len(seg["steps"]),
                      _lib.ptr(out), ST())
        else:
            pool["perm"] = torch.from_numpy(seg["perm"].astype(np.int64)).to(DEV)
            out = torch.empty(len(seg["steps"]), 4, device=DEV)
            _lib.call("sppOnpActorEpoch", n._h, _lib.ptr(pool["x"]), _lib.ptr(pool["act"]), _lib.ptr(pool["lp_old"]),
                      _lib.ptr(pool["adv"]), _lib.ptr(pool["nxt"]), _lib.ptr(pool["perm"]), N, case["bs"],
                      _lib.ptr(out), ST())
        self.keep.append((pool, out))

    def finish(self, nsteps):
        self.n.check_actor_epochs()  # (the shared timeout flag of the persistent launches)


def load_state(hd, p, m, v):
    put(hd.p, p)
    put(hd.m, m)
    put(hd.v, v)


def within_tau(got, ref, rms_ref, layout, tau, what):
    """|got - ref| <= tau x rms(rms_ref over the layer), for EVERY element."""
    worst = 0.0
    for name, sl in oc.layer_slices(layout):
        rms = np.sqrt(np.mean(np.asarray(rms_ref[sl], np.float64) ** 2))
        d = np.abs(np.asarray(got[sl], np.float64) - np.asarray(ref[sl], np.float64)) / rms
        worst = max(worst, float(d.max()))
        assert d.max() <= tau, "%s %s: element %d is %.3g x rms(layer) off (tau %.1e); gpu %r ref %r" % (
            what, name, sl.start + int(d.argmax()), d.max(), tau, got[sl][d.argmax()], ref[sl][d.argmax()])
    return worst


@pytest.mark.parametrize("name", list(oc.CASES))
def test_persistent_kernel_resumes_hands_off_and_covers_every_shard(name):
    case = oc.make_case(name)
    tau, lay, ix = oc.tau(name), case["layout"], case["probes"]
    ref = oc.run_oracle(case, torch.float64)
    pref = oc.probe_reference(case)
    make = AcmHandle if case["kind"] == "acm" else OnpHandle
    hd, twin = make(case), make(case)  # (twin: the per-step path from the launch's start state)
    for h in (hd, twin):
        load_state(h, case["p0"], case["m0"], case["v0"])
    lr_max = max(s["lr"] for s in case["segs"])
    nsteps, snap, launched = 0, None, None
    for s, seg in enumerate(case["segs"]):
        hd.set_lr(seg["lr"])
        if s == 1:
            torch.cuda.synchronize()
            snap = (host(hd.p), host(hd.m), host(hd.v))
            hd.launch(case, seg)  # ONE persistent launch
        else:
            for rows in seg["steps"]:
                hd.step(rows)
        torch.cuda.synchronize()
        nsteps += len(seg["steps"])
        p, m, v = host(hd.p), host(hd.m), host(hd.v)  # (s == 1: straight after the launch: stored back)
        if s == 1:
            launched = (m, v)
        assert all(np.isfinite(x).all() for x in (p, m, v)), (name, s)
        # exact probes
        pp, pm, pv, pt = pref[s]
        assert pt == nsteps
        assert (bits(m[ix]) == bits(pm)).all(), (name, s, "m", int((bits(m[ix]) != bits(pm)).sum()))
        assert (bits(v[ix]) == bits(pv)).all(), (name, s, "v", int((bits(v[ix]) != bits(pv)).sum()))
        ulps = np.abs(p[ix].astype(np.float64) - pp) / np.spacing(np.abs(pp))
        assert ulps.max() <= nsteps, (name, s, "p", ulps.max())
        # every element
        rp, rm, rv = ref[s]
        wm = within_tau(m, rm, rm, lay, tau, "%s segment %d m" % (name, s))
        wv = within_tau(v, rv, rv, lay, tau, "%s segment %d v" % (name, s))
        # parameters
        d = np.abs(p.astype(np.float64) - rp)
        print("%s after segment %d (%d steps): probes exact, p within %.0f ulp; max |d| / rms(layer) m %.2e v %.2e "
              "(tau %.1e); |dp| / lr max %.4f mean %.6f" % (name, s, nsteps, ulps.max(), wm, wv, tau, d.max() / lr_max,
                                                            d.mean() / lr_max))
        assert d.max() <= 2 * lr_max * nsteps * 1.01 and d.mean() <= 0.01 * lr_max, (name, s, d.max(), d.mean())
    hd.finish(nsteps)
    # same state, two paths: the twin reaches the launch's start per-step, takes the same (p, m, v), and runs the
    # launch's steps one at a time
    twin.set_lr(case["segs"][0]["lr"])
    for rows in case["segs"][0]["steps"]:
        twin.step(rows)
    torch.cuda.synchronize()
    for x, y in zip(snap, (twin.p, twin.m, twin.v)):  # the per-step path is deterministic: replicated ranks agree
        assert (bits(x) == bits(host(y))).all(), name
    twin.set_lr(case["segs"][1]["lr"])
    for rows in case["segs"][1]["steps"]:
        twin.step(rows)
    torch.cuda.synchronize()
    rm, rv = ref[1][1], ref[1][2]
    wm = within_tau(launched[0], host(twin.m), rm, lay, tau, "%s two paths m" % name)
    wv = within_tau(launched[1], host(twin.v), rv, lay, tau, "%s two paths v" % name)
    print("%s: one launch against per-step from the same state: max |d| / rms(layer) m %.2e v %.2e" % (name, wm, wv))
