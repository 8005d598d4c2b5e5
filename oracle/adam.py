"""ORACLE (test infrastructure only): torch.optim.Adam step, restated.

Third-party algorithm (torch 1.3.1 pinned by the reference, 2.10 here; the
golden vectors come from the installed 2.10 single-tensor CPU path):
  m <- lerp(m, g, 1-b1); v <- v*b2 + (1-b2) g^2
  p <- p - lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
Used by every optimizer of the hot path (rltoolkit/rl.py:62, ddpg.py:132-135,
sac.py:107-110, acm.py:176-183); betas (0.9, 0.999), eps 1e-8, no weight decay.

Besides OracleAdam (torch tensors, any dtype, resumable from given moments and step
count) there are two flat numpy restatements of the same step from a given state
(p, m, v, t), with the optional polyak average of a target towards the NEW parameter:
  adam_steps_f64   float64 throughout: the reference
  adam_steps_f32   float32 with one rounding per operation, in the operation order the
                   device kernels state (k_adam, optim.hip; the in-register Adam of
                   sgd_mlp.hip): what a correct kernel produces bit for bit
Both take the learning rate and tau as the float32 values the library stores.
"""
import math

import numpy as np
import torch


class OracleAdam:
    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, m=None, v=None, t=0):
        """m, v, t: resume from these moments (lists like params; copied) and step count."""
        self.params = list(params)
        self.lr, self.b1, self.b2, self.eps = lr, betas[0], betas[1], eps
        self.m = [torch.zeros_like(p) for p in self.params] if m is None else \
            [torch.as_tensor(x).to(p.dtype).reshape(p.shape).clone() for x, p in zip(m, self.params)]
        self.v = [torch.zeros_like(p) for p in self.params] if v is None else \
            [torch.as_tensor(x).to(p.dtype).reshape(p.shape).clone() for x, p in zip(v, self.params)]
        assert len(self.m) == len(self.params) and len(self.v) == len(self.params)
        self.t = int(t)

    @torch.no_grad()
    def step(self, grads):
        self.t += 1
        bc1 = 1 - self.b1 ** self.t
        bc2s = (1 - self.b2 ** self.t) ** 0.5
        step_size = self.lr / bc1
        for p, g, m, v in zip(self.params, grads, self.m, self.v):
            if g is None:
                g = torch.zeros_like(p)
            m.lerp_(g, 1 - self.b1)
            v.mul_(self.b2).addcmul_(g, g, value=1 - self.b2)
            denom = (v.sqrt() / bc2s).add_(self.eps)
            p.addcdiv_(m, denom, value=-step_size)


def _lrs(lr, n):
    lrs = [lr] * n if np.ndim(lr) == 0 else list(lr)
    assert len(lrs) == n, "one learning rate per step"
    return [float(np.float32(x)) for x in lrs]  # the library keeps its rates as float


def adam_steps_f64(p, m, v, t, grads, lr, target=None, tau=None):
    """len(grads) Adam steps from the state (p, m, v, t steps taken) in float64.  ``lr``: one rate or one per
    step.  ``target``/``tau``: after every step target <- target * (1 - tau) + tau * p_new.
    Returns (p, m, v, target or None, t + len(grads))."""
    p, m, v = (np.array(x, np.float64) for x in (p, m, v))
    tg = None if target is None else np.array(target, np.float64)
    tau = None if tau is None else float(np.float32(tau))
    for g, a in zip(grads, _lrs(lr, len(grads))):
        t += 1
        g = np.asarray(g, np.float64)
        m = m + 0.1 * (g - m)
        v = v * 0.999 + (0.001 * g) * g
        bc1, bc2s = 1.0 - 0.9 ** t, math.sqrt(1.0 - 0.999 ** t)
        p = p - (a / bc1) * (m / (np.sqrt(v) / bc2s + 1e-8))
        if tg is not None:
            tg = tg * (1.0 - tau) + tau * p
    return p, m, v, tg, t


def adam_steps_f32(p, m, v, t, grads, lr, target=None, tau=None):
    """The same steps as the device computes them: float32, every operation rounded once, none fused:
         m = m + 0.1f * (g - m)
         v = v * 0.999f + (0.001f * g) * g
         denom = sqrt(v) / bc2s + 1e-8f
         p = p + neg_step * (m / denom)
         target = target * float(1 - (double)tau) + tau * p
       with neg_step = float(-(lr / (1 - 0.9^t))) and bc2s = float(sqrt(1 - 0.999^t)) from doubles."""
    f = np.float32
    p, m, v = (np.array(x, f) for x in (p, m, v))
    tg = None if target is None else np.array(target, f)
    for g, a in zip(grads, _lrs(lr, len(grads))):
        t += 1
        g = np.asarray(g, f)
        assert g.dtype == f and p.dtype == f and m.dtype == f and v.dtype == f
        m = m + f(0.1) * (g - m)
        v = v * f(0.999) + (f(0.001) * g) * g
        neg_step = f(-(a / (1.0 - 0.9 ** t)))
        bc2s = f(math.sqrt(1.0 - 0.999 ** t))
        denom = np.sqrt(v) / bc2s + f(1e-8)
        p = p + neg_step * (m / denom)
        if tg is not None:
            omtau = f(1.0 - float(f(tau)))
            tg = tg * omtau + f(tau) * p
    return p, m, v, tg, t


def adam_scales(p0, m0, grads, lr, v_ref):
    """Per-element scales of the normalised errors of p, m and v after len(grads) steps:
       s_p = max(|p0|, K lr), s_m = max(|m0|, max_k |g_k|), s_v = max(s_m^2, v_ref)."""
    K = len(grads)
    lr_max = float(np.max(lr))
    s_p = np.maximum(np.abs(np.asarray(p0, np.float64)), K * lr_max)
    gmax = np.max(np.abs(np.stack([np.asarray(g, np.float64) for g in grads])), axis=0)
    s_m = np.maximum(np.abs(np.asarray(m0, np.float64)), gmax)
    s_m = np.maximum(s_m, 1e-30)  # (elements with no gradient and no moment: both sides are exact zeros)
    s_v = np.maximum(s_m ** 2, np.asarray(v_ref, np.float64))
    return s_p, s_m, s_v


def designed_state(rng, n):
    """A resumed optimizer state for n elements: p0 ~ U(-1, 1); |m0| log-uniform in [1e-6, 1e2] with random
    signs, independent of the gradient it will meet; v0 = m0^2 x 10^U(0, 2) in [1e-12, 1e6] (|m| <= sqrt(v), as
    Adam's own moments are: a step stays lr-sized); a block of exact zeros in both (elements n/8 .. n/4)."""
    f = np.float32
    p0 = rng.uniform(-1, 1, n).astype(f)
    m0 = (10.0 ** rng.uniform(-6, 2, n) * rng.choice([-1.0, 1.0], n)).astype(f)
    v0 = (m0.astype(np.float64) ** 2 * 10.0 ** rng.uniform(0, 2, n)).astype(f)
    m0[n // 8:n // 4] = 0
    v0[n // 8:n // 4] = 0
    return p0, m0, v0


def designed_gradient(rng, n, huge=4):
    """A gradient of n elements that exercises every term of the step: magnitudes log-uniform in
    [1e-6, 1e2] with random signs; exact zeros in elements 0 .. n/4 (with designed_state: the first half of
    them over live moments, the second over zero moments, where the step must leave p bit-unchanged);
    ``huge`` entries of +-1e18 at random places outside the zero blocks.  Every non-zero |g| >= 1e-6, so with
    designed_state every intermediate of the step stays in the normal float32 range."""
    g = (10.0 ** rng.uniform(-6, 2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[:n // 4] = 0
    if huge and n - n // 4 > huge:
        at = n // 4 + rng.choice(n - n // 4, huge, replace=False)
        g[at] = (1e18 * rng.choice([-1.0, 1.0], huge)).astype(np.float32)
    return g
