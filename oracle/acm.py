"""ORACLE (test infrastructure only): AcMTrainer.batch_update, restated.

rltoolkit/acm/acm.py:246-258 — y_pred = ACM(x); loss = MSE(y_pred, y); Adam step.
Batch assembly: acm_cat (acm.py:260-264) = cat(obs[:, idx], next_obs[:, idx]).
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import nets
from .adam import OracleAdam


class OracleAcmTrainer:
    def __init__(self, inp, ac, lr=3e-3, ac_lim=1.0, params=None, dtype=torch.float32, m=None, v=None, t=0):
        """dtype float64: a reference whose own rounding is negligible.  m, v (flat, state_dict order), t:
        resume Adam from these moments and step count."""
        self.layout = nets.acm_layout(inp, ac)
        self.dtype = dtype
        self.p = {n: torch.as_tensor(params[n]).to(dtype).clone().requires_grad_(True) for n, _ in self.layout}
        self.lim = torch.as_tensor(ac_lim).to(dtype)
        split = lambda flat: None if flat is None else [  # noqa: E731
            x.clone() for x in nets.unflatten(torch.as_tensor(flat).to(dtype), self.layout, dtype=dtype).values()]
        self.opt = OracleAdam(self.p.values(), lr, m=split(m), v=split(v), t=t)

    def batch_update(self, x, y):
        x = torch.as_tensor(np.asarray(x)).to(self.dtype)
        y = torch.as_tensor(np.asarray(y)).to(self.dtype)
        if y.dim() < 2:
            y = y.reshape(len(y), -1)
        loss = F.mse_loss(nets.acm(self.p, x, self.lim), y)
        g = torch.autograd.grad(loss, list(self.p.values()))
        self.last_grad = torch.cat([t.reshape(-1) for t in g]).numpy()
        self.opt.step(g)
        return loss.item()

    def flat(self):
        return nets.flatten(self.p).numpy()

    def moments(self):
        """(exp_avg, exp_avg_sq), flat in state_dict order."""
        return (torch.cat([x.reshape(-1) for x in self.opt.m]).numpy(),
                torch.cat([x.reshape(-1) for x in self.opt.v]).numpy())


def acm_cat(obs, next_obs, idx=None):
    obs, next_obs = np.asarray(obs), np.asarray(next_obs)
    if idx is not None:
        obs, next_obs = obs[:, idx], next_obs[:, idx]
    return np.concatenate([obs, next_obs], axis=1)
