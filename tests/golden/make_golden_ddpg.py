"""Generator of tests/golden/ddpg_vanilla_hcheetah.npz: vanilla DDPG from the reference implementation.

Run once where the reference checkout is available (the tests only read the .npz):

    python tests/golden/make_golden_ddpg.py

Uses make_golden.py's dependency stand-ins (gym, tensorboard) and its save() / load() / fill_params helpers.
DDPG(env_name="HalfCheetah-v2", gamma=0.99) runs 2 update calls at B = 100 on seeded batches; recorded are the
losses, the post-update actor / critic / actor_targ / critic_targ, and noise_action for a few observations
with the torch.randn draw injected.  Inputs are rebuilt from the seed by tests/ddpg_ref.py golden_inputs.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402  (stand-ins first, then the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rltoolkit.algorithms import DDPG  # noqa: E402

from ddpg_ref import GOLDEN_SEED, NETS, golden_inputs  # noqa: E402


def gen_ddpg_vanilla(seed=GOLDEN_SEED, B=100, steps=2):
    torch.manual_seed(0)
    m = DDPG(env_name="HalfCheetah-v2", gamma=0.99, actor_lr=1e-3, critic_lr=1e-3, buffer_size=1000,
             update_batch_size=B, use_gpu=False)
    ob, ac = m.ob_dim, m.ac_dim
    mods = {"actor": m._actor, "critic": m._critic, "actor_targ": m.actor_targ, "critic_targ": m.critic_targ}
    assert tuple(mods) == NETS
    for i, mod in enumerate(mods.values()):
        mg.load(mod, seed * 100 + i)
    params, batches, act_obs, act_draw = golden_inputs(seed, ob, ac, B, steps)
    for k, mod in mods.items():  # the rebuilt inputs are the ones loaded
        np.testing.assert_array_equal(mg.flat_params(mod), np.concatenate([v.ravel() for v in params[k].values()]))
    out = dict(dims=np.array([ob, ac, B]), seed=np.array(seed), ac_lim=m.ac_lim.numpy().astype(np.float32),
               tau=np.array(m.tau), gamma=np.array(m.gamma), act_noise=np.array(m.act_noise),
               max_ep_len=np.array(m.max_ep_len if m.max_ep_len is not None else -1))
    # noise_action (ddpg.py:171-176) before the updates, one observation at a time as the rollout calls it
    randn, acts, dets = torch.randn, [], []
    for o, d in zip(act_obs, act_draw):
        torch.randn = lambda *a, _d=d, **k: torch.from_numpy(_d.copy())
        try:
            acts.append(m.noise_action(torch.from_numpy(o)[None], m.act_noise).numpy()[0])
            dets.append(m.noise_action(torch.from_numpy(o)[None], 0, deterministic=True).numpy()[0])
        finally:
            torch.randn = randn
    out["noise_action"], out["det_action"] = np.array(acts, np.float32), np.array(dets, np.float32)
    losses = []
    for batch in batches:
        m.update(*(torch.from_numpy(x) for x in batch))
        losses.append([m.loss["critic"], m.loss["actor"]])
    out["losses"] = np.array(losses)
    for k, mod in mods.items():
        out["post_" + k] = mg.flat_params(mod)
    mg.save("ddpg_vanilla_hcheetah.npz", **out)


if __name__ == "__main__":
    gen_ddpg_vanilla()
