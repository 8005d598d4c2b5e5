"""GPU parity of vanilla DDPG (spprl.DDPG, rltoolkit/algorithms/ddpg/ddpg.py) against the reference-generated
fixture tests/golden/ddpg_vanilla_hcheetah.npz (HalfCheetah dims, 2 updates of B = 100) and the torch
restatement tests/ddpg_ref.py.  Tolerances as tests/test_gpu_sac.py: losses rel 1e-4 / abs 1e-6, gradients
relative error < 2e-4, post-Adam parameters within the first-step sign-flip allowance; the team (small-batch)
and one-wave forms of the phase kernels both against the float64 restatement."""
import ctypes

import numpy as np
import pytest
import torch

import spprl
from spprl import _lib
from bf16_cases import assert_tensor_grads, fp32_elem_tol
from ddpg_ref import DdpgRef, ddpg_vanilla_case, noise_action

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = {"actor": _lib.SPP_NET_ACTOR, "critic": _lib.SPP_NET_CRITIC1, "actor_targ": _lib.SPP_NET_ACTOR_TARG,
         "critic_targ": _lib.SPP_NET_CRITIC1_TARG}
OB, AC = 17, 6


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def build(params, B, **kw):
    ag = spprl.DDPG(env_name="HalfCheetah-v2", gamma=0.99, actor_lr=1e-3, critic_lr=1e-3, max_batch=B,
                    buffer_size=kw.pop("buffer_size", 64), device=DEV, **kw)
    if params is not None:
        for k, net in NAMES.items():
            ag.load_net(net, params[k])
    return ag


def params_of(ag):
    return {k: {n: v.numpy().copy() for n, v in ag.net_state(net).items()} for k, net in NAMES.items()}


def draw_batch(rng, B):
    return (rng.randn(B, OB).astype(np.float32), rng.randn(B, OB).astype(np.float32),
            rng.uniform(-1, 1, (B, AC)).astype(np.float32), rng.randn(B).astype(np.float32),
            (rng.rand(B) < 0.1).astype(np.int8))


def check_against_float64(ag, batch, what):
    """One update of ag against the float64 restatement from ag's own parameters; returns the gradients."""
    B = batch[0].shape[0]
    o = DdpgRef(OB, AC, gamma=0.99, params=params_of(ag), dtype=torch.float64)
    ag.update(*batch)
    torch.cuda.synchronize()
    ol = o.update(*batch)
    grads = {}
    for k in ("critic", "actor"):
        g = ag.grads[NAMES[k]].cpu().numpy()
        e = relerr(g, o.last["grads"][k])
        print(what, k, "rel %.3g" % e)
        assert e < 2e-4, (what, k, e)
        assert_tensor_grads(g, o.last["grads"][k], o.layouts[k], 2e-4, "%s %s" % (what, k), fp32_elem_tol(B))
        assert ag.loss[k] == pytest.approx(ol[k], rel=1e-4, abs=1e-6), (what, k)
        grads[k] = g
    return grads


def test_update_matches_restatement_and_reference():
    fx, params, batches, _, _ = ddpg_vanilla_case()
    ob, ac, B = (int(v) for v in fx["dims"])
    ag = build(params, B)
    assert ag.tau == 0.005 and ag.act_noise == 0.1 and ag.max_ep_len == 1000  # DDPG forwards both; Q3
    o = DdpgRef(ob, ac, ac_lim=fx["ac_lim"], gamma=0.99, params=params)
    for i, batch in enumerate(batches):
        ag.update(*batch)
        ol = o.update(*batch)
        torch.cuda.synchronize()
        for k in ("critic", "actor"):
            e = relerr(ag.grads[NAMES[k]].cpu().numpy(), o.last["grads"][k])
            assert e < 2e-4, (k, e)
        gl = ag.loss
        assert set(gl) == {"actor", "critic"}
        for j, k in enumerate(("critic", "actor")):
            assert gl[k] == pytest.approx(ol[k], rel=1e-4, abs=1e-6), k
            assert gl[k] == pytest.approx(float(fx["losses"][i][j]), rel=1e-4, abs=1e-6), k
    for k in NAMES:  # the second Adam step and both polyaks
        d = np.abs(ag.params[NAMES[k]].cpu().numpy() - fx["post_" + k])
        assert d.max() <= 2 * len(batches) * 1e-3 * 1.01, (k, d.max())
        assert np.mean(d > 1e-5) < 2e-3, (k, np.mean(d > 1e-5))


def test_tau_and_act_noise_are_honoured():
    ag = build(None, 32, seed=1, tau=0.25, act_noise=0.3)
    assert ag.tau == 0.25 and ag.act_noise == 0.3
    p0 = params_of(ag)
    batch = draw_batch(np.random.RandomState(0), 32)
    o = DdpgRef(OB, AC, gamma=0.99, tau=0.25, params=p0)
    ag.update(*batch)
    o.update(*batch)
    torch.cuda.synchronize()
    for k in ("actor_targ", "critic_targ"):
        np.testing.assert_allclose(ag.params[NAMES[k]].cpu().numpy(), o.flat(k), atol=2 * 1e-3 * 0.25 * 1.01 + 1e-7)
        assert np.abs(ag.params[NAMES[k]].cpu().numpy() - np.concatenate([v.ravel() for v in p0[k].values()])).max() > 0


@pytest.mark.parametrize("B", [1, 33, 100, 1000, 8192])
def test_team_kernels_match_float64_restatement(B, monkeypatch):
    """Small batches (at most one 32-sample tile per CU) run the team forms of the phase kernels
    (csrc/ddpg_team.h); SPP_SAC_TEAM=0 forces the one-wave kernels.  Both against the float64 restatement at the
    same tolerance, and not bit-identical to each other (a different q / fc3 / one-block-layer summation order:
    evidence that the team kernels ran)."""
    batch = draw_batch(np.random.RandomState(B), B)
    grads = {}
    for team in ("1", "0"):
        monkeypatch.setenv("SPP_SAC_TEAM", team)
        grads[team] = check_against_float64(build(None, B, seed=5), batch, "team=%s B=%d" % (team, B))
    assert any(not np.array_equal(grads["1"][k], grads["0"][k]) for k in ("critic", "actor"))


def second_tile_batch():
    """One tile more than the one-wave phase grid's waves (tests/test_gpu_gen_inputs.py second_tile_batch)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 32 * (4 * cus + 1)


@pytest.mark.parametrize("which", ["257_tiles", "second_tile"])
def test_one_wave_kernels_by_selection(which):
    """B = 8224 (257 tiles: more tiles than CUs, so the one-wave kernels by selection) and 4 * CUs * 32 + 32 (one
    wave of the one-wave grid takes a second tile)."""
    B = 8224 if which == "257_tiles" else second_tile_batch()
    assert B // 32 > torch.cuda.get_device_properties(0).multi_processor_count
    check_against_float64(build(None, B, seed=6), draw_batch(np.random.RandomState(B % 1000), B), which)


def test_act_modes_match_restatement():
    fx, params, _, _, _ = ddpg_vanilla_case()
    ag = build(params, 100)
    rng = np.random.RandomState(2)
    E = 300
    obs = (rng.randn(E, OB) * 1.3).astype(np.float32)
    noise = (rng.randn(E, AC) * 3).astype(np.float32)  # (x3: some actions reach the clip)
    t = lambda z: torch.from_numpy(z).to(DEV)  # noqa: E731
    tgt, env = ag.act(t(obs), noise=t(noise), mode=1)  # noise_action with act_noise 0.1
    torch.cuda.synchronize()
    want = noise_action(params["actor"], obs, 1.0, noise, 0.1)
    assert (np.abs(want) == 1.0).any()
    np.testing.assert_allclose(env.cpu().numpy(), want, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(tgt.cpu().numpy(), env.cpu().numpy())  # process_action is the identity
    assert np.abs(env.cpu().numpy()).max() <= 1.0
    tgt, env = ag.act(t(obs), mode=2, act_noise=0.0)  # test(): deterministic
    torch.cuda.synchronize()
    np.testing.assert_allclose(env.cpu().numpy(), noise_action(params["actor"], obs, 1.0, None, 0.0), rtol=1e-5,
                               atol=1e-5)
    np.testing.assert_array_equal(tgt.cpu().numpy(), env.cpu().numpy())
    u = rng.uniform(-1, 1, (E, AC)).astype(np.float32)
    tgt, env = ag.act(t(obs), eps=t(u), mode=0)  # initial_act: the env's own sample, unchanged
    torch.cuda.synchronize()
    np.testing.assert_array_equal(env.cpu().numpy(), u)
    np.testing.assert_array_equal(tgt.cpu().numpy(), u)


def test_act_matches_reference_fixture():
    fx, params, _, act_obs, act_draw = ddpg_vanilla_case()
    ag = build(params, 100)
    t = lambda z: torch.from_numpy(z).to(DEV)  # noqa: E731
    _, env = ag.act(t(act_obs), noise=t(act_draw), mode=1)
    _, det = ag.act(t(act_obs), mode=2, act_noise=0.0)
    torch.cuda.synchronize()
    np.testing.assert_allclose(env.cpu().numpy(), fx["noise_action"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(det.cpu().numpy(), fx["det_action"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("E", [1, 33])
def test_team_act_equals_one_wave(E, monkeypatch):
    fx, params, _, _, _ = ddpg_vanilla_case()
    rng = np.random.RandomState(E)
    obs = (rng.randn(E, OB) * 1.3).astype(np.float32)
    noise = rng.randn(E, AC).astype(np.float32)
    u = rng.uniform(-1, 1, (E, AC)).astype(np.float32)
    t = lambda z: torch.from_numpy(z).to(DEV)  # noqa: E731
    out = {}
    for team in ("1", "0"):
        monkeypatch.setenv("SPP_SAC_TEAM", team)
        ag = build(params, 100)
        out[team] = [ag.act(t(obs), noise=t(noise), mode=1)[1].cpu().numpy(),
                     ag.act(t(obs), mode=2, act_noise=0.0)[1].cpu().numpy(),
                     ag.act(t(obs), eps=t(u), mode=0)[1].cpu().numpy()]
    want = noise_action(params["actor"], obs, 1.0, noise, 0.1)
    for team in ("1", "0"):
        np.testing.assert_allclose(out[team][0], want, rtol=1e-5, atol=1e-5, err_msg=team)
        np.testing.assert_array_equal(out[team][2], u)
    for a, b in zip(out["1"], out["0"]):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-5)


def test_reference_schedule_loop():
    """The baseline's loop: 1 env, random frames, B = 100 grad steps every 50 frames, time-limit ends stored as
    end but not done (Q3), obs stats per iteration."""
    ag = build(None, 100, seed=1, n_envs=1, batch_size=250, iterations=2, random_frames=100, update_freq=50,
               grad_steps=5, buffer_size=10_000, env_spec=(17, 6, 1.0, 120))
    assert ag.schedule == "reference"
    ag.train()
    torch.cuda.synchronize()
    rb = ag.replay_buffer
    assert ag.stats_logger.frames == 2 * 360 and len(rb) == 720  # whole episodes of 120 frames
    obs, nobs, act, rew, done = rb.gather(torch.arange(len(rb)))
    assert int(done.sum()) == 0  # 6 episodes ended at the time limit: none of them is done
    assert set(ag.loss) == {"actor", "critic"}
    for k, val in ag.loss.items():
        assert np.isfinite(val), k
    assert np.abs(act.cpu().numpy()).max() <= 1.0
    assert np.isfinite(ag.test(episodes=2))


def test_fused_loop_runs():
    E = 256
    ag = build(None, 100 * E, seed=2, n_envs=E, batch_size=2 * E, iterations=2, random_frames=E,
               buffer_size=100_000)
    assert ag.schedule == "fused"
    ag.train()
    torch.cuda.synchronize()
    assert ag.stats_logger.frames == 4 * E
    for k, v in ag.loss.items():
        assert np.isfinite(v), k
    _, _, act, _, _ = ag.replay_buffer.gather(torch.arange(len(ag.replay_buffer)))
    assert np.abs(act.cpu().numpy()).max() <= 1.0


def _ring_agent(params, Bs, seed=9):
    """An obs_norm agent whose ring holds 400 transitions with observations beyond the +-10 clip."""
    ag = build(params, Bs, obs_norm=True, buffer_size=512)
    rb = ag.replay_buffer
    r = np.random.RandomState(seed)
    prev = rb.add_obs(r.randn(OB).astype(np.float32) * 4)
    for t in range(400):
        nxt = rb.add_obs((r.randn(OB) * 4 + 1).astype(np.float32))
        rb.add_timestep(prev, nxt, r.uniform(-1, 1, AC).astype(np.float32), float(r.randn()), bool(r.rand() < 0.1),
                        False)
        prev = nxt
    return ag


@pytest.mark.parametrize("stats", [False, True])
def test_obs_norm_staged_equals_caller_batch(stats):
    """sppAgentStageFromReplay + sppAgentStagePost(normalize = 2) -- the z-score of the ring's statistics although
    the agent's normaliser is min-max (its actor output's identity) -- leaves the parameters of the caller-batch
    update on the gathered, normalised tuples, bit for bit."""
    params = ddpg_vanilla_case()[1]
    Bs = 120
    a1, a2 = _ring_agent(params, Bs), _ring_agent(params, Bs)
    if stats:
        a1.update_obs_stats()
        a2.update_obs_stats()
    idx = torch.from_numpy(np.random.RandomState(5).randint(0, len(a1.replay_buffer), Bs)).to(DEV)
    a1.update_from_replay(idx, 91, 3)
    batch = a2.replay_buffer.gather(idx)
    raw = a2.replay_buffer
    raw.obs_norm = False
    unnorm = raw.gather(idx)
    raw.obs_norm = True
    assert not torch.equal(batch[0], unnorm[0])  # the normalisation ran (the clip at +-10 at least)
    a2.update(*batch)
    torch.cuda.synchronize()
    for net in NAMES.values():
        np.testing.assert_array_equal(a1.params[net].cpu().numpy(), a2.params[net].cpu().numpy(), err_msg=str(net))
    assert a1.loss == a2.loss


def test_checkpoint_round_trip(tmp_path):
    a1, a2 = build(None, 32, seed=3), build(None, 32, seed=4)
    a1.update(*draw_batch(np.random.RandomState(1), 32))
    d = a1.collect_params_dict()
    assert list(d) == ["actor", "critic", "obs_mean", "obs_std", "min_obs", "max_obs"]  # ddpg.py:331-339
    obs = torch.from_numpy(np.random.RandomState(2).randn(40, OB).astype(np.float32)).to(DEV)
    want = a1.act(obs, mode=2)[1].cpu().numpy()
    assert not np.array_equal(a2.act(obs, mode=2)[1].cpu().numpy(), want)
    path = str(tmp_path / "ddpg.pt")
    a1.save(path)
    a2.load(path)
    np.testing.assert_array_equal(a2.act(obs, mode=2)[1].cpu().numpy(), want)
    with pytest.raises(AttributeError):
        a1.pre_train()


def _create(algo, ob, aout, ac, acm_critic=0, custom_loss=0.0):
    cfg = _lib.AgentConfig(algo, ob, aout, ac, acm_critic, 1, 0, custom_loss, 0.99, 0.005, 1e-3, 1e-3, 0.0, 0.0, 0.0,
                           64)
    h = ctypes.c_void_p()
    lib = _lib.load()
    rc = lib.sppAgentCreate(ctypes.byref(h), ctypes.byref(cfg), 0)
    msg = lib.sppGetLastError().decode()
    if rc == 0:
        lib.sppAgentDestroy(h)
    return rc, msg


def test_refusals():
    rc, msg = _create(_lib.SPP_ALGO_DDPG, 17, 17, 6)
    assert rc != 0 and "aout == ac" in msg
    rc, msg = _create(_lib.SPP_ALGO_DDPG, 17, 6, 6, custom_loss=0.1)
    assert rc != 0 and "vanilla DDPG" in msg
    rc, msg = _create(_lib.SPP_ALGO_DDPG, 17, 6, 6, acm_critic=1)
    assert rc != 0 and "vanilla DDPG" in msg
    rc, msg = _create(_lib.SPP_ALGO_DDPG, 11, 3, 3)
    assert rc != 0 and "no kernel instantiation" in msg and "ob=11" in msg
    rc, msg = _create(_lib.SPP_ALGO_DDPG, 17, 6, 6)
    assert rc == 0, msg
