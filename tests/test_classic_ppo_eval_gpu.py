"""gymrl_classic_ppo_eval on an MI355X (csrc/eval_classic_ppo.hip): whole deterministic episodes of CartPole-v1, MountainCar-v0 and
Acrobot-v1 under PPOTrainer's actor-critic in ONE launch, against the step loop act_forward -> categorical_sample(deterministic) ->
VecEnv.step on eval()'s own streams.  Every comparison is exact: returns (the float64 sum of the float32 rewards), lengths,
terminated flags and final observations."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E_MAX = 33                                             # two full workgroups and one lane of a third; the first 10 are the E = 10 case
CASES = pytest.mark.parametrize("env_name,hidden", [(e, h) for e in ("CartPole-v1", "MountainCar-v0", "Acrobot-v1") for h in (64, 32)])
_CTX = {}


def _trainer(env_name, hidden, fused_eval=False):
    from gymrl_amd import ops
    from gymrl_amd.ppo_lunarlander import Config, PPOTrainer
    assert torch.cuda.is_available() and ops.device_ok(), "gpu tests need an MI355X"
    cfg = Config()
    cfg.env_name, cfg.hidden_dim, cfg.seed, cfg.fused_eval = env_name, hidden, 5, fused_eval
    cfg.num_envs, cfg.update_freq = 16, 8
    return PPOTrainer(cfg)


def _loop(tr, E):
    """The step loop on eval()'s streams under act_forward's logits, episode e = env EVAL_ENV_ID0 + e -> dict of numpy arrays [E]
    (returns64: the float64 sum of the float32 rewards; returns32: the stepper's own float32 ep_ret_out)."""
    from gymrl_amd import ops
    from gymrl_amd.envs import VecEnv
    dev = tr.device
    env = VecEnv(tr.cfg.env_name, E, device=dev, seed=tr.base_seed + tr.EVAL_SEED_OFFSET, env_id0=tr.EVAL_ENV_ID0)
    obs = env.reset()
    nxt, term = torch.empty_like(obs), torch.empty_like(obs)
    rew, ep_ret = torch.empty(E, device=dev), torch.zeros(E, device=dev)
    done, termd, trunc = (torch.zeros(E, dtype=torch.uint8, device=dev) for _ in range(3))
    running = torch.ones(E, dtype=torch.bool, device=dev)
    ret64 = torch.zeros(E, dtype=torch.float64, device=dev)
    out = dict(returns32=torch.zeros(E, device=dev), lengths=torch.zeros(E, dtype=torch.int32, device=dev),
               terminated=torch.zeros(E, dtype=torch.uint8, device=dev), final_obs=torch.zeros_like(obs))
    tr.model.refresh_act()
    for step in range(env.max_steps):
        logits, _ = tr.model.act_forward(obs, refresh=False)
        act = ops.categorical_sample(logits, deterministic=True)[0]
        env.step(act, nxt, rew, done_out=done, term_obs_out=term, ep_ret_out=ep_ret, terminated_out=termd, truncated_out=trunc)
        ret64 += torch.where(running, rew.double(), torch.zeros_like(ret64))
        first = done.bool() & running
        out["returns32"] = torch.where(first, ep_ret, out["returns32"])
        out["lengths"] = torch.where(first, torch.full_like(out["lengths"], step + 1), out["lengths"])
        out["terminated"] = torch.where(first, termd, out["terminated"])
        out["final_obs"] = torch.where(first[:, None], term, out["final_obs"])
        running &= ~first
        obs, nxt = nxt, obs
        if not bool(running.any()):
            break
    assert not bool(running.any()), "every episode ends at the TimeLimit at the latest"
    out["returns64"] = ret64
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ctx(env_name, hidden):
    """One trainer with a fresh policy and its step-loop reference per case, computed once and shared (never modified)."""
    key = (env_name, hidden)
    if key not in _CTX:
        tr = _trainer(env_name, hidden)
        _CTX[key] = (tr, _loop(tr, E_MAX))
    return _CTX[key]


def _launch(tr, E, **kw):
    from gymrl_amd import ops
    net = tr._eval_net()
    assert net is not None
    out = ops.classic_ppo_eval(tr.env.kind, net, E, tr.base_seed + tr.EVAL_SEED_OFFSET, tr.EVAL_ENV_ID0, device=tr.device, **kw)
    return tuple(None if t is None else t.cpu().numpy() for t in out)


@CASES
@pytest.mark.parametrize("E", [10, E_MAX])
def test_one_launch_is_the_step_loop(env_name, hidden, E):
    tr, want = _ctx(env_name, hidden)
    ret, length, termd = tr.evaluate(E)
    assert ret.dtype == np.float64 and ret.shape == length.shape == termd.shape == (1, E)
    assert np.array_equal(ret[0], want["returns64"][:E])
    assert np.array_equal(ret[0].astype(np.float32), want["returns32"][:E])            # where the loop only has float32
    assert np.array_equal(length[0], want["lengths"][:E]) and np.array_equal(termd[0], want["terminated"][:E])
    ret2, length2, termd2, final = _launch(tr, E, want_final_obs=True)
    assert np.array_equal(ret2, ret) and np.array_equal(length2, length) and np.array_equal(termd2, termd)
    assert final.dtype == np.float32 and final.shape == (1, E, tr.env.obs_dim)
    assert np.array_equal(final[0], want["final_obs"][:E])
    assert int(length.min()) >= 1 and int(length.max()) <= tr.env.max_steps


@CASES
def test_population_rows_are_the_policies_evaluated_alone(env_name, hidden):
    tr, _ = _ctx(env_name, hidden)
    E = 10
    own = tr.flat_params.detach().clone()
    gen = torch.Generator().manual_seed(3)
    params = own.unsqueeze(0) + 0.3 * torch.randn(3, own.numel(), generator=gen).to(tr.device)
    together = tr.evaluate(E, params)
    assert together[0].shape == (3, E)
    try:
        for p in range(3):
            tr.flat_params.copy_(params[p])
            alone = tr.evaluate(E)
            for got, one in zip(together, alone):
                assert np.array_equal(got[p], one[0]), p
    finally:
        tr.flat_params.copy_(own)
    one = tr.evaluate(E, params[1])                                         # a single vector is a population of one
    assert all(np.array_equal(g[0], t[1]) for g, t in zip(one, together))


@CASES
def test_stream_offset_and_cap(env_name, hidden):
    tr, want = _ctx(env_name, hidden)
    shifted = tr.evaluate(4, stream_offset=5)
    assert np.array_equal(shifted[0][0], want["returns64"][5:9]) and np.array_equal(shifted[1][0], want["lengths"][5:9])
    assert np.array_equal(shifted[2][0], want["terminated"][5:9])
    ret, length, termd, _ = _launch(tr, E_MAX, cap=7)
    assert np.array_equal(length, np.full((1, E_MAX), 7)) and not termd.any()
    assert np.array_equal(ret[0], {"CartPole-v1": 7.0, "MountainCar-v0": -7.0, "Acrobot-v1": -7.0}[env_name] * np.ones(E_MAX))


@CASES
def test_fused_eval_returns_the_loops_list_and_evaluate_moves_nothing(env_name, hidden):
    tr, want = _ctx(env_name, hidden)
    state, count, flat = tr.env.state.clone(), tr.rollout_count, tr.flat_params.detach().clone()
    steps = tr.step_count
    tr.evaluate(10)
    tr.evaluate(3, params=flat.unsqueeze(0).repeat(2, 1), stream_offset=2)
    assert torch.equal(tr.env.state, state) and tr.rollout_count == count and tr.step_count == steps
    assert torch.equal(tr.flat_params, flat)
    assert tr.cfg.fused_eval is False and tr._eval_fused(10) is None
    tr.cfg.fused_eval = True
    try:
        got = tr.eval(10)
    finally:
        tr.cfg.fused_eval = False
    assert isinstance(got, list) and got == want["returns32"][:10].tolist()
    assert torch.equal(tr.env.state, state) and tr.rollout_count == count and torch.equal(tr.flat_params, flat)


def test_a_network_the_forward_refuses_keeps_the_loop_and_the_error():
    tr = _trainer("Acrobot-v1", 260, fused_eval=True)                       # wider than the one-launch forward's LDS buffers
    assert tr.model._act_net() is False and tr._eval_net() is None and not tr._persistent_ok()
    off = _trainer("Acrobot-v1", 260, fused_eval=False)
    assert tr.eval(2) == off.eval(2)                                        # the loop, whatever the switch says
    with pytest.raises(RuntimeError, match="gymrl_classic_ppo_eval"):
        tr.evaluate(2)
