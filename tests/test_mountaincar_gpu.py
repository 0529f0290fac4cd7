"""MountainCar-v0 on an MI355X: the batched stepper (csrc/env_classic.hip, kind 3) and the one-launch episode kernel
(csrc/mountaincar.hip) against tests/mountaincar_ref.py.  The state is float64, every operation is spelled out and cos is the
device's det_sincos restated on the host, so every comparison is array_equal: observations, rewards, flags, episode returns and
lengths, ep_stats and the float64 state."""
import subprocess
import sys

import numpy as np
import pytest

import mountaincar_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED, T_STEPS, N_MAX = 42, 420, 130
ALWAYS_RIGHT = (0.0, 0.0, -1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0)             # lb = -1 < v < ub = 1 everywhere: action 2
NEVER_IN_BAND = ref.RULE_COEFS[:8] + (-1.0,)                               # ub < -0.07 everywhere: action 0
PERTURBED = (-0.1, 0.27, 0.028, 0.33, 0.88, 0.009, -0.06, 0.4, 0.065)
# (pos, vel): into the wall, the issue's (0, 0.0699), into the speed clamp upwards (and the position clamp), just the speed
# clamp, the speed clamp downwards, past the goal moving left, at rest on the wall
SEAM_STARTS = ((-1.19, -0.05), (0.0, 0.0699), (0.55, 0.0699), (0.45, 0.0699), (-0.5, -0.0699), (0.55, -0.01), (-1.2, 0.0))


def _gpu():
    import torch
    from gymrl_amd import ops
    if not (torch.cuda.is_available() and ops.device_ok()):
        pytest.fail("gpu test without a usable MI355X")
    return torch, ops, torch.device("cuda:0")


_REFS = {}


def _ref_traces(policy, env_id0=0, n=N_MAX, steps=T_STEPS, abandon_cap=0):
    """Reference traces of envs env_id0 .. env_id0 + n - 1, computed once and shared (never modified).  An env's trace does not
    depend on the vector it is stepped in, so a vector of N envs is the first N columns."""
    key = (policy, env_id0, n, steps, abandon_cap)
    if key not in _REFS:
        _REFS[key] = ref.stepper_traces(SEED, env_id0, n, ref.POLICIES[policy], steps, abandon_cap)
    return _REFS[key]


def _state_fields(buf, n):
    """The SoA state buffer of include/gymrl.h: f64 position, f64 velocity, f64 ep_ret, i32 ep_len, u32 episode, each [n] and
    padded to 256 bytes."""
    raw, off, out = buf.cpu().numpy(), 0, {}
    for name, dt in (("pos", np.float64), ("vel", np.float64), ("ep_ret", np.float64), ("ep_len", np.int32), ("episode", np.uint32)):
        nbytes = n * np.dtype(dt).itemsize
        out[name] = raw[off:off + nbytes].view(dt).copy()
        off += (nbytes + 255) & ~255
    assert off == raw.size
    return out


def _run_stepper(n, policy, steps, env_id0=0, abandon_cap=0):
    torch, ops, dev = _gpu()
    from gymrl_amd.envs import VecEnv
    env = VecEnv("MountainCar-v0", n, device=dev, seed=SEED, env_id0=env_id0)
    assert (env.obs_dim, env.act_dim, env.discrete, env.max_steps) == (2, 3, True, 200)
    z = lambda dt, *shape: torch.zeros(steps, n, *shape, dtype=dt, device=dev)   # noqa: E731
    out = dict(obs=z(torch.float32, 2), term_obs=z(torch.float32, 2), rew=z(torch.float32), terminated=z(torch.uint8), truncated=z(torch.uint8),
               done=z(torch.uint8), abandoned=z(torch.uint8), ep_ret_out=z(torch.float32), ep_len_out=z(torch.int32))
    obs_dev, term_dev = env.reset(), torch.empty(n, 2, device=dev)          # observation rows want 16-byte alignment: not a [t] slice
    obs0 = obs_dev.cpu().numpy()
    obs, act, states = obs0, ref.POLICIES[policy], []
    actions = np.zeros((steps, n), np.int32)
    for t in range(steps):
        actions[t] = ref.actions(obs, act)
        env.step(torch.from_numpy(actions[t]).to(dev), obs_dev, out["rew"][t], done_out=out["done"][t], term_obs_out=term_dev,
                 ep_ret_out=out["ep_ret_out"][t], ep_len_out=out["ep_len_out"][t], terminated_out=out["terminated"][t],
                 truncated_out=out["truncated"][t])
        if abandon_cap:
            env.abandon(abandon_cap, obs_dev, out["abandoned"][t], out["ep_ret_out"][t], out["ep_len_out"][t])
        out["obs"][t].copy_(obs_dev)
        out["term_obs"][t].copy_(term_dev)
        obs = obs_dev.cpu().numpy()
        states.append(_state_fields(env.state, n))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got.update(obs0=obs0, action=actions, ep_stats=env.ep_stats.cpu().numpy())
    for k in states[0]:
        got[k] = np.stack([s[k] for s in states])
    return got


def _assert_stepper(got, want, n, what):
    for k in ("obs0", "obs", "term_obs", "rew", "terminated", "truncated", "done", "abandoned", "ep_ret_out", "ep_len_out", "action",
              "pos", "vel", "ep_ret", "ep_len", "episode"):
        w = want[k][:n] if k == "obs0" else want[k][:, :n]
        assert got[k].dtype == w.dtype and np.array_equal(got[k], w), f"{what}: {k}"
    ended = (want["done"][:, :n] | want["abandoned"][:, :n]).astype(bool)
    stats = [float(ended.sum()), float(want["ep_ret_out"][:, :n][ended].astype(np.float64).sum()), float(want["ep_len_out"][:, :n][ended].sum())]
    assert got["ep_stats"].tolist() == stats, f"{what}: ep_stats"


@pytest.mark.parametrize("policy", ["rule", "pump", "pump-left"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])          # a lone lane, around the wave seam, two full waves and a ragged third
def test_stepper(n, policy):
    want = _ref_traces(policy)
    _assert_stepper(_run_stepper(n, policy, T_STEPS), want, n, f"{policy} N={n}")
    done = want["done"][:, :n]
    assert (done.sum(axis=0) >= 2).all()                                    # two auto-resets per env
    if policy == "rule":
        assert want["terminated"][:, :n].any() and (want["action"][:, :n] == 2).any() and (want["action"][:, :n] == 0).any()
    if policy == "pump":
        assert (want["pos"][:, :n] == -1.2).any() and want["terminated"][:, :n].any()
    if policy == "pump-left":
        assert (want["pos"][:, :n] == -1.2).any() and not want["terminated"][:, :n].any() and want["truncated"][:, :n].sum() == 2 * n


def test_abandon():
    want = _ref_traces("pump-left", steps=120, abandon_cap=50)
    assert (want["abandoned"].sum(axis=0) == 2).all() and not want["done"].any()
    _assert_stepper(_run_stepper(65, "pump-left", 120, abandon_cap=50), want, 65, "abandon(50)")


def _evaluate(E, coefs=None, start=None, cap=200, stream_id0=ref.EVAL_STREAM0):
    torch, ops, dev = _gpu()
    td = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)   # noqa: E731
    out = ops.mountaincar_rule_eval(E, SEED, stream_id0, cap, dev, coefs=td(coefs), start=td(start), want_final_state=True)
    return tuple(t.cpu().numpy() for t in out)


def _assert_eval(got, want, what):
    for g, w, name in zip(got, want, ("returns", "lengths", "reached", "final_state")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{what}: {name}"


@pytest.mark.parametrize("P,E", [(1, 1), (1, 10), (3, 43)])   # 129 lanes: both policy seams inside a wave, a ragged last block
def test_episode_kernel(P, E):
    coefs = None if P == 1 else np.array([ref.RULE_COEFS, NEVER_IN_BAND, PERTURBED])
    want = ref.eval_population(SEED, ref.EVAL_STREAM0, E, coefs)
    _assert_eval(_evaluate(E, coefs), want, f"P={P} E={E}")
    ret, length, reached, _ = want
    assert reached[0].all() and (ret == -length).all()
    if P == 3:
        assert (length[1] == 200).all() and not reached[1].any()            # never in band: action 0 for ever, truncated
        assert len(set(length[0].tolist())) > 1 and not np.array_equal(length[0], length[2])
        _assert_eval(_evaluate(E, coefs[:1]), tuple(w[:1] for w in want), "the reference's constants handed in")
        _assert_eval(_evaluate(E, None), tuple(w[:1] for w in want), "coefs = NULL")
        # a shard of the population is the population's lanes: policy 2's episodes from their own stream block
        part = _evaluate(E, coefs[2:], stream_id0=ref.EVAL_STREAM0 + 2 * E)
        _assert_eval(part, tuple(w[2:] for w in want), "stream_id0 shard")


def test_episode_kernel_cap():
    coefs = np.array([ref.RULE_COEFS, NEVER_IN_BAND, PERTURBED])
    want = ref.eval_population(SEED, ref.EVAL_STREAM0, 43, coefs, cap=50)
    _assert_eval(_evaluate(43, coefs, cap=50), want, "cap=50")
    assert (want[1] == 50).all() and not want[2].any()
    want = ref.eval_population(SEED, ref.EVAL_STREAM0, 43, coefs, cap=110)   # some lanes are through, some are cut
    assert 0 < want[2][0].sum() < 43
    _assert_eval(_evaluate(43, coefs, cap=110), want, "cap=110")


def test_episode_kernel_start_overrides():
    coefs = np.array([ALWAYS_RIGHT, NEVER_IN_BAND])
    start = np.broadcast_to(np.array(SEAM_STARTS), (2, len(SEAM_STARTS), 2)).copy()
    for cap in (1, 200):
        _assert_eval(_evaluate(len(SEAM_STARTS), coefs, start, cap), ref.eval_population(SEED, 0, len(SEAM_STARTS), coefs, start, cap), f"cap={cap}")
    _, length, reached, final = _evaluate(len(SEAM_STARTS), coefs, start, 1)
    assert (length == 1).all()
    assert final[1, 0].tolist() == [-1.2, 0.0] and reached[1, 0] == 0                       # pushed left into the wall
    assert final[0, 1].tolist() == [0.0699 + (0.001 + -0.0025), 0.0699 + (0.001 + -0.0025)]  # (0, 0.0699): gravity wins, no clamp
    assert final[0, 2].tolist() == [0.6, 0.07] and reached[0, 2] == 1                       # both clamps
    assert final[0, 3].tolist() == [0.45 + 0.07, 0.07] and reached[0, 3] == 1               # the speed clamp
    assert final[1, 4].tolist() == [-0.5 + -0.07, -0.07]                                    # ... downwards
    assert final[1, 5][0] >= 0.5 and final[1, 5][1] < 0.0 and reached[1, 5] == 0            # past the goal moving left


def test_episode_kernel_is_the_steppers_first_episode():
    """Episode i of the kernel = the first episode of env i of a VecEnv(seed, env_id0 = stream_id0) under the host policy."""
    n = 65
    got = _run_stepper(n, "rule", 200, env_id0=ref.EVAL_STREAM0)
    ret, length, reached, final = (a[0] for a in _evaluate(n))
    first = got["done"].argmax(axis=0)
    cols = np.arange(n)
    assert got["done"][first, cols].all()
    assert np.array_equal(got["ep_len_out"][first, cols], length) and np.array_equal(first + 1, length)
    assert np.array_equal(got["ep_ret_out"][first, cols].astype(np.float64), ret)
    assert np.array_equal(got["terminated"][first, cols], reached)
    assert np.array_equal(got["term_obs"][first, cols], final.astype(np.float32))
    live = first > 0                                                        # the float64 state one step before the end
    assert live.all()
    _, _, _, before = (a[0] for a in _evaluate_prefix(n, length - 1))
    assert np.array_equal(np.stack([got["pos"][first - 1, cols], got["vel"][first - 1, cols]], axis=1), before)


def _evaluate_prefix(n, caps):
    """Episode i cut after caps[i] steps: one launch per distinct cap, each lane taken from its own."""
    out = None
    for cap in sorted(set(caps.tolist())):
        got = _evaluate(n, cap=int(cap))
        out = [g.copy() for g in got] if out is None else out
        for o, g in zip(out, got):
            o[0, caps == cap] = g[0, caps == cap]
    return out


def _agent(**cfg):
    _gpu()
    from gymrl_amd.mountaincar_baseline import Config, RuleBasedAgent
    c = Config()
    for k, v in cfg.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    return RuleBasedAgent(c)


def test_agent_surface(capsys):
    agent = _agent()
    assert (agent.cfg.env_name, agent.cfg.seed, agent.cfg.test_episodes, agent.cfg.episode_cap) == ("MountainCar-v0", 42, 10, 200)
    ret, length, reached = agent.evaluate(1)
    assert ret.shape == length.shape == reached.shape == (1, 1)
    # the reference's loop through the single-env view is the kernel's episode of the same stream, each time it is called
    for _ in range(2):
        reward, steps = agent.run_episode()
        assert (reward, steps) == (float(ret[0, 0]), int(length[0, 0]))
    want = ref.eval_population(42, ref.EVAL_STREAM0, 10)
    rewards = agent.eval(10)
    assert rewards == want[0][0].tolist()
    text = capsys.readouterr().out
    assert "Environment: MountainCar-v0" in text and "Action space: Discrete(3)" in text
    assert f"  Episode 10: Reward = {want[0][0, 9]:.0f}, Steps = {want[1][0, 9]}" in text
    assert f"Evaluation: Mean Reward = {want[0].mean():.1f}, Mean Steps = {want[1].mean():.1f}" in text
    # select_action is the restated rule; a population of coefficient sets evaluates in one call
    g = np.load(f"{ROOT}/tests/golden/mountaincar_rule.npz")
    assert [agent.select_action(o) for o in g["obs"][:300]] == ref.actions(g["obs"][:300], ref.POLICIES["rule"]).tolist()
    coefs = np.array([ref.RULE_COEFS, NEVER_IN_BAND, PERTURBED])
    got = agent.evaluate(7, coefs)
    for g_, w in zip(got, ref.eval_population(42, ref.EVAL_STREAM0, 7, coefs)):
        assert np.array_equal(g_, w)
    cut = _agent(episode_cap=50).evaluate(3)
    assert (cut[1] == 50).all() and not cut[2].any()
    with pytest.raises(NotImplementedError):
        agent.run_episode(render=True)


def test_script_entry_point():
    r = subprocess.run([sys.executable, "-m", "gymrl_amd.mountaincar_baseline"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("  Episode ") and ": Reward = " in ln and ", Steps = " in ln]
    assert len(lines) == 10
    assert "Environment: MountainCar-v0" in r.stdout and "Evaluating for 10 episodes..." in r.stdout
    assert "Evaluation: Mean Reward = " in r.stdout and "Visual Test: Reward = " in r.stdout
