"""Acrobot-v1 on an MI355X: the batched stepper (csrc/env_classic.hip, kind 5) against tests/acrobot_ref.py.  The state is float64,
every operation of the RK4 step is spelled out in include/gymrl.h and sin / cos are the device's det_sincos restated on the host,
so every comparison is array_equal: observations, terminal observations, rewards, flags, episode returns and lengths, ep_stats and
the float64 state read back."""
import numpy as np
import pytest

import acrobot_ref as ref

pytestmark = pytest.mark.gpu

SEED, T_STEPS = 42, 40
N_RAGGED = 65                                          # kEnvBlock + 1: a full workgroup and one lane of a second
TERMINATOR = (3.0, 0.0, 0.0, 0.0)                      # env 0 of every run: over the line on its first step, then auto-reset
DEV = "cuda:0"


def _gpu():
    import torch
    from gymrl_amd import ops
    if not (torch.cuda.is_available() and ops.device_ok()):
        pytest.fail("gpu test without a usable MI355X")
    return torch, ops


_REFS = {}


def _ref_traces(policy, env_id0=0, abandon_cap=0):
    """Reference traces of N_RAGGED envs, computed once and shared (never modified).  An env's trace does not depend on the vector it
    is stepped in, so a vector of N envs is the first N columns."""
    key = (policy, env_id0, abandon_cap)
    if key not in _REFS:
        _REFS[key] = ref.stepper_traces(SEED, env_id0, N_RAGGED, ref.POLICIES[policy], T_STEPS, abandon_cap, starts={0: TERMINATOR})
    return _REFS[key]


def _state_fields(buf, n):
    """The SoA state buffer of include/gymrl.h: f64 th1, th2, dth1, dth2, ep_ret, i32 ep_len, u32 episode, each [n] and padded to
    256 bytes."""
    raw, off, out = buf.cpu().numpy(), 0, {}
    for name, dt in (("th1", np.float64), ("th2", np.float64), ("dth1", np.float64), ("dth2", np.float64), ("ep_ret", np.float64),
                     ("ep_len", np.int32), ("episode", np.uint32)):
        nbytes = n * np.dtype(dt).itemsize
        out[name] = raw[off:off + nbytes].view(dt).copy()
        off += (nbytes + 255) & ~255
    assert off == raw.size
    state = np.stack([out.pop(k) for k in ("th1", "th2", "dth1", "dth2")], axis=1)
    return dict(out, state=state)


def _run_stepper(n, policy, env_id0=0, abandon_cap=0):
    torch, ops = _gpu()
    from gymrl_amd.envs import VecEnv
    env = VecEnv("Acrobot-v1", n, device=DEV, seed=SEED, env_id0=env_id0)
    assert (env.obs_dim, env.act_dim, env.discrete, env.max_steps) == (6, 3, True, 500)
    steps = T_STEPS
    z = lambda dt, *shape: torch.zeros(steps, n, *shape, dtype=dt, device=DEV)   # noqa: E731
    out = dict(obs=z(torch.float32, 6), term_obs=z(torch.float32, 6), rew=z(torch.float32), terminated=z(torch.uint8), truncated=z(torch.uint8),
               done=z(torch.uint8), abandoned=z(torch.uint8), ep_ret_out=z(torch.float32), ep_len_out=z(torch.int32))
    obs_dev, term_dev = env.reset(), torch.empty(n, 6, device=DEV)          # observation rows want 16-byte alignment: not a [t] slice
    drawn = _state_fields(env.state, n)["state"]
    assert np.array_equal(drawn, np.array([ref.draw(SEED, env_id0 + i) for i in range(n)]))     # the reset draw, before env 0 is moved
    assert np.array_equal(obs_dev.cpu().numpy(), np.stack([ref.obs_of(y) for y in drawn]))
    pitch = (n * 8 + 255) & ~255
    for k, v in enumerate(TERMINATOR):                                      # env 0: lane 0 of each of the first four float64 fields
        env.state[k * pitch:k * pitch + 8].view(torch.float64).fill_(v)
    obs_dev[0].copy_(torch.from_numpy(ref.obs_of(TERMINATOR)))
    obs0 = obs_dev.cpu().numpy()
    obs, act, states = obs0, ref.POLICIES[policy], []
    actions = np.zeros((steps, n), np.int32)
    for t in range(steps):
        actions[t] = ref.actions(obs, act, t)
        env.step(torch.from_numpy(actions[t]).to(DEV), obs_dev, out["rew"][t], done_out=out["done"][t], term_obs_out=term_dev,
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
              "state", "ep_ret", "ep_len", "episode"):
        w = want[k][:n] if k == "obs0" else want[k][:, :n]
        assert got[k].dtype == w.dtype and got[k].shape == w.shape and np.array_equal(got[k], w), f"{what}: {k}"
    ended = (want["done"][:, :n] | want["abandoned"][:, :n]).astype(bool)
    stats = [float(ended.sum()), float(want["ep_ret_out"][:, :n][ended].astype(np.float64).sum()), float(want["ep_len_out"][:, :n][ended].sum())]
    assert got["ep_stats"].tolist() == stats, f"{what}: ep_stats"


@pytest.mark.parametrize("policy", ["pump", "idle", "cycle"])
@pytest.mark.parametrize("n", [1, N_RAGGED])
def test_stepper(n, policy):
    want = _ref_traces(policy)
    _assert_stepper(_run_stepper(n, policy), want, n, f"{policy} N={n}")
    # env 0 goes over the line on its first step: reward 0, an episode of length 1 and return 0, auto-reset into episode 1's draw
    assert want["terminated"][0, 0] == 1 and want["rew"][0, 0] == 0.0 and want["ep_len_out"][0, 0] == 1 and want["episode"][0, 0] == 1
    assert not np.array_equal(want["obs"][0, 0], want["term_obs"][0, 0]) and want["terminated"][1:].sum() == 0
    assert (want["rew"][1:] == -1.0).all() and not want["truncated"].any()
    if policy == "cycle":
        assert want["action"][:, 0].tolist() == [t % 3 for t in range(T_STEPS)]
    if policy == "pump" and n > 1:
        assert {0, 2} == set(want["action"][:, 1:n].ravel().tolist())


@pytest.mark.parametrize("cap", [1, 7])
def test_abandon(cap):
    want = _ref_traces("cycle", abandon_cap=cap)
    assert (want["abandoned"][:, 1:].sum(axis=0) == T_STEPS // cap).all() and want["done"].sum() == 1
    if cap == 7:                                                            # env 0: one step, the auto-reset, then 39 = 5 * 7 + 4
        assert want["abandoned"][:, 0].sum() == 5 and want["ep_len_out"][7, 0] == 7
    for n in (1, N_RAGGED):
        _assert_stepper(_run_stepper(n, "cycle", abandon_cap=cap), want, n, f"abandon({cap}) N={n}")


def test_env_ids_above_two_to_the_32():
    id0 = (1 << 33) + 5
    want = _ref_traces("pump", env_id0=id0)
    assert not np.array_equal(want["obs0"][1:], _ref_traces("pump")["obs0"][1:])      # the high word reaches the draw
    assert not np.array_equal(want["obs0"][1:], ref.stepper_traces(SEED, 5, 3, ref.pump, 1)["obs0"][1:])
    _assert_stepper(_run_stepper(N_RAGGED, "pump", env_id0=id0), want, N_RAGGED, "env_id0 = 2^33 + 5")
