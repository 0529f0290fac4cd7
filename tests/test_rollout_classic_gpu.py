"""gymrl_rollout_classic on an MI355X (csrc/rollout_classic.hip): PPOTrainer on MountainCar-v0 and Acrobot-v1 with one launch per
chunk writes the slab, bootstrap value, GAE chunk maps, env state and episode statistics of the step-by-step sequence
gymrl_mlp_forward -> gymrl_categorical_sample -> gymrl_env_step, bit for bit — the contract
tests/test_hip_parity.py::test_persistent_rollout_cartpole_bit_identical_to_stepwise holds gymrl_rollout_cartpole to.

Random play on these two envs ends at the TimeLimit only, so every rollout's reset is followed by the same few writes into both
trainers' state buffers (the SoA layout of include/gymrl.h): env 0 and the last env (the ragged workgroup's) start where the next
step terminates, env 1 starts three steps in front of the TimeLimit."""
import numpy as np
import pytest

import acrobot_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# name -> (TimeLimit, float64 state fields in front of ep_ret, the planted state, its float32 observation)
ENVS = {
    "MountainCar-v0": (200, 2, (0.45, 0.06), lambda y: np.asarray(y, np.float64).astype(np.float32)),
    "Acrobot-v1": (500, 4, (3.0, 0.0, 0.0, 0.0), acrobot_ref.obs_of),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from gymrl_amd import ops
    assert ops.device_ok(), "libgymrl_hip.so did not find a gfx950 device"
    return torch.device("cuda:0")


def _plant_after_reset(tr, planted_len):
    """Every env.reset() of the trainer is followed by the planted starts, written into the state buffer and the observation row."""
    env, n = tr.env, tr.env.n
    cap, n_state, start, obs_of = ENVS[env.name]
    pitch = (n * 8 + 255) & ~255                                            # every [n] field is padded to 256 bytes
    len_at = (n_state + 1) * pitch                                          # ep_len i32[n] follows the state fields and ep_ret
    obs_row = torch.from_numpy(obs_of(start)).to(env.device)
    reset = env.reset

    def reset_and_plant(obs_out=None, seed=None):
        out = reset(obs_out, seed=seed)
        for i in (0, n - 1):
            for k, v in enumerate(start):
                env.state[k * pitch + 8 * i:k * pitch + 8 * i + 8].view(torch.float64).fill_(v)
            out[i].copy_(obs_row)
        env.state[len_at + 4:len_at + 8].view(torch.int32).fill_(planted_len)   # env 1: its observation does not carry the length
        return out
    env.reset = reset_and_plant


def _episode_lengths(dones, planted_len):
    """Lengths of the episodes that ended inside a rollout that began with a reset: dones u8[T, N] -> list."""
    d = dones.cpu().numpy().astype(bool)
    out = []
    for i in range(d.shape[1]):
        at = np.flatnonzero(d[:, i])
        if at.size:
            out.append(int(at[0]) + 1 + (planted_len if i == 1 else 0))
            out.extend(np.diff(at).tolist())
    return out


@pytest.mark.parametrize("env_name,N,T,chunk,hidden", [
    ("MountainCar-v0", 40, 210, 16, 64), ("MountainCar-v0", 48, 30, 1, 32),
    ("Acrobot-v1", 24, 520, 64, 32), ("Acrobot-v1", 40, 48, 7, 64), ("Acrobot-v1", 256, 32, 0, 256)])
def test_persistent_rollout_bit_identical_to_stepwise(dev, env_name, N, T, chunk, hidden):
    """T past the TimeLimit (210 > 200, 520 > 500), a ragged last workgroup (N = 40, 24), chunks that do not align with T or with
    the GAE chunk of 16 (16 into 210, 7), one-step launches (chunk 1), the whole rollout in one launch at hidden 256 (chunk 0)."""
    from gymrl_amd import ops
    from gymrl_amd.ppo_lunarlander import Config, PPOTrainer
    cap = ENVS[env_name][0]
    planted_len = cap - 3

    def make(persistent):
        cfg = Config()
        cfg.env_name = env_name
        cfg.num_envs, cfg.update_freq, cfg.num_epochs, cfg.num_minibatches, cfg.seed = N, T, 1, 2, 11
        cfg.hidden_dim, cfg.persistent_rollout, cfg.rollout_chunk = hidden, persistent, chunk
        tr = PPOTrainer(cfg)
        _plant_after_reset(tr, planted_len)
        return tr
    a, b = make(True), make(False)
    assert a._persistent_ok() and not b._persistent_ok()
    assert a.env.kind in (ops.MOUNTAINCAR, ops.ACROBOT) and a.env.max_steps == cap
    for rollout in range(2):
        nva, nvb = a.collect_rollout(), b.collect_rollout()
        assert torch.equal(nva, nvb)                                        # the bootstrap value
        ba, bb = a.buffer, b.buffer
        for name in ("states", "actions", "log_probs", "values", "rewards", "dones"):
            assert torch.equal(getattr(ba, name), getattr(bb, name)), (rollout, name)
        d = ba.dones.bool()
        lengths = _episode_lengths(ba.dones, planted_len)
        assert any(n < cap for n in lengths), "the rollout must contain an episode that terminated"
        assert any(n == cap for n in lengths) and max(lengths) == cap, "the rollout must contain an episode the TimeLimit ended"
        assert torch.equal(ba.ep_returns[d], bb.ep_returns[d])
        assert torch.equal(a.env.state, b.env.state), rollout
        assert torch.equal(a.env.ep_stats, b.env.ep_stats) and int(a.env.ep_stats[0]) > 0
        adv_a, ret_a = a.compute_gae()
        adv_b, ret_b = b.compute_gae()
        assert torch.equal(adv_a, adv_b) and torch.equal(ret_a, ret_b) and torch.equal(a._moments, b._moments)
    a.update(a.collect_rollout()), b.update(b.collect_rollout())
    assert torch.equal(a.flat_params, b.flat_params)


def test_cartpole_through_the_new_entry_is_the_old_entry(dev, monkeypatch):
    """gymrl_rollout_classic(GYMRL_ENV_CARTPOLE) launches gymrl_rollout_cartpole's kernel: the same rollout from the same start."""
    from gymrl_amd import ops
    from gymrl_amd.ppo_lunarlander import Config, PPOTrainer

    def make():
        cfg = Config()
        cfg.env_name = "CartPole-v1"
        cfg.num_envs, cfg.update_freq, cfg.num_epochs, cfg.num_minibatches, cfg.seed = 40, 32, 1, 2, 11
        cfg.hidden_dim, cfg.persistent_rollout, cfg.rollout_chunk = 64, True, 16
        return PPOTrainer(cfg)
    a, b = make(), make()
    assert a._persistent_ok() and b._persistent_ok()
    nva = a.collect_rollout().clone()
    calls = []

    def through_classic(*args, **kw):
        calls.append(kw.get("ep_stats") is not None)
        return ops.rollout_classic(ops.CARTPOLE, *args, **kw)
    monkeypatch.setattr(ops, "rollout_cartpole", through_classic)
    nvb = b.collect_rollout()
    assert len(calls) == 2                                                  # 32 steps in chunks of 16
    assert torch.equal(nva, nvb)
    for name in ("states", "actions", "log_probs", "values", "rewards", "dones"):
        assert torch.equal(getattr(a.buffer, name), getattr(b.buffer, name)), name
    d = a.buffer.dones.bool()
    assert int(d.sum()) > 0 and torch.equal(a.buffer.ep_returns[d], b.buffer.ep_returns[d])
    assert torch.equal(a.env.state, b.env.state) and torch.equal(a.env.ep_stats, b.env.ep_stats)
    adv_a, ret_a = a.compute_gae()
    adv_b, ret_b = b.compute_gae()
    assert torch.equal(adv_a, adv_b) and torch.equal(ret_a, ret_b) and torch.equal(a._moments, b._moments)
