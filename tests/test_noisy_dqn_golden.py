"""NoisyNet dueling DQN without a GPU: the module's surface, and tests/noisy_dqn_ref.py (numpy float32) against the golden
recorded from the reference's own update() (tests/golden/make_golden_noisy_dqn.py): fed the golden's raw draws and sample
order it reproduces both updates and both select_action modes.  The bars are the ones tests/test_trainers_gpu.py holds the
DQN and Rainbow goldens to: loss within 1e-5 relative, parameters within 2e-6 after each Adam step."""
import os

import numpy as np
import pytest

import noisy_dqn_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noisy_dqn_update.npz")
LOSS_RTOL, PARAM_ATOL = 1e-5, 2e-6


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def params(g, prefix):
    return {k[len(prefix):]: g[k].copy() for k in g if k.startswith(prefix)}


def test_module_imports_and_config_is_the_references():
    from gymrl_amd import noisy_dqn_cartpole as m
    cfg = m.Config()
    want = dict(env_name="CartPole-v1", seed=None, max_episodes=500, max_steps=10000, batch_size=64, gamma=0.99, lr=0.001,
                target_update_freq=500, memory_capacity=10000, hidden_dim=64, sigma_init=0.5)
    for k, v in want.items():
        assert getattr(cfg, k) == v, k
    assert (cfg.num_envs, cfg.updates_per_step, cfg.use_graphs, cfg.fused_step, cfg.chunk_steps) == (1, 1, True, False, 16)
    for name in ("NoisyLinear", "NoisyDuelingQNetwork", "ReplayBuffer", "NoisyDQNTrainer"):
        assert hasattr(m, name)


def test_state_dict_keys_and_shapes_equal_the_goldens(golden):
    from gymrl_amd.noisy_dqn_cartpole import NoisyDuelingQNetwork
    want = params(golden, "p0_")
    H, D = want["fc1.weight_mu"].shape
    net = NoisyDuelingQNetwork(D, want["advantage_stream.weight_mu"].shape[0], H, float(golden["sigma_init"]))
    sd = net.state_dict()
    assert list(sd) == list(want)
    for k, v in sd.items():
        assert tuple(v.shape) == want[k].shape, k
    import torch
    net.load_state_dict({k: torch.from_numpy(v) for k, v in want.items()})      # a reference checkpoint loads
    # the reference's init: sigma = sigma_init / sqrt(fan), mu within +-1 / sqrt(in)
    fresh = NoisyDuelingQNetwork(D, 2, H, 0.5).state_dict()
    assert np.allclose(fresh["fc2.weight_sigma"].numpy(), 0.5 / np.sqrt(H)) and np.allclose(fresh["fc2.bias_sigma"].numpy(), 0.5 / np.sqrt(H))
    assert np.allclose(want["fc1.weight_sigma"], 0.5 / np.sqrt(D)) and np.allclose(want["value_stream.bias_sigma"], 0.5)
    assert float(fresh["fc1.weight_mu"].abs().max()) <= 1 / np.sqrt(D)


def test_numpy_restatement_reproduces_both_updates(golden):
    g = golden
    p, t = params(g, "p0_"), params(g, "t0_")
    adam = R.new_adam(p)
    D, H, A = R.dims_of(p)
    L = R.raw_len(D, H, A)
    assert g["raw"].shape == (2, 2 * L)
    for u in range(2):
        o = g["order"][u]
        batch = tuple(g[k][o] for k in ("states", "actions", "rewards", "next_states", "dones"))
        loss, q_mean = R.update(p, t, adam, batch, g["raw"][u][:L], g["raw"][u][L:], float(g["gamma"]), float(g["lr"]))
        print(f"update {u}: loss {loss!r} golden {g['loss'][u]!r}")
        assert abs(loss - g["loss"][u]) <= LOSS_RTOL * abs(g["loss"][u])
        assert abs(q_mean - g["q_mean"][u]) <= 1e-5 * max(1.0, abs(g["q_mean"][u]))
        want = params(g, f"p{u + 1}_")
        for k in p:
            if R._trainable(k):
                err = float(np.abs(p[k] - want[k]).max())
                assert err <= PARAM_ATOL, (u, k, err)
    moved = max(float(np.abs(p[k] - g["p0_" + k]).max()) for k in p if k.endswith("_sigma"))
    assert moved > 100 * PARAM_ATOL            # sigma learns: the bar is far below what two steps change


def test_numpy_restatement_reproduces_both_select_action_modes(golden):
    g = golden
    p = params(g, "p2_")
    assert abs(g["act_q_noisy"][0] - g["act_q_noisy"][1]) > 1e-4 and abs(g["act_q_det"][0] - g["act_q_det"][1]) > 1e-4
    a, q = R.select_action(p, g["act_state"], g["act_raw"])
    assert a == int(g["act_noisy"]) and np.abs(q - g["act_q_noisy"]).max() <= 1e-5
    a, q = R.select_action(p, g["act_state"])
    assert a == int(g["act_det"]) and np.abs(q - g["act_q_det"]).max() <= 1e-5
