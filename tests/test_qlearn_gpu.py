"""The tabular Q-learning kernels (csrc/tabular.hip) against tests/tabular_ref.py on an MI355X.  Every run is the reference's
float64 loop in the reference's operation order under the same counter-keyed draws, so every comparison is array_equal: tables,
episode rewards, lengths, action counts and episode counts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tabular_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

FROZEN_CFG = dict(seed=42, max_episodes=30, max_steps=100, lr=0.1, gamma=0.9, epsilon_start=0.95, epsilon_end=0.01, epsilon_decay=200)
CLIFF_CFG = dict(seed=42, max_episodes=40, max_steps=200, lr=0.1, gamma=0.9, epsilon_start=0.95, epsilon_end=0.01, epsilon_decay=300)


def _trainer(module, cfg, num_runs=1, run_id0=0, steps_per_launch=0, **more):
    import importlib
    import torch
    from gymrl_amd import ops
    if not (torch.cuda.is_available() and ops.device_ok()):
        pytest.fail("gpu test without a usable MI355X")
    mod = importlib.import_module("gymrl_amd." + module)
    c = mod.Config()
    for k, v in dict(cfg, num_runs=num_runs, run_id0=run_id0, steps_per_launch=steps_per_launch, **more).items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    return mod.QLearningTrainer(c)


def _frozen(cfg, num_runs=1, is_slippery=True, shaped=True, **kw):
    return _trainer("qlearning_frozenlake", cfg, num_runs, is_slippery=is_slippery, use_reward_shaping=shaped, **kw)


def _cliff(cfg, num_runs=1, **kw):
    return _trainer("qlearning_cliffwalking", cfg, num_runs, **kw)


def _assert_same(tr, want, what):
    R = tr.num_runs
    assert np.array_equal(np.asarray(tr.Q).reshape(want["Q"].shape), want["Q"]), f"{what}: Q"
    assert np.array_equal(np.asarray(tr.episode_rewards, np.float64).reshape(R, -1), want["rewards"]), f"{what}: episode rewards"
    assert np.array_equal(tr.episode_lengths, want["lengths"]), f"{what}: episode lengths"
    assert np.array_equal(tr.run_sample_counts, want["k"]), f"{what}: k"
    assert np.array_equal(tr.run_episodes, want["episodes"]), f"{what}: episodes"


_REFS = {}


def _ref(name, env, cfg, num_runs, run_id0=0):
    """A reference population, computed once and shared by the tests that compare with it (never modified)."""
    key = (name, num_runs, run_id0, tuple(sorted(cfg.items())))
    if key not in _REFS:
        _REFS[key] = ref.train_population(env, cfg, num_runs, run_id0)
    return _REFS[key]


@pytest.mark.parametrize("R", [1, 3, 65])        # 65: across the wave seam into a one-lane workgroup
def test_frozenlake_slippery_shaped(R):
    tr = _frozen(FROZEN_CFG, R)
    tr.train()
    _assert_same(tr, _ref("fl_ss", ref.FrozenLake(True, True), FROZEN_CFG, R), f"FrozenLake slippery shaped R={R}")
    assert (np.asarray(tr.Q).reshape(R, 16, 4) != 0).any()


def test_frozenlake_plain():
    tr = _frozen(FROZEN_CFG, 3, is_slippery=False, shaped=False)
    tr.train()
    _assert_same(tr, _ref("fl_pp", ref.FrozenLake(False, False), FROZEN_CFG, 3), "FrozenLake non-slippery unshaped")


@pytest.mark.parametrize("R,episodes", [(3, 40), (65, 5)])
def test_cliffwalking(R, episodes):
    cfg = dict(CLIFF_CFG, max_episodes=episodes)
    tr = _cliff(cfg, R)
    tr.train()
    _assert_same(tr, _ref("cw", ref.CliffWalking(), cfg, R), f"CliffWalking R={R}")


def test_chunk_seams_give_identical_bits():
    """steps_per_launch 7, 64 and the whole run: the record between launches continues every run bit for bit."""
    cfg = dict(FROZEN_CFG, max_episodes=12)
    want = _ref("fl_ss", ref.FrozenLake(True, True), cfg, 3)
    for chunk in (7, 64, 0):
        tr = _frozen(cfg, 3, steps_per_launch=chunk)
        tr.train()
        _assert_same(tr, want, f"FrozenLake steps_per_launch={chunk}")
    cfg = dict(CLIFF_CFG, max_episodes=4)
    want = _ref("cw", ref.CliffWalking(), cfg, 3)
    for chunk in (7, 64, 0):
        tr = _cliff(cfg, 3, steps_per_launch=chunk)
        tr.train()
        _assert_same(tr, want, f"CliffWalking steps_per_launch={chunk}")


def test_sharding_by_run_id0():
    """Runs 0..9 in one call = two calls of five with run_id0 0 and 5."""
    cfg = dict(FROZEN_CFG, max_episodes=12)
    whole = _frozen(cfg, 10)
    whole.train()
    _assert_same(whole, _ref("fl_ss", ref.FrozenLake(True, True), cfg, 10), "runs 0..9")
    for id0 in (0, 5):
        part = _frozen(cfg, 5, run_id0=id0)
        part.train()
        assert np.array_equal(part.Q, whole.Q[id0:id0 + 5])
        assert np.array_equal(part.episode_rewards, whole.episode_rewards[id0:id0 + 5])
        assert np.array_equal(part.episode_lengths, whole.episode_lengths[id0:id0 + 5])
        assert np.array_equal(part.run_sample_counts, whole.run_sample_counts[id0:id0 + 5])


def test_never_done():
    """CliffWalking, epsilon 0, zero table, 2 episodes of 50 steps (tests/test_tabular_ref.py: within that budget the greedy walk
    never reaches the goal): every episode ends at max_steps without a done flag, every update uses the non-terminal target."""
    cfg = dict(CLIFF_CFG, max_episodes=2, max_steps=50, epsilon_start=0.0, epsilon_end=0.0)
    want = _ref("cw", ref.CliffWalking(), cfg, 3)
    assert want["never_done"] and (want["lengths"] == 50).all()
    tr = _cliff(cfg, 3)
    tr.train()
    _assert_same(tr, want, "never done")
    assert (tr.episode_lengths == 50).all() and (tr.run_sample_counts == 100).all()
    first = _cliff(dict(cfg, max_episodes=1, max_steps=1), 1)
    first.train()
    assert first.Q[36, 0] == 0.0 + 0.1 * ((-1.0 + 0.9 * 0.0) - 0.0)
    assert np.count_nonzero(first.Q) == 1


def _cliff_table(first_action):
    Q = np.zeros((48, 4))
    Q[36, first_action] = 1.0
    for s in range(24, 35):
        Q[s, 1] = 1.0                       # eleven RIGHT along the row above the cliff
    Q[35, 2] = 1.0                          # DOWN into the goal
    return Q


def test_evaluation_cliffwalking_hand_tables():
    tr = _cliff(CLIFF_CFG, 1)
    tr.Q = _cliff_table(0)                  # UP, eleven RIGHT, DOWN
    returns, lengths, finished = tr._evaluate(4, tr.cfg.max_steps)
    assert (returns == -13.0).all() and (lengths == 13).all() and (finished == 1).all()
    assert tr.eval(3) == [-13.0, -13.0, -13.0] and tr.eval_finished.all()
    tr.Q = _cliff_table(3)                  # LEFT at the start: stays on 36 for ever
    returns, lengths, finished = tr._evaluate(4, tr.cfg.max_steps)
    assert (returns == -200.0).all() and tr.cfg.max_steps == 200 and (lengths == 200).all() and (finished == 0).all()
    tr.eval(2)
    assert not tr.eval_finished.any()


def test_evaluation_frozenlake():
    # non-slippery: DOWN DOWN RIGHT RIGHT DOWN RIGHT = 0 4 8 9 10 14 15
    Q = np.zeros((16, 4))
    for s, a in ((0, 1), (4, 1), (8, 2), (9, 2), (10, 1), (14, 2)):
        Q[s, a] = 1.0
    tr = _frozen(FROZEN_CFG, 1, is_slippery=False)
    tr.Q = Q
    returns, lengths, success = tr._evaluate(20, 100)
    assert (returns == 1.0).all() and (lengths == 6).all() and (success == 1).all()
    # slippery, on trained tables of three runs: the reference's episodes one by one
    tr = _frozen(FROZEN_CFG, 3)
    tr.train()
    got = tr._evaluate(20, 100)
    want = ref.eval_population(ref.FrozenLake(True, True), tr.Q, 42, 20, 100)
    for g, w, name in zip(got, want, ("returns", "lengths", "success")):
        assert np.array_equal(g, w), name
    assert len({tuple(r) for r in got[1].tolist()}) > 1          # the runs' episodes differ: the streams do
    # a shard's evaluation streams are the whole population's
    part = _frozen(FROZEN_CFG, 1, run_id0=2)
    part.Q = tr.Q[2]
    for g, w in zip(part._evaluate(20, 100), got):
        assert np.array_equal(g[0], w[2])


@pytest.mark.parametrize("module", ["qlearning_frozenlake", "qlearning_cliffwalking"])
def test_default_config_end_to_end(module):
    """One run of each script at its own Config: tables and the 500 episode rewards equal the reference's, and the kernel's greedy
    evaluation agrees with the reference's own.  No return value is fixed in advance; the one reached is recorded."""
    tr = _trainer(module, {})
    cfg = {k: getattr(tr.cfg, k) for k in FROZEN_CFG}
    env = ref.FrozenLake(tr.cfg.is_slippery, tr.cfg.use_reward_shaping) if module.endswith("frozenlake") else ref.CliffWalking()
    assert cfg["max_episodes"] == 500
    tr.train()
    _assert_same(tr, _ref(module, env, cfg, 1), module)
    cap = 100 if module.endswith("frozenlake") else tr.cfg.max_steps
    got = tr._evaluate(20, cap)
    want = ref.eval_population(env, tr.Q, tr.cfg.seed, 20, cap)
    for g, w, name in zip(got, want, ("returns", "lengths", "flags")):
        assert np.array_equal(g, w), name
    out = os.path.join(ROOT, "profiles", "qlearn_micro.jsonl")
    if os.environ.get("GYMRL_QLEARN_RECORD"):
        with open(out, "a") as f:
            f.write(json.dumps({"what": "default_config_greedy_eval", "script": module, "runs": 1, "train_actions": int(tr.sample_count),
                                "last_50_train_reward_mean": float(np.mean(tr.episode_rewards[-50:])),
                                "eval_return_mean": float(got[0].mean()), "eval_goal_rate": float(got[2].mean())}) + "\n")


def test_visual_episode_is_not_an_evaluation_episode_again():
    """test()'s extra greedy episode draws from its own stream block: on slippery FrozenLake it is the reference's episode of
    that stream, not eval()'s first episode replayed."""
    from gymrl_amd.tabular import VISUAL_STREAM_OFFSET
    tr = _frozen(FROZEN_CFG, 1)
    tr.train()
    env = ref.FrozenLake(True, True)
    got = tr._evaluate(1, 100, VISUAL_STREAM_OFFSET)
    want = ref.eval_episode(env, tr.Q.tolist(), 42, ref.EVAL_STREAM0 + VISUAL_STREAM_OFFSET, 100)
    assert (float(got[0][0, 0]), int(got[1][0, 0]), bool(got[2][0, 0])) == want
    assert VISUAL_STREAM_OFFSET >= 1 << 39                       # beyond run_id * episodes + episode of any evaluation


def test_script_entry_point_prints_progress():
    r = subprocess.run([sys.executable, "-m", "gymrl_amd.qlearning_cliffwalking", "--num_runs", "4", "--max_episodes", "20"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Environment: CliffWalking-v0" in r.stdout and "States: 48, Actions: 4" in r.stdout
    assert "Episode 20/20 | Reward: " in r.stdout and "Avg(20): " in r.stdout and "Epsilon: " in r.stdout
    assert "Training completed!" in r.stdout and "Evaluation: Mean = " in r.stdout and "Visual Test: Reward = " in r.stdout


def test_select_action_and_update_restate_one_reference_step():
    cfg = dict(FROZEN_CFG, max_episodes=1, max_steps=1)
    env = ref.FrozenLake(True, True)
    want = ref.train_run(env, cfg, 0)
    tr = _frozen(cfg, 1)
    state = 0
    action = tr.select_action(state)
    u, explore, slip = ref.step_draw(42, 0, 1)
    assert tr.sample_count == 1 and tr.epsilon == ref.epsilon(cfg, 1)
    assert action == (explore if u < ref.epsilon(cfg, 1) else 0)
    nxt, reward, terminated, truncated = env.step(state, action, slip, 0)
    shaped = tr._shape_reward(state, nxt, reward, terminated or truncated)
    assert shaped == env.train_reward(state, nxt, reward)
    tr.update(state, action, shaped, nxt, terminated or truncated)
    assert np.array_equal(tr.Q, np.array(want["Q"]))
    assert tr.select_action(0, deterministic=True) == ref.greedy(want["Q"][0]) and tr.sample_count == 1
    # ... and the device takes the same step
    dev = _frozen(cfg, 1)
    dev.train()
    assert np.array_equal(dev.Q, tr.Q) and dev.sample_count == 1
    many = _frozen(cfg, 4)
    with pytest.raises(RuntimeError, match="num_runs == 1"):
        many.select_action(0)
    with pytest.raises(RuntimeError, match="num_runs == 1"):
        many.update(0, 0, -1.0, 1, False)
