"""SARSA, Expected SARSA and Double Q-learning (csrc/tabular.hip: gymrl_tabular_train) against tests/tabular_td_ref.py on an
MI355X.  Every run is the header's float64 loop in its operation order under the same counter-keyed draws, so every comparison
is array_equal: both tables, episode rewards, lengths, draw counts and episode counts.  The shapes are chosen for where the
kernel can go wrong, not for learning: a ragged second workgroup, episodes that run out at max_steps (SARSA drops a drawn
action), launch seams that divide nothing, planted ties."""
import numpy as np
import pytest

import tabular_ref as ref
import tabular_td_ref as td

pytestmark = pytest.mark.gpu

FROZEN_CFG = dict(seed=42, max_episodes=10, max_steps=24, lr=0.1, gamma=0.9, epsilon_start=0.95, epsilon_end=0.01, epsilon_decay=200)
CLIFF_CFG = dict(seed=42, max_episodes=6, max_steps=25, lr=0.1, gamma=0.9, epsilon_start=0.95, epsilon_end=0.01, epsilon_decay=300)
RULES = ("sarsa", "expected_sarsa", "double_q")
# name -> (module, reference env, the trainer's flags)
ENVS = {"cliff": ("sarsa_cliffwalking", ref.CliffWalking(), {}),
        "fl_slip_shaped": ("sarsa_frozenlake", ref.FrozenLake(True, True), dict(is_slippery=True, use_reward_shaping=True)),
        "fl_slip_plain": ("sarsa_frozenlake", ref.FrozenLake(True, False), dict(is_slippery=True, use_reward_shaping=False)),
        "fl_firm_shaped": ("sarsa_frozenlake", ref.FrozenLake(False, True), dict(is_slippery=False, use_reward_shaping=True)),
        "fl_firm_plain": ("sarsa_frozenlake", ref.FrozenLake(False, False), dict(is_slippery=False, use_reward_shaping=False))}


def _cfg(env):
    return CLIFF_CFG if env == "cliff" else FROZEN_CFG


def _trainer(rule, env, cfg, num_runs=1, steps_per_launch=0, run_id0=0):
    import importlib
    import torch
    from gymrl_amd import ops
    if not (torch.cuda.is_available() and ops.device_ok()):
        pytest.fail("gpu test without a usable MI355X")
    module, _, flags = ENVS[env]
    mod = importlib.import_module("gymrl_amd." + module)
    c = mod.Config()
    for k, v in dict(cfg, rule=rule, num_runs=num_runs, steps_per_launch=steps_per_launch, run_id0=run_id0, **flags).items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    return mod.TDTrainer(c)


_REFS = {}


def _ref(rule, env, cfg, num_runs, start=None):
    """A reference population, computed once and shared by the tests that compare with it (never modified).  start: None or
    (name, Q [R][S][4], Q2 or None) planted tables."""
    key = (rule, env, num_runs, tuple(sorted(cfg.items())), start and start[0])
    if key not in _REFS:
        Q, Q2 = (None, None) if start is None else start[1:]
        _REFS[key] = td.train_population(td.RULES[rule], ENVS[env][1], cfg, num_runs, Q=Q, Q2=Q2 if rule == "double_q" else None)
    return _REFS[key]


def _assert_same(tr, want, what):
    R = tr.num_runs
    assert np.array_equal(np.asarray(tr.Q).reshape(want["Q"].shape), want["Q"]), f"{what}: Q"
    if want["Q2"] is None:
        assert tr.Q2 is None
    else:
        assert np.array_equal(np.asarray(tr.Q2).reshape(want["Q2"].shape), want["Q2"]), f"{what}: Q2"
    assert np.array_equal(np.asarray(tr.episode_rewards, np.float64).reshape(R, -1), want["rewards"]), f"{what}: episode rewards"
    assert np.array_equal(tr.episode_lengths, want["lengths"]), f"{what}: episode lengths"
    assert np.array_equal(tr.run_sample_counts, want["k"]), f"{what}: k"
    assert np.array_equal(tr.run_episodes, want["episodes"]), f"{what}: episodes"


CASES = [(env, R) for env in ENVS for R in (1, 65)]          # 65: across the wave seam into a one-lane workgroup


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("env,R", CASES)
def test_rule_on_env(rule, env, R):
    cfg = _cfg(env)
    tr = _trainer(rule, env, cfg, R)
    tr.train()
    want = _ref(rule, env, cfg, R)
    _assert_same(tr, want, f"{rule} {env} R={R}")
    assert env.endswith("_plain") or (want["Q"] != 0).any()  # the env's own reward is 0 until a run reaches the goal
    if env == "cliff":                                       # every episode runs out at max_steps; SARSA has drawn one action more
        assert (want["lengths"] == cfg["max_steps"]).all()
        assert (want["k"] == cfg["max_episodes"] * (cfg["max_steps"] + (rule == "sarsa"))).all()
    elif R == 65:                                            # FrozenLake: episodes of both kinds
        assert (want["lengths"] == cfg["max_steps"]).any() and (want["lengths"] < cfg["max_steps"]).any()


def test_double_q_cliffwalking_deals_32_runs_to_a_workgroup():
    """33 runs: two workgroups of that instance, the second with one run."""
    tr = _trainer("double_q", "cliff", CLIFF_CFG, 33)
    tr.train()
    want = _ref("double_q", "cliff", CLIFF_CFG, 33)
    _assert_same(tr, want, "double_q cliff R=33")
    assert (want["Q"][32] != 0).any() and (want["Q2"][32] != 0).any() and not np.array_equal(want["Q"][31], want["Q"][32])


def _seam_after_last_step(rule, want, chunk):
    """Does a launch seam (every `chunk` iterations = draws) fall right behind an episode's last step, for some run?  Behind a
    done step SARSA's iteration has also drawn the next episode's first action."""
    hits = 0
    for lengths, draws, k in zip(want["lengths"], want["draws"], want["k"]):
        at, iters = 0, []
        for e, (n, d) in enumerate(zip(lengths, draws)):
            at += d
            iters.append(at + (1 if rule == "sarsa" and d == n and e + 1 < len(lengths) else 0))
        hits += sum(i % chunk == 0 and i < k for i in iters)
    return hits


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("env", ["cliff", "fl_slip_shaped"])
def test_launch_seams_give_identical_bits(rule, env):
    """steps_per_launch = 7 divides neither an episode nor the run: SARSA's pending action and both Double-Q tables cross the
    seams, also where one falls right behind an episode's last step."""
    cfg = _cfg(env)
    want = _ref(rule, env, cfg, 3)
    tr = _trainer(rule, env, cfg, 3, steps_per_launch=7)
    tr.train()
    _assert_same(tr, want, f"{rule} {env} steps_per_launch=7")
    whole = _trainer(rule, env, cfg, 3)
    whole.train()
    _assert_same(whole, want, f"{rule} {env} one launch")
    if env != "cliff":                                       # CliffWalking's 25 steps / 26 draws an episode meet a multiple of 7 at the 7th
        assert _seam_after_last_step(rule, want, 7) > 0


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("eps", [0.0, 1.0])
def test_epsilon_tables_of_all_zero_and_all_one(rule, eps):
    for env in ("cliff", "fl_slip_plain"):
        cfg = dict(_cfg(env), epsilon_start=eps, epsilon_end=eps)
        assert {ref.epsilon(cfg, k) for k in (1, 77, 5000)} == {eps}
        tr = _trainer(rule, env, cfg, 3)
        tr.train()
        _assert_same(tr, _ref(rule, env, cfg, 3), f"{rule} {env} eps={eps}")


def _planted(n_states, R):
    """Starting tables with ties at planted values: small dyadic numbers, many equal within a row and across the two tables."""
    rng = np.random.RandomState(7)
    Q = rng.randint(-2, 3, size=(R, n_states, 4)) * 0.25
    Q2 = rng.randint(-2, 3, size=(R, n_states, 4)) * 0.25
    return Q, Q2


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("env", ["cliff", "fl_slip_shaped"])
def test_nonzero_starting_tables(rule, env):
    cfg, R = _cfg(env), 5
    Q, Q2 = _planted(ENVS[env][1].n_states, R)
    assert any(len(set(row)) < 4 for row in Q[0].tolist())
    tr = _trainer(rule, env, cfg, R)
    tr.Q = Q.copy()
    if rule == "double_q":
        tr.Q2 = Q2.copy()
    tr.train()
    _assert_same(tr, _ref(rule, env, cfg, R, start=("planted", Q, Q2)), f"{rule} {env} planted tables")


@pytest.mark.parametrize("env", ["cliff", "fl_slip_shaped"])
def test_rule_0_is_the_qlearning_kernel(env):
    import importlib
    cfg = _cfg(env)
    new = _trainer("qlearning", env, cfg, 65, steps_per_launch=7)
    new.train()
    module, ref_env, flags = ENVS[env]
    mod = importlib.import_module("gymrl_amd." + module.replace("sarsa", "qlearning"))
    c = mod.Config()
    for k, v in dict(cfg, num_runs=65, **flags).items():
        setattr(c, k, v)
    old = mod.QLearningTrainer(c)
    old.train()
    for name in ("Q", "episode_rewards", "episode_lengths", "run_sample_counts", "run_episodes"):
        assert np.array_equal(getattr(new, name), getattr(old, name)), name
    want = ref.train_population(ref_env, cfg, 65)
    assert np.array_equal(new.Q, want["Q"]) and np.array_equal(new.run_sample_counts, want["k"]) and new.Q2 is None


def test_double_q_evaluates_on_the_sum_of_its_tables(capsys):
    import torch
    from gymrl_amd import ops
    from gymrl_amd.tabular import EVAL_STREAM0
    tr = _trainer("double_q", "fl_slip_shaped", FROZEN_CFG, 3)
    tr.train()
    assert (tr.Q != tr.Q2).any()
    both = torch.from_numpy(tr.Q + tr.Q2).cuda()
    want = ops.qlearn_eval(ops.FROZENLAKE, both, 20, 42, EVAL_STREAM0, 100, is_slippery=True)
    got = tr._evaluate(20, 100)
    for g, w, name in zip(got, want, ("returns", "lengths", "success")):
        assert np.array_equal(g, w.cpu().numpy()), name
    host = ref.eval_population(ref.FrozenLake(True, True), tr.Q + tr.Q2, 42, 20, 100)
    for g, w in zip(got, host):
        assert np.array_equal(g, w)
    assert np.array_equal(tr.eval(20), got[0])
    tr.test()
    assert "Visual Test: " in capsys.readouterr().out
    cw = _trainer("double_q", "cliff", CLIFF_CFG, 2)
    cw.train()
    cw.test()
    assert "Visual Test: Reward = " in capsys.readouterr().out


@pytest.mark.parametrize("rule", RULES + ("qlearning",))
@pytest.mark.parametrize("env", ["cliff", "fl_slip_shaped"])
def test_host_select_action_and_update_replay_a_device_run(rule, env):
    """num_runs = 1: the trainer's host restatement, driven like the header's loop, ends on the device run's bits after 3 episodes."""
    cfg = dict(_cfg(env), max_episodes=3)
    dev = _trainer(rule, env, cfg, 1, run_id0=4)
    dev.train()
    tr = _trainer(rule, env, cfg, 1, run_id0=4)
    world = ENVS[env][1]
    slip_of = lambda k: ref.step_draw(cfg["seed"], 4, k)[2]  # noqa: E731
    rewards, lengths = [], []
    for _ in range(3):
        s, ret, steps = world.start, 0.0, 0
        if rule == "sarsa":
            a = tr.select_action(s)
            slip = slip_of(tr.sample_count)
        for _ in range(cfg["max_steps"]):
            if rule != "sarsa":
                a = tr.select_action(s)
                slip = slip_of(tr.sample_count)
            s2, r, terminated, truncated = world.step(s, a, slip, steps)
            done = terminated or truncated
            r = world.train_reward(s, s2, r)
            if rule == "sarsa":
                a2 = None if done else tr.select_action(s2)
                tr.update(s, a, r, s2, done, a2)
                slip = slip_of(tr.sample_count)
            else:
                tr.update(s, a, r, s2, done)
            ret, steps = ret + r, steps + 1
            if done:
                break
            s = s2
            if rule == "sarsa":
                a = a2
        rewards.append(ret)
        lengths.append(steps)
    assert np.array_equal(tr.Q, dev.Q) and tr.sample_count == dev.sample_count
    assert (tr.Q2 is None and dev.Q2 is None) if rule != "double_q" else np.array_equal(tr.Q2, dev.Q2)
    assert rewards == dev.episode_rewards and lengths == dev.episode_lengths[0].tolist()
    many = _trainer(rule, env, cfg, 2)
    with pytest.raises(RuntimeError, match="num_runs == 1"):
        many.select_action(0)
    with pytest.raises(RuntimeError, match="num_runs == 1"):
        many.update(0, 0, -1.0, 1, False, 0)
