"""The plain-Python restatement of SARSA, Expected SARSA and Double Q-learning (tests/tabular_td_ref.py) tied to the Q-learning
reference it is built on and to the three loops of include/gymrl.h in closed form.  No GPU."""
import numpy as np

import tabular_ref as ref
import tabular_td_ref as td

FROZEN_CFG = dict(seed=42, max_episodes=8, max_steps=30, lr=0.1, gamma=0.9, epsilon_start=0.95, epsilon_end=0.01, epsilon_decay=200)
CLIFF_CFG = dict(seed=42, max_episodes=6, max_steps=25, lr=0.1, gamma=0.9, epsilon_start=0.95, epsilon_end=0.01, epsilon_decay=300)


def test_rule_0_is_tabular_refs_qlearning():
    for env, cfg in ((ref.FrozenLake(True, True), FROZEN_CFG), (ref.FrozenLake(False, False), FROZEN_CFG), (ref.CliffWalking(), CLIFF_CFG)):
        for stream in (0, 7):
            got, want = td.train_run(td.QLEARNING, env, cfg, stream), ref.train_run(env, cfg, stream)
            for key in ("Q", "rewards", "lengths", "k", "episodes"):
                assert got[key] == want[key], key
            assert got["draws"] == want["lengths"] and got["Q2"] is None


def test_sarsa_without_exploration_is_qlearnings_first_episode():
    """eps = 0 on deterministic CliffWalking: every target bootstraps from the greedy entry of the next row, which is that row's
    maximum, so as long as no step returns to a state already written SARSA's first episode writes Q-learning's values."""
    env = ref.CliffWalking()
    path = [[0.0] * 4 for _ in range(48)]                    # UP, eleven RIGHT, DOWN into the goal: 13 steps, no state twice
    path[36][0] = 1.0
    for s in range(24, 35):
        path[s][1] = 1.0
    path[35][2] = 1.0
    cfg = dict(CLIFF_CFG, max_episodes=1, max_steps=40, epsilon_start=0.0, epsilon_end=0.0)
    got, want = td.train_run(td.SARSA, env, cfg, 3, Q=path), ref.train_run(env, cfg, 3, Q=path)
    assert got["Q"] == want["Q"] and got["rewards"] == want["rewards"] == [-13.0] and got["lengths"] == want["lengths"] == [13]
    assert got["Q"] != path and got["k"] == want["k"] == 13                     # terminated: no extra draw
    # from a zero table the greedy walk is 36 -> 24 -> 12 -> 0: the same for three steps (SARSA has drawn a fourth action) ...
    cfg = dict(cfg, max_steps=3)
    got, want = td.train_run(td.SARSA, env, cfg, 3), ref.train_run(env, cfg, 3)
    assert got["Q"] == want["Q"] and np.count_nonzero(np.array(got["Q"])) == 3 and (got["k"], want["k"]) == (4, 3)
    # ... and on the fifth the rules part: UP at 0 stays on 0, SARSA is committed to the UP it chose before Q[0, UP] moved,
    # Q-learning looks again and goes RIGHT
    cfg = dict(cfg, max_steps=5)
    got, want = td.train_run(td.SARSA, env, cfg, 3), ref.train_run(env, cfg, 3)
    assert got["Q"][0][:2] == [-0.1 + 0.1 * ((-1.0 + 0.9 * 0.0) - -0.1), 0.0] and want["Q"][0][:2] == [-0.1, -0.1]


def test_sarsa_draw_count_per_episode():
    """A terminated episode takes one draw per step; one that runs out at max_steps has drawn the action of a step it never takes."""
    cfg = dict(FROZEN_CFG, max_episodes=40, max_steps=12)
    out = td.train_run(td.SARSA, ref.FrozenLake(True, True), cfg, 0)
    ran_out = [n for n, d in zip(out["lengths"], out["draws"]) if d == n + 1]
    ended = [n for n, d in zip(out["lengths"], out["draws"]) if d == n]
    assert len(ran_out) + len(ended) == 40 and ran_out and ended
    assert all(n == 12 for n in ran_out) and out["k"] == sum(out["draws"]) == sum(out["lengths"]) + len(ran_out)
    assert out["k"] <= td.draws_needed(td.SARSA, cfg) == 40 * 13
    # CliffWalking never terminates inside 25 steps of a fresh table: every episode takes max_steps + 1 draws
    out = td.train_run(td.SARSA, ref.CliffWalking(), CLIFF_CFG, 0)
    assert out["lengths"] == [25] * 6 and out["draws"] == [26] * 6 and out["k"] == td.draws_needed(td.SARSA, CLIFF_CFG)


def test_sarsa_picks_the_next_action_before_the_write():
    """s2 == s (a step into the wall): a2 is the first maximum of the row BEFORE Q[s, a] moves."""
    cfg = dict(CLIFF_CFG, max_episodes=1, max_steps=1, epsilon_start=0.0, epsilon_end=0.0, lr=0.5, gamma=1.0)
    Q = [[0.0] * 4 for _ in range(48)]
    Q[36] = [-5.0, -5.0, -5.0, 1.0]                          # LEFT at the start state: stays on 36
    out = td.train_run(td.SARSA, ref.CliffWalking(), cfg, 0, Q=Q)
    assert out["Q"][36][3] == 1.0 + 0.5 * ((-1.0 + 1.0 * 1.0) - 1.0) and out["k"] == 2


def test_double_q_coin_and_exploring_action_bits():
    cfg = dict(FROZEN_CFG, max_episodes=1, max_steps=1)
    env = ref.FrozenLake(False, False)
    coins = []
    for stream in range(64):
        word = td.action_word(42, stream, 1)
        u, explore, slip = ref.step_draw(42, stream, 1)
        assert explore == (word * 4) >> 32 == word >> 30
        coin = word & 1
        coins.append(coin)
        # one exploring step from planted tables: exactly one entry of exactly the coin's table moves
        QA = [[1.0] * 4 for _ in range(16)]
        QB = [[2.0] * 4 for _ in range(16)]
        out = td.train_run(td.DOUBLE_Q, env, cfg, stream, Q=QA, Q2=QB, eps=lambda k: 1.0)
        nxt, r, terminated, _ = env.step(0, explore, slip, 0)
        assert not terminated
        moved, kept = (out["Q2"], out["Q"]) if coin else (out["Q"], out["Q2"])
        own, other = (2.0, 1.0) if coin else (1.0, 2.0)
        assert moved[0][explore] == own + 0.1 * ((r + 0.9 * other) - own)
        assert sum(v != own for row in moved for v in row) == 1 and all(v == other for row in kept for v in row)
    assert 16 <= sum(coins) <= 48                            # a fair bit over 64 streams (6 sigma would be 8..56)


def test_double_q_acts_on_the_sum():
    cfg = dict(FROZEN_CFG, max_episodes=1, max_steps=1, epsilon_start=0.0, epsilon_end=0.0)
    QA = [[0.0] * 4 for _ in range(16)]
    QB = [[0.0] * 4 for _ in range(16)]
    QA[0], QB[0] = [3.0, 0.0, 1.0, 0.0], [0.0, 0.0, 2.5, 0.0]      # QA alone says LEFT, the sum says RIGHT
    out = td.train_run(td.DOUBLE_Q, ref.FrozenLake(False, False), cfg, 0, Q=QA, Q2=QB)
    changed = [(t, a) for t, (new, old) in enumerate(((out["Q"], QA), (out["Q2"], QB))) for a in range(4) if new[0][a] != old[0][a]]
    assert len(changed) == 1 and changed[0][1] == 2


def test_expected_sarsa_limits():
    """eps = 0: 0 * 0.25 * sum + 1 * max is the maximum itself, Q-learning bit for bit.  eps = 1: r + gamma * 0.25 * sum."""
    for env, cfg in ((ref.FrozenLake(True, True), FROZEN_CFG), (ref.CliffWalking(), CLIFF_CFG)):
        greedy = dict(cfg, epsilon_start=0.0, epsilon_end=0.0)
        got, want = td.train_run(td.EXPECTED_SARSA, env, greedy, 1), ref.train_run(env, greedy, 1)
        assert got["Q"] == want["Q"] and got["rewards"] == want["rewards"] and got["k"] == want["k"]
    cfg = dict(CLIFF_CFG, max_episodes=1, max_steps=1)
    Q = [[0.0] * 4 for _ in range(48)]
    Q[24], Q[36] = [1.0, 2.0, 4.0, 8.5], [0.5, 0.25, 0.125, 4.0]
    _, explore, _ = ref.step_draw(42, 0, 1)
    nxt, r, _, _ = ref.CliffWalking().step(36, explore)
    out = td.train_run(td.EXPECTED_SARSA, ref.CliffWalking(), cfg, 0, Q=Q, eps=[1.0])
    q = Q[nxt]
    target = r + 0.9 * (0.25 * (((q[0] + q[1]) + q[2]) + q[3]))
    assert out["Q"][36][explore] == Q[36][explore] + 0.1 * (target - Q[36][explore])
    # in between, the two parts are rounded separately and then added
    out = td.train_run(td.EXPECTED_SARSA, ref.CliffWalking(), cfg, 0, Q=Q, eps=[0.3])
    u = ref.step_draw(42, 0, 1)[0]
    a = explore if u < 0.3 else 3
    nxt, r, _, _ = ref.CliffWalking().step(36, a)
    q = Q[nxt]
    target = r + 0.9 * (0.3 * 0.25 * (((q[0] + q[1]) + q[2]) + q[3]) + (1.0 - 0.3) * max(q))
    assert out["Q"][36][a] == Q[36][a] + 0.1 * (target - Q[36][a])


def test_population_stacks_runs():
    out = td.train_population(td.DOUBLE_Q, ref.FrozenLake(True, False), FROZEN_CFG, 3, run_id0=5)
    one = td.train_run(td.DOUBLE_Q, ref.FrozenLake(True, False), FROZEN_CFG, 6)
    assert out["Q"].shape == out["Q2"].shape == (3, 16, 4) and out["Q"][1].tolist() == one["Q"] and out["Q2"][1].tolist() == one["Q2"]
    assert out["k"][1] == one["k"] and out["lengths"][1].tolist() == one["lengths"]
