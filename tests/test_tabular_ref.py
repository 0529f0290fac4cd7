"""The rules of FrozenLake-v1 (4x4) and CliffWalking-v0 that include/gymrl.h states, pinned in closed form on the test
reference (tests/tabular_ref.py) that the kernels are compared with bit for bit.  No GPU."""
import numpy as np

import tabular_ref as ref
from test_rng_distributions import assert_chi2

# successor of every state under LEFT, DOWN, RIGHT, UP on SFFF / FHFH / FFFH / HFFG, written out by hand
FROZEN_SUCCESSORS = (
    (0, 4, 1, 0), (0, 5, 2, 1), (1, 6, 3, 2), (2, 7, 3, 3),
    (4, 8, 5, 0), (4, 9, 6, 1), (5, 10, 7, 2), (6, 11, 7, 3),
    (8, 12, 9, 4), (8, 13, 10, 5), (9, 14, 11, 6), (10, 15, 11, 7),
    (12, 12, 13, 8), (12, 13, 14, 9), (13, 14, 15, 10), (14, 15, 15, 11),
)


def test_frozenlake_every_successor_and_the_flags():
    env = ref.FrozenLake(is_slippery=False)
    assert [c for row in env.MAP for c in row].index("S") == env.start == 0
    assert {i for i, c in enumerate("".join(env.MAP)) if c == "H"} == set(env.holes) == {5, 7, 11, 12}
    assert "".join(env.MAP).index("G") == env.goal == 15
    for s in range(16):
        for d in range(4):
            nxt, reward, terminated, truncated = env.step(s, d, 0, 0)
            assert nxt == FROZEN_SUCCESSORS[s][d], (s, d)
            assert reward == (1.0 if nxt == 15 else 0.0)
            assert terminated == (nxt in (5, 7, 11, 12, 15)) and not truncated


def test_frozenlake_border_clipping():
    env = ref.FrozenLake(is_slippery=False)
    for s in (0, 4, 8, 12):
        assert env.step(s, 0, 0, 0)[0] == s              # LEFT on the left edge
    for s in (3, 7, 11, 15):
        assert env.step(s, 2, 0, 0)[0] == s              # RIGHT on the right edge
    for s in (0, 1, 2, 3):
        assert env.step(s, 3, 0, 0)[0] == s              # UP on the top edge
    for s in (12, 13, 14, 15):
        assert env.step(s, 1, 0, 0)[0] == s              # DOWN on the bottom edge


def test_frozenlake_slip_directions():
    env = ref.FrozenLake(is_slippery=True)
    for a in range(4):
        assert [env.direction(a, c) for c in range(3)] == [(a - 1) % 4, a, (a + 1) % 4]
    # from 9 (row 2, col 1) under DOWN: LEFT -> 8, DOWN -> 13, RIGHT -> 10
    assert [env.step(9, 1, c, 0)[0] for c in range(3)] == [8, 13, 10]
    # the non-slippery env ignores the slip choice
    assert [ref.FrozenLake(is_slippery=False).step(9, 1, c, 0)[0] for c in range(3)] == [13, 13, 13]


def test_frozenlake_shaped_reward_precedence():
    env = ref.FrozenLake(shaped=True)
    assert env.train_reward(4, 5, 0.0) == -10.0          # a hole
    assert env.train_reward(14, 15, 1.0) == 100.0        # the goal
    assert env.train_reward(0, 0, 0.0) == -5.0           # stayed in place
    assert env.train_reward(0, 1, 0.0) == -1.0           # any other move
    # precedence: a hole or the goal wins over "stayed" (neither can be stayed in, but the order is the reference's)
    assert env.train_reward(5, 5, 0.0) == -10.0 and env.train_reward(15, 15, 1.0) == 100.0
    plain = ref.FrozenLake(shaped=False)
    assert plain.train_reward(14, 15, 1.0) == 1.0 and plain.train_reward(0, 0, 0.0) == 0.0


def test_frozenlake_truncates_at_its_own_hundredth_step():
    env = ref.FrozenLake(is_slippery=False)
    assert env.step(0, 0, 0, 98) == (0, 0.0, False, False)
    assert env.step(0, 0, 0, 99) == (0, 0.0, False, True)
    assert env.step(14, 2, 0, 99) == (15, 1.0, True, True)                   # both flags on the 100th step
    # a run whose step budget is larger than the env's limit still ends its episodes at 100: greedy LEFT on a zero table
    cfg = dict(seed=1, max_episodes=2, max_steps=150, lr=0.1, gamma=0.9, epsilon_start=0.0, epsilon_end=0.0, epsilon_decay=1.0)
    out = ref.train_run(env, cfg, 0)
    assert out["lengths"] == [100, 100] and out["k"] == 200 and not out["never_done"]


def test_cliffwalking_rules():
    env = ref.CliffWalking()
    assert env.step(36, 1) == (36, -100.0, False, False)                     # RIGHT from the start: the cliff, back to 36
    for col in range(1, 11):
        assert env.step(24 + col, 2) == (36, -100.0, False, False)           # DOWN onto every cliff cell
    assert env.step(35, 2) == (47, -1.0, True, False)                        # the goal terminates, at the ordinary -1
    assert env.step(46 - 12, 1) == (35, -1.0, False, False)
    assert env.step(36, 0) == (24, -1.0, False, False)
    # border clipping
    assert env.step(0, 0)[0] == 0 and env.step(0, 3)[0] == 0 and env.step(11, 1)[0] == 11 and env.step(11, 0)[0] == 11
    assert env.step(36, 3)[0] == 36 and env.step(36, 2)[0] == 36 and env.step(24, 3)[0] == 24
    # no time limit of its own
    assert env.step(0, 0, 0, 10 ** 6)[3] is False
    # every non-cliff move is one cell
    for s in range(48):
        for a, (dr, dc) in enumerate(((-1, 0), (0, 1), (1, 0), (0, -1))):
            row, col = divmod(s, 12)
            r2, c2 = min(max(row + dr, 0), 3), min(max(col + dc, 0), 11)
            want = 36 if (r2 == 3 and 1 <= c2 <= 10) else r2 * 12 + c2
            assert env.step(s, a)[0] == want, (s, a)


def test_draw_laws():
    """The slip choice over 30 000 draws: three equally likely values; the exploring action and u alongside it."""
    n = 30000
    draws = [ref.step_draw(42, 3, k) for k in range(1, n + 1)]
    slip = np.bincount([d[2] for d in draws], minlength=3)
    assert slip.sum() == n and len(slip) == 3
    assert_chi2(slip, np.full(3, n / 3), "slip choice")
    act = np.bincount([d[1] for d in draws], minlength=4)
    assert len(act) == 4
    assert_chi2(act, np.full(4, n / 4), "exploring action")
    u = np.array([d[0] for d in draws])
    assert u.min() >= 0.0 and u.max() < 1.0
    assert_chi2(np.bincount((u * 10).astype(int), minlength=10), np.full(10, n / 10), "u deciles")
    # streams differ, and the layout is the documented one
    assert ref.step_draw(42, 3, 1) != ref.step_draw(42, 4, 1) != ref.step_draw(42, 3, 2)
    from oracle import oracle as orc
    x, y, z, w = orc.philox(42, 5, 1, 7, ref.RNG_TABULAR)
    assert ref.step_draw(42, (1 << 32) + 5, 7) == (((x >> 5) * 67108864.0 + (y >> 6)) * 2.0 ** -53, (z * 4) >> 32, (w * 3) >> 32)


def test_first_update_and_never_done_in_closed_form():
    """CliffWalking, epsilon 0, zero table: the first maximum of a zero row is UP, so the run climbs 36 -> 24 -> 12 -> 0; each
    visited entry drops to lr * (-1) and the tie-break moves on (the walk is not UP for ever: with 200 steps it reaches the
    goal).  Within 2 episodes of 50 steps it never does: every episode runs out of steps, every target is non-terminal."""
    cfg = dict(seed=42, max_episodes=2, max_steps=50, lr=0.1, gamma=0.9, epsilon_start=0.0, epsilon_end=0.0, epsilon_decay=300.0)
    out = ref.train_run(ref.CliffWalking(), cfg, 0)
    assert out["never_done"] and out["lengths"] == [50, 50] and out["k"] == 100
    one = ref.train_run(ref.CliffWalking(), dict(cfg, max_episodes=1, max_steps=1), 0)
    assert one["Q"][36][0] == 0.0 + 0.1 * ((-1.0 + 0.9 * 0.0) - 0.0)
    three = ref.train_run(ref.CliffWalking(), dict(cfg, max_episodes=1, max_steps=3), 0)
    assert [three["Q"][s][0] for s in (36, 24, 12)] == [-0.1, -0.1, -0.1]


def test_trainer_host_draw_is_the_reference_draw():
    """select_action's host-side draw (gymrl_amd/tabular.py: Philox on Python integers) against this file's reference through
    oracle.philox: 64-bit streams and seeds, evaluation-range streams, k up to the default run's last action."""
    from gymrl_amd import tabular
    assert tabular.RNG_TABULAR == ref.RNG_TABULAR and tabular.EVAL_STREAM0 == ref.EVAL_STREAM0
    for seed in (0, 42, (0x299F31D0 << 32) | 0xA4093822, (1 << 64) - 1):
        for stream in (0, 1, 64, (5 << 32) + 3, (1 << 40) + 7, (1 << 40) + (1 << 39) + 2, (1 << 63) + 11):
            for k in (1, 2, 255, 4097, 99999, 100000, (1 << 31) - 1):
                assert tabular.step_draw(seed, stream, k, 4) == ref.step_draw(seed, stream, k), (seed, stream, k)
