"""Plain-Python float64 restatement of FrozenLake-v1 (4x4), CliffWalking-v0 and one tabular Q-learning run, written from
the rules in include/gymrl.h; the draws go through oracle.philox.  Test infrastructure: no GPU, no gymrl_amd import.

A run is train() of qlearning_frozenlake.py / qlearning_cliffwalking.py with np.random replaced by the counter-keyed draw
of (stream, k): python floats are IEEE float64 and every expression below keeps the reference's operation order, so the
kernel's tables are compared with array_equal.
"""
import math

import numpy as np

from oracle import oracle as orc

RNG_TABULAR = 0x70000000
EVAL_STREAM0 = 1 << 40
N_ACTIONS = 4


def step_draw(seed, stream, k):
    """ONE Philox call per (stream, k): words 0, 1 -> u in [0, 1), word 2 -> exploring action, word 3 -> slip choice."""
    x, y, z, w = orc.philox(seed, stream & 0xFFFFFFFF, stream >> 32, k, RNG_TABULAR)
    u = (float(x >> 5) * 67108864.0 + float(y >> 6)) * 2.0 ** -53
    return u, (z * N_ACTIONS) >> 32, (w * 3) >> 32


class FrozenLake:
    """SFFF / FHFH / FFFH / HFFG.  0 LEFT, 1 DOWN, 2 RIGHT, 3 UP."""
    n_states, start, goal, holes, limit = 16, 0, 15, frozenset((5, 7, 11, 12)), 100
    MAP = ("SFFF", "FHFH", "FFFH", "HFFG")

    def __init__(self, is_slippery=True, shaped=False):
        self.is_slippery, self.shaped = is_slippery, shaped

    @staticmethod
    def move(state, direction):
        row, col = divmod(state, 4)
        if direction == 0:
            col = max(col - 1, 0)
        elif direction == 1:
            row = min(row + 1, 3)
        elif direction == 2:
            col = min(col + 1, 3)
        else:
            row = max(row - 1, 0)
        return row * 4 + col

    @staticmethod
    def direction(action, slip_choice):
        return ((action - 1) % 4, action, (action + 1) % 4)[slip_choice]

    def step(self, state, action, slip_choice, steps_before):
        """-> (next_state, reward, terminated, truncated); steps_before: steps already taken in this episode."""
        nxt = self.move(state, self.direction(action, slip_choice) if self.is_slippery else action)
        terminated = nxt in self.holes or nxt == self.goal
        return nxt, 1.0 if nxt == self.goal else 0.0, terminated, steps_before + 1 >= self.limit

    def train_reward(self, state, nxt, reward):
        if not self.shaped:
            return reward
        if nxt in self.holes:
            return -10.0
        if nxt == self.goal:
            return 100.0
        if nxt == state:
            return -5.0
        return -1.0


class CliffWalking:
    """4 x 12.  0 UP, 1 RIGHT, 2 DOWN, 3 LEFT."""
    n_states, start, goal, is_slippery = 48, 36, 47, False

    def step(self, state, action, slip_choice=0, steps_before=0):
        row, col = divmod(state, 12)
        if action == 0:
            row = max(row - 1, 0)
        elif action == 1:
            col = min(col + 1, 11)
        elif action == 2:
            row = min(row + 1, 3)
        else:
            col = max(col - 1, 0)
        if row == 3 and 1 <= col <= 10:
            return self.start, -100.0, False, False
        nxt = row * 12 + col
        return nxt, -1.0, nxt == self.goal, False

    def train_reward(self, state, nxt, reward):
        return reward


def epsilon(cfg, k):
    return cfg["epsilon_end"] + (cfg["epsilon_start"] - cfg["epsilon_end"]) * math.exp(-1.0 * k / cfg["epsilon_decay"])


def greedy(row):
    best = 0
    for a in range(1, N_ACTIONS):
        if row[a] > row[best]:
            best = a
    return best


def train_run(env, cfg, stream, Q=None):
    """One run -> dict(Q [S][4], rewards, lengths, k, episodes, never_done: no update ever used the terminal target)."""
    Q = [[0.0] * N_ACTIONS for _ in range(env.n_states)] if Q is None else [list(map(float, r)) for r in Q]
    rewards, lengths, k, never_done = [], [], 0, True
    for _ in range(cfg["max_episodes"]):
        state, ret, steps = env.start, 0.0, 0
        for _ in range(cfg["max_steps"]):
            k += 1
            u, explore, slip = step_draw(cfg["seed"], stream, k)
            action = explore if u < epsilon(cfg, k) else greedy(Q[state])
            nxt, reward, terminated, truncated = env.step(state, action, slip, steps)
            done = terminated or truncated
            reward = env.train_reward(state, nxt, reward)
            predict = Q[state][action]
            target = reward if done else reward + cfg["gamma"] * max(Q[nxt])
            Q[state][action] = predict + cfg["lr"] * (target - predict)
            never_done = never_done and not done
            state, ret, steps = nxt, ret + reward, steps + 1
            if done:
                break
        rewards.append(ret)
        lengths.append(steps)
    return dict(Q=Q, rewards=rewards, lengths=lengths, k=k, episodes=len(rewards), never_done=never_done)


def train_population(env, cfg, num_runs, run_id0=0):
    runs = [train_run(env, cfg, run_id0 + r) for r in range(num_runs)]
    return dict(Q=np.array([r["Q"] for r in runs], np.float64), rewards=np.array([r["rewards"] for r in runs], np.float64),
                lengths=np.array([r["lengths"] for r in runs], np.int32), k=np.array([r["k"] for r in runs], np.int32),
                episodes=np.array([r["episodes"] for r in runs], np.int32), never_done=all(r["never_done"] for r in runs))


def eval_episode(env, Q, seed, stream, cap):
    """One greedy episode -> (return of the env's own reward, steps, reached the goal)."""
    state, ret, steps = env.start, 0.0, 0
    while steps < cap:
        slip = step_draw(seed, stream, steps + 1)[2] if env.is_slippery else 0
        state, reward, terminated, truncated = env.step(state, greedy(Q[state]), slip, steps)
        ret, steps = ret + reward, steps + 1
        if terminated or truncated:
            return ret, steps, bool(terminated and state == env.goal)
    return ret, steps, False


def eval_population(env, Q, seed, num_episodes, cap, run_id0=0):
    """[R, E] returns, lengths, flags with the trainers' stream numbering."""
    Q = np.asarray(Q, np.float64)
    Q = Q[None] if Q.ndim == 2 else Q
    out = [[eval_episode(env, Q[r].tolist(), seed, EVAL_STREAM0 + run_id0 * num_episodes + r * num_episodes + e, cap)
            for e in range(num_episodes)] for r in range(len(Q))]
    return (np.array([[o[0] for o in row] for row in out], np.float64), np.array([[o[1] for o in row] for row in out], np.int32),
            np.array([[o[2] for o in row] for row in out], np.uint8))
