"""Plain-Python float64 restatement of SARSA, Expected SARSA and Double Q-learning for one run, written from the three loops in
include/gymrl.h on the env steps and the draw of tests/tabular_ref.py.  Test infrastructure: no GPU, no gymrl_amd import.

Python floats are IEEE float64 and every expression keeps the header's operation order, so the kernel's tables are compared
with array_equal.  `eps` is a callable k -> eps_k, or a sequence with eps_k at index k - 1 (the table the kernel is handed).
"""
import numpy as np

import tabular_ref as ref
from oracle import oracle as orc

QLEARNING, SARSA, EXPECTED_SARSA, DOUBLE_Q = 0, 1, 2, 3
RULES = {"qlearning": QLEARNING, "sarsa": SARSA, "expected_sarsa": EXPECTED_SARSA, "double_q": DOUBLE_Q}


def action_word(seed, stream, k):
    """Word 2 of the draw of (stream, k): its top bits are the exploring action, its low bit Double Q-learning's coin."""
    return orc.philox(seed, stream & 0xFFFFFFFF, stream >> 32, k, ref.RNG_TABULAR)[2]


def draws_needed(rule, cfg):
    return cfg["max_episodes"] * (cfg["max_steps"] + (1 if rule == SARSA else 0))


def _eps_fn(cfg, eps):
    if eps is None:
        return lambda k: ref.epsilon(cfg, k)
    return eps if callable(eps) else (lambda k: eps[k - 1])


def _table(env, Q):
    return [[0.0] * ref.N_ACTIONS for _ in range(env.n_states)] if Q is None else [list(map(float, r)) for r in Q]


class _Run:
    """k and select(row) of one run: the behaviour policy all rules share."""

    def __init__(self, cfg, stream, eps):
        self.seed, self.stream, self.eps_of, self.k = cfg["seed"], stream, _eps_fn(cfg, eps), 0
        self.draw_log = []                                   # (k, u, explored) of every select

    def select(self, row):
        self.k += 1
        self.eps = self.eps_of(self.k)
        u, explore, self.slip = ref.step_draw(self.seed, self.stream, self.k)
        self.draw_log.append((self.k, u, u < self.eps))
        return explore if u < self.eps else ref.greedy(row)


def train_run(rule, env, cfg, stream, Q=None, Q2=None, eps=None):
    """One run -> dict(Q, Q2 (None unless DOUBLE_Q), rewards, lengths, k, episodes, draws: k spent per episode)."""
    Q = _table(env, Q)
    Q2 = _table(env, Q2) if rule == DOUBLE_Q else None
    run = _Run(cfg, stream, eps)
    lr, gamma = cfg["lr"], cfg["gamma"]
    rewards, lengths, draws = [], [], []
    for _ in range(cfg["max_episodes"]):
        s, ret, steps, k0 = env.start, 0.0, 0, run.k
        if rule == SARSA:
            a = run.select(Q[s])
            slip = run.slip
        for _ in range(cfg["max_steps"]):
            if rule == DOUBLE_Q:
                a = run.select([Q[s][j] + Q2[s][j] for j in range(ref.N_ACTIONS)])
                slip = run.slip
            elif rule != SARSA:
                a = run.select(Q[s])
                slip = run.slip
            s2, r, terminated, truncated = env.step(s, a, slip, steps)
            done = terminated or truncated
            r = env.train_reward(s, s2, r)
            T = Q                                             # the table that is written
            if rule == SARSA:
                if done:
                    target = r
                else:
                    a2 = run.select(Q[s2])                    # before this step's write
                    slip = run.slip
                    target = r + gamma * Q[s2][a2]
            elif rule == EXPECTED_SARSA:
                q0, q1, q2, q3 = Q[s2]
                e = run.eps
                target = r if done else r + gamma * (e * 0.25 * (((q0 + q1) + q2) + q3) + (1.0 - e) * max(q0, q1, q2, q3))
            elif rule == DOUBLE_Q:
                coin = action_word(cfg["seed"], stream, run.k) & 1
                T, other = (Q2, Q) if coin else (Q, Q2)
                target = r if done else r + gamma * other[s2][ref.greedy(T[s2])]
            else:
                target = r if done else r + gamma * max(Q[s2])
            T[s][a] = T[s][a] + lr * (target - T[s][a])
            ret, steps = ret + r, steps + 1
            if done:
                break
            s = s2
            if rule == SARSA:
                a = a2
        rewards.append(ret)
        lengths.append(steps)
        draws.append(run.k - k0)
    return dict(Q=Q, Q2=Q2, rewards=rewards, lengths=lengths, k=run.k, episodes=len(rewards), draws=draws, draw_log=run.draw_log)


def train_population(rule, env, cfg, num_runs, run_id0=0, Q=None, Q2=None, eps=None):
    """Q / Q2: None (zero tables) or [R][S][4] starting tables."""
    runs = [train_run(rule, env, cfg, run_id0 + r, None if Q is None else Q[r], None if Q2 is None else Q2[r], eps) for r in range(num_runs)]
    out = dict(Q=np.array([r["Q"] for r in runs], np.float64), rewards=np.array([r["rewards"] for r in runs], np.float64),
               lengths=np.array([r["lengths"] for r in runs], np.int32), k=np.array([r["k"] for r in runs], np.int32),
               episodes=np.array([r["episodes"] for r in runs], np.int32), draws=np.array([r["draws"] for r in runs], np.int32))
    out["Q2"] = np.array([r["Q2"] for r in runs], np.float64) if rule == DOUBLE_Q else None
    return out
