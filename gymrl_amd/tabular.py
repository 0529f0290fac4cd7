"""What qlearning_frozenlake.py and qlearning_cliffwalking.py share: a population of `num_runs` independent tabular Q-learning
runs behind the reference's QLearningTrainer surface (qlearning_frozenlake.py:36-177 / qlearning_cliffwalking.py:34-144).

train() is csrc/tabular.hip's gymrl_qlearn_train: one lane per run, every run's table in LDS, `steps_per_launch` steps of
every run per launch and nothing but the launches in between.  eval() / test() are gymrl_qlearn_eval.  select_action() and
update() are the reference's two methods restated on the host in float64 for one run; they are not on the hot path.
TabularTD (below) is the same population under SARSA, Expected SARSA or Double Q-learning: sarsa_frozenlake.py /
sarsa_cliffwalking.py.
"""
import math

import numpy as np
import torch

from . import ops

EVAL_STREAM0 = 1 << 40          # evaluation draws: a stream range no training run reaches (the trainers' env_id0 habit)
VISUAL_STREAM_OFFSET = 1 << 39  # test()'s extra greedy episode: streams eval() never draws from
RNG_TABULAR = 0x70000000        # csrc/tabular_device.hpp


def philox4x32(key, c0, c1, c2, c3):
    """Philox4x32-10 (csrc/gymrl_device.hpp) on Python integers: the host side of select_action's draw."""
    k0, k1, m = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF, 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & m, (p0 >> 32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return c0, c1, c2, c3


def step_draw(seed, stream, k, n_actions):
    """(u, exploring action, slip choice) of (stream, k): csrc/tabular_device.hpp's word layout."""
    x, y, z, w = philox4x32(seed, stream & 0xFFFFFFFF, stream >> 32, k, RNG_TABULAR)
    return (float(x >> 5) * 67108864.0 + float(y >> 6)) * 2.0 ** -53, (z * n_actions) >> 32, (w * 3) >> 32


class TabularQLearning:
    """Subclasses set: kind (ops.FROZENLAKE / ops.CLIFFWALKING), report_every, and print their own evaluation lines."""
    kind = None
    report_every = 50

    def __init__(self, config):
        self.cfg = config
        cfg = config
        self.device = torch.device(cfg.device)
        self.num_runs = int(cfg.num_runs)
        if self.num_runs < 1:
            raise ValueError("num_runs must be at least 1")
        self.n_states, self.n_actions = ops.TABULAR_STATES[self.kind], ops.TABULAR_ACTIONS
        shape = (self.n_states, self.n_actions)
        self.Q = np.zeros(shape if self.num_runs == 1 else (self.num_runs,) + shape)
        self.epsilon = cfg.epsilon_start
        self.sample_count = 0
        self.episode_rewards = [] if self.num_runs == 1 else np.zeros((self.num_runs, 0))
        self.episode_lengths = np.zeros((self.num_runs, 0), np.int32)
        print(f"Environment: {cfg.env_name}")
        print(f"States: {self.n_states}, Actions: {self.n_actions}")

    # ---- the reference's per-step methods, host float64, one run ----
    def _one_run(self, what):
        if self.num_runs != 1:
            raise RuntimeError(f"{what} restates one run's step on the host: it needs num_runs == 1 (got {self.num_runs}); "
                               "train() steps a population on the device")

    def _epsilon_at(self, k):
        cfg = self.cfg
        return cfg.epsilon_end + (cfg.epsilon_start - cfg.epsilon_end) * math.exp(-1.0 * k / cfg.epsilon_decay)

    def _get_epsilon(self):
        self.sample_count += 1
        self.epsilon = self._epsilon_at(self.sample_count)
        return self.epsilon

    def select_action(self, state, deterministic=False):
        self._one_run("select_action")
        if not deterministic:
            eps = self._get_epsilon()
            u, explore, _ = step_draw(self.cfg.seed, self.cfg.run_id0, self.sample_count, self.n_actions)
            if u < eps:
                return int(explore)
        return int(np.argmax(self.Q[state, :]))

    def update(self, state, action, reward, next_state, done):
        self._one_run("update")
        predict = self.Q[state, action]
        if done:
            target = reward
        else:
            target = reward + self.cfg.gamma * np.max(self.Q[next_state, :])
        self.Q[state, action] += self.cfg.lr * (target - predict)

    # ---- the population on the device ----
    def _flags(self):
        return dict(is_slippery=bool(getattr(self.cfg, "is_slippery", False)), shaped=bool(getattr(self.cfg, "use_reward_shaping", False)))

    def _tables(self, Q):
        return torch.from_numpy(np.ascontiguousarray(Q, np.float64).reshape(self.num_runs, self.n_states, self.n_actions)).to(self.device)

    # what a rule other than Q-learning changes about train() and _evaluate() (TabularTD below)
    def _draw_budget(self):
        return self.cfg.max_episodes * self.cfg.max_steps

    def _state_bytes(self):
        return ops.qlearn_state_bytes(self.num_runs)

    def _launch(self, Q, state, eps, chunk, rew, length, k_dev, done_dev, restart):
        cfg = self.cfg
        ops.qlearn_train(self.kind, Q, state, eps, cfg.seed, cfg.run_id0, cfg.max_episodes, cfg.max_steps, chunk, cfg.lr, cfg.gamma,
                         rew, length, k_dev, done_dev, restart=restart, **self._flags())

    def _greedy_table(self):
        return self.Q

    def train(self):
        print("Starting training...")
        cfg, R, dev = self.cfg, self.num_runs, self.device
        total = self._draw_budget()
        chunk = int(cfg.steps_per_launch) if cfg.steps_per_launch else total
        eps = torch.tensor([self._epsilon_at(k) for k in range(1, total + 1)], dtype=torch.float64).to(dev)
        Q = self._tables(self.Q)
        state = torch.zeros(self._state_bytes(), dtype=torch.uint8, device=dev)
        rew = torch.zeros(R, cfg.max_episodes, dtype=torch.float64, device=dev)
        length = torch.zeros(R, cfg.max_episodes, dtype=torch.int32, device=dev)
        k_dev = torch.zeros(R, dtype=torch.int32, device=dev)
        done_dev = torch.zeros(R, dtype=torch.int32, device=dev)
        reported, launched = 0, 0
        while True:
            self._launch(Q, state, eps, chunk, rew, length, k_dev, done_dev, restart=launched == 0)
            launched += chunk
            finished = int(done_dev.min().item())              # episodes every run has behind it
            if finished // self.report_every > reported // self.report_every:
                self._report(rew[:, :finished].cpu().numpy(), length[:, :finished].cpu().numpy(), reported, finished)
            reported = finished
            if finished >= cfg.max_episodes or launched >= total:
                break
        self.Q = Q.cpu().numpy().reshape(self.Q.shape)
        rewards, self.episode_lengths = rew.cpu().numpy(), length.cpu().numpy()
        self.episode_rewards = rewards[0].tolist() if R == 1 else rewards
        self.sample_count = int(k_dev[0].item())
        self.run_sample_counts, self.run_episodes = k_dev.cpu().numpy(), done_dev.cpu().numpy()
        if self.sample_count:
            self.epsilon = self._epsilon_at(self.sample_count)
        print("Training completed!")

    def _report(self, rew, length, since, upto):
        """The reference's progress line for every report_every-th episode in (since, upto]: rank-0 style, the mean over the
        runs where there are several.  Epsilon is the one after the episode's last action (run 0's, the runs' mean count)."""
        n = self.report_every
        k_after = np.cumsum(length, axis=1)
        for e in range((since // n + 1) * n, upto + 1, n):
            k = int(round(float(k_after[:, e - 1].mean())))
            print(f"Episode {e}/{self.cfg.max_episodes} | Reward: {rew[:, e - 1].mean():.1f} | "
                  f"Avg({n}): {rew[:, e - n:e].mean():.1f} | Epsilon: {self._epsilon_at(k):.3f}")

    def _evaluate(self, num_episodes, cap, stream_offset=0):
        """(returns, lengths, reached) of num_episodes greedy episodes per run, numpy [R, num_episodes].  stream_offset moves the
        env draws to another block of streams: test()'s extra episode uses VISUAL_STREAM_OFFSET, so it is not eval()'s first."""
        stream0 = EVAL_STREAM0 + stream_offset + self.cfg.run_id0 * num_episodes
        out = ops.qlearn_eval(self.kind, self._tables(self._greedy_table()), num_episodes, self.cfg.seed, stream0, cap, is_slippery=self._flags()["is_slippery"])
        return tuple(t.cpu().numpy() for t in out)


def step_coin(seed, stream, k):
    """Double Q-learning's coin of (stream, k): the low bit of the word whose top bits are the exploring action."""
    return philox4x32(seed, stream & 0xFFFFFFFF, stream >> 32, k, RNG_TABULAR)[2] & 1


class TabularTD(TabularQLearning):
    """The same population under Config.rule: "sarsa", "expected_sarsa", "double_q" or "qlearning" (include/gymrl.h states
    the loops; csrc/tabular.hip's gymrl_tabular_train runs them).  Double Q-learning keeps its second table in self.Q2 and acts
    and evaluates on Q + Q2.  select_action() / update() restate the rule on the host for one run: SARSA's update takes the
    next action, Expected SARSA's uses the epsilon select_action drew with, Double Q-learning's the coin of that draw."""

    def __init__(self, config):
        if config.rule not in ops.TABULAR_RULES:
            raise ValueError(f"rule is {config.rule!r}: one of {sorted(ops.TABULAR_RULES)}")
        super().__init__(config)
        self.rule = ops.TABULAR_RULES[config.rule]
        self.Q2 = np.zeros_like(self.Q) if config.rule == "double_q" else None
        print(f"Rule: {config.rule}")

    def _greedy_table(self):
        return self.Q if self.Q2 is None else self.Q + self.Q2

    def select_action(self, state, deterministic=False):
        self._one_run("select_action")
        if not deterministic:
            eps = self._get_epsilon()
            u, explore, _ = step_draw(self.cfg.seed, self.cfg.run_id0, self.sample_count, self.n_actions)
            if u < eps:
                return int(explore)
        return int(np.argmax(self._greedy_table()[state, :]))

    def update(self, state, action, reward, next_state, done, next_action=None):
        self._one_run("update")
        cfg, rule, Q = self.cfg, self.cfg.rule, self.Q
        if rule == "double_q" and step_coin(cfg.seed, cfg.run_id0, self.sample_count):
            Q, other = self.Q2, self.Q
        elif rule == "double_q":
            other = self.Q2
        if done:
            target = reward
        elif rule == "sarsa":
            if next_action is None:
                raise ValueError("SARSA's update needs the action select_action chose in next_state")
            target = reward + cfg.gamma * Q[next_state, next_action]
        elif rule == "expected_sarsa":
            q0, q1, q2, q3 = Q[next_state, :]
            eps = self.epsilon
            target = reward + cfg.gamma * (eps * 0.25 * (((q0 + q1) + q2) + q3) + (1.0 - eps) * max(q0, q1, q2, q3))
        elif rule == "double_q":
            target = reward + cfg.gamma * other[next_state, int(np.argmax(Q[next_state, :]))]
        else:
            target = reward + cfg.gamma * np.max(Q[next_state, :])
        predict = Q[state, action]
        Q[state, action] = predict + cfg.lr * (target - predict)

    # ---- the population on the device ----
    def _draw_budget(self):
        return ops.tabular_draws(self.rule, self.cfg.max_episodes, self.cfg.max_steps)

    def _state_bytes(self):
        return ops.tabular_state_bytes(self.rule, self.num_runs)

    def _launch(self, Q, state, eps, chunk, rew, length, k_dev, done_dev, restart):
        cfg = self.cfg
        ops.tabular_train(self.rule, self.kind, Q, state, eps, cfg.seed, cfg.run_id0, cfg.max_episodes, cfg.max_steps, chunk, cfg.lr,
                          cfg.gamma, rew, length, k_dev, done_dev, Q2=self._Q2_dev, restart=restart, **self._flags())

    def train(self):
        self._Q2_dev = None if self.Q2 is None else self._tables(self.Q2)
        super().train()
        if self.Q2 is not None:
            self.Q2 = self._Q2_dev.cpu().numpy().reshape(self.Q2.shape)
        self._Q2_dev = None
