"""Tabular Q-learning on CliffWalking-v0 — MI355X engine behind the reference's algorithms/qlearning_cliffwalking.py surface:
Config :21-31, QLearningTrainer :34-144 (_get_epsilon :49-54, select_action :56-59, update :61-69, train :71-103,
eval :105-124, test :126-144).

`num_runs` independent runs on 48 x 4 tables train as one launch, one lane per run (gymrl_amd/tabular.py, csrc/tabular.hip).
The table is a dense array where the reference keeps a defaultdict of zero rows: the same values.  One deliberate
departure: the reference's eval() loops `while not done` and never returns for a table whose greedy path misses the goal;
here an evaluation episode stops after cfg.max_steps and is reported as not finished.
"""
import numpy as np

from . import ops
from .tabular import VISUAL_STREAM_OFFSET, TabularQLearning


class Config:
    def __init__(self):
        self.env_name = "CliffWalking-v0"
        self.seed = 42
        self.max_episodes = 500
        self.max_steps = 200
        self.lr = 0.1
        self.gamma = 0.9
        self.epsilon_start = 0.95
        self.epsilon_end = 0.01
        self.epsilon_decay = 300
        self.device = "cuda"
        # --- population additions (the defaults are the reference's single run) ---
        self.num_runs = 1                    # independent runs, one lane each; run r draws from stream run_id0 + r
        self.run_id0 = 0
        self.steps_per_launch = 0            # steps of every run per launch; 0: the whole run in one launch


class QLearningTrainer(TabularQLearning):
    kind = ops.CLIFFWALKING
    report_every = 20

    def eval(self, num_episodes: int = 20) -> list:
        print(f"\nEvaluating for {num_episodes} episodes...")
        returns, _, finished = self._evaluate(num_episodes, self.cfg.max_steps)
        self.eval_finished = finished.astype(bool)[0] if self.num_runs == 1 else finished.astype(bool)
        for episode in range(num_episodes):
            cut = "" if finished[:, episode].all() else f" (stopped at {self.cfg.max_steps} steps, not finished)"
            print(f"  Episode {episode + 1}: Reward = {returns[:, episode].mean():.0f}{cut}")
        print(f"Evaluation: Mean = {np.mean(returns):.1f} +/- {np.std(returns):.1f}")
        return returns[0].tolist() if self.num_runs == 1 else returns

    def test(self):
        self.eval(num_episodes=10)
        print("\nStarting visual test...")                 # one more greedy episode, reported instead of rendered
        returns, lengths, _ = self._evaluate(1, self.cfg.max_steps, VISUAL_STREAM_OFFSET)
        print(f"Visual Test: Reward = {returns[0, 0]:.0f}, Steps = {int(lengths[0, 0])}")


if __name__ == "__main__":
    from .utils.cli import run_script
    run_script(Config, QLearningTrainer)
