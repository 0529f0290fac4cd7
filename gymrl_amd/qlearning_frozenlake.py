"""Tabular Q-learning on FrozenLake-v1 — MI355X engine behind the reference's algorithms/qlearning_frozenlake.py surface:
Config :20-33, QLearningTrainer :36-177 (_get_epsilon :56-61, _shape_reward :63-79, select_action :81-84, update :86-94,
train :96-129, eval :131-153, test :155-177).

One run is a serial chain on a 16 x 4 table; `num_runs` of them — the learning curve over a thousand seeds — train as one
launch, one lane per run (gymrl_amd/tabular.py, csrc/tabular.hip).  The env is the kernel's own FrozenLake (include/gymrl.h
states its rules); its draws are counter-keyed Philox streams, not np.random's.
"""
from . import ops
from .tabular import VISUAL_STREAM_OFFSET, TabularQLearning


class Config:
    def __init__(self):
        self.env_name = "FrozenLake-v1"
        self.map_name = "4x4"
        self.is_slippery = True
        self.seed = 42
        self.max_episodes = 500
        self.max_steps = 100
        self.lr = 0.1
        self.gamma = 0.9
        self.epsilon_start = 0.95
        self.epsilon_end = 0.01
        self.epsilon_decay = 200
        self.use_reward_shaping = True
        self.device = "cuda"
        # --- population additions (the defaults are the reference's single run) ---
        self.num_runs = 1                    # independent runs, one lane each; run r draws from stream run_id0 + r
        self.run_id0 = 0
        self.steps_per_launch = 0            # steps of every run per launch; 0: the whole run in one launch


class QLearningTrainer(TabularQLearning):
    kind = ops.FROZENLAKE
    report_every = 50
    env_limit = 100                          # the env's own TimeLimit: evaluation episodes end by it

    def __init__(self, config: Config):
        if config.map_name != "4x4":
            raise ValueError("the FrozenLake kernel is the 4x4 map")
        super().__init__(config)

    def _shape_reward(self, state, next_state, reward, done):
        if not self.cfg.use_reward_shaping:
            return reward
        if next_state in (5, 7, 11, 12):
            return -10.0
        elif next_state == 15:
            return 100.0
        elif state == next_state:
            return -5.0
        return -1.0

    def eval(self, num_episodes: int = 20) -> list:
        print(f"\nEvaluating for {num_episodes} episodes...")
        returns, _, success = self._evaluate(num_episodes, self.env_limit)
        print(f"Evaluation: Success Rate = {success.mean() * 100:.1f}%")
        return returns[0].tolist() if self.num_runs == 1 else returns

    def test(self):
        self.eval(num_episodes=20)
        print("\nStarting visual test...")                 # one more greedy episode, reported instead of rendered
        returns, lengths, success = self._evaluate(1, self.env_limit, VISUAL_STREAM_OFFSET)
        result = "SUCCESS" if success[0, 0] else "FAIL"
        print(f"Visual Test: {result} in {int(lengths[0, 0])} steps")


if __name__ == "__main__":
    from .utils.cli import run_script
    run_script(Config, QLearningTrainer)
