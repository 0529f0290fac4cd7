"""SARSA, Expected SARSA and Double Q-learning on FrozenLake-v1 (4x4): qlearning_frozenlake.py's population, Config,
reward shaping and eval() / test() under another update rule (gymrl_amd/tabular.py: TabularTD; csrc/tabular.hip:
gymrl_tabular_train; no reference script).

    python -m gymrl_amd.sarsa_frozenlake --num_runs 4096                         # SARSA
    python -m gymrl_amd.sarsa_frozenlake --rule expected_sarsa --num_runs 4096
    python -m gymrl_amd.sarsa_frozenlake --rule double_q --is_slippery false --num_runs 4096
"""
from . import qlearning_frozenlake
from .tabular import TabularTD


class Config(qlearning_frozenlake.Config):
    def __init__(self):
        super().__init__()
        self.rule = "sarsa"                  # "sarsa" | "expected_sarsa" | "double_q" | "qlearning"


class TDTrainer(TabularTD, qlearning_frozenlake.QLearningTrainer):
    pass


if __name__ == "__main__":
    from .utils.cli import run_script
    run_script(Config, TDTrainer)
