"""SARSA, Expected SARSA and Double Q-learning on CliffWalking-v0: qlearning_cliffwalking.py's population, Config and
eval() / test() under another update rule (gymrl_amd/tabular.py: TabularTD; csrc/tabular.hip: gymrl_tabular_train; no
reference script).  The textbook comparison, as a distribution over seeds:

    python -m gymrl_amd.sarsa_cliffwalking --num_runs 4096                       # SARSA
    python -m gymrl_amd.sarsa_cliffwalking --rule expected_sarsa --num_runs 4096
    python -m gymrl_amd.sarsa_cliffwalking --rule double_q --num_runs 4096
    python -m gymrl_amd.sarsa_cliffwalking --rule qlearning --num_runs 4096      # qlearning_cliffwalking.py's bits
"""
from . import qlearning_cliffwalking
from .tabular import TabularTD


class Config(qlearning_cliffwalking.Config):
    def __init__(self):
        super().__init__()
        self.rule = "sarsa"                  # "sarsa" | "expected_sarsa" | "double_q" | "qlearning"


class TDTrainer(TabularTD, qlearning_cliffwalking.QLearningTrainer):
    pass


if __name__ == "__main__":
    from .utils.cli import run_script
    run_script(Config, TDTrainer)
