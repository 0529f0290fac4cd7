"""Dueling double DQN + prioritised replay — MI355X engine behind the reference's algorithms/ddqn_per_duel_cartpole.py surface:
Config :35-55, DuelingQNetwork :58-78, SumTree :81-122, PrioritizedReplayBuffer :125-168, DDQNPERDuelTrainer :171-349.

ddqn_per_cartpole.py with another network: one hidden layer, then a value head and an advantage head, Q = V + (A - mean A).
The buffer, the sum tree and the trainer are that module's; on the layer-by-layer path the combine and its backward go through
autograd.  With Config.fused_step the dueling instances of csrc/ddqn_step.hip run (gymrl_ddqn_update with dueling = 1,
gymrl_ddqn_duel_act_step): the same arithmetic, the same bits.  With Config.fused_eval, eval() is one launch of whole episodes
(csrc/eval_duel.hip): the same list.
"""
import torch.nn as nn

from . import ops
from .ddqn_per_cartpole import Config, DDQNPERTrainer, PrioritizedReplayBuffer, SumTree  # noqa: F401  (the script's surface)
from .nn import SmallLinear


class DuelingQNetwork(nn.Module):
    """ddqn_per_duel_cartpole.py:58-78 (same module tree and nn.Linear's default init, so reference state_dicts load unchanged)."""

    def __init__(self, state_dim, action_dim, hidden_dim=256):
        super().__init__()
        self.fc1 = SmallLinear(state_dim, hidden_dim, act="relu")
        self.value_stream = SmallLinear(hidden_dim, 1)
        self.advantage_stream = SmallLinear(hidden_dim, action_dim)

    def forward(self, x):
        x = self.fc1(x)
        value = self.value_stream(x)
        advantage = self.advantage_stream(x)
        return value + (advantage - advantage.mean(dim=-1, keepdim=True))


class DDQNPERDuelTrainer(DDQNPERTrainer):
    DUELING = True
    _act_step = staticmethod(ops.ddqn_duel_act_step)

    def _make_network(self, state_dim, action_dim, hidden_dim):
        return DuelingQNetwork(state_dim, action_dim, hidden_dim)

    @staticmethod
    def _layers(net):
        return net.fc1, net.value_stream, net.advantage_stream

    def _eval_duel_policy(self):
        """eval() acts greedily on fc1 -> value_stream + advantage_stream (csrc/eval_duel.hip).  (_eval_policy() stays
        None: the network is no three-layer MLP.)"""
        net = self.policy_net
        pair = lambda m: (m.weight, m.bias)     # noqa: E731
        return [pair(net.fc1)], pair(net.value_stream), pair(net.advantage_stream), self.flat_params


if __name__ == "__main__":       # python -m gymrl_amd.ddqn_per_duel_cartpole [--<Config attribute> <value> ...]  (:352-368)
    from .utils.cli import run_script
    run_script(Config, DDQNPERDuelTrainer)
