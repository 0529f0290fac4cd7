"""Categorical DQN (C51, Bellemare et al. 2017) on dqn_cartpole.DQNTrainer's loop.  The reference has no distributional
learner (its Rainbow carries none either); this module adds one in the engine's own terms.

The network is DQN's trunk with a Linear(H, A * M) head: logits f32[N, A, M], atom j of action a at a * M + j, on the fixed
support z_j = v_min + j (v_max - v_min) / (M - 1).  Acting takes the expected values (gymrl_c51_q) to gymrl_epsilon_greedy;
the update replaces gymrl_dqn_td_loss with gymrl_c51_loss (csrc/c51.hip): target selection, softmax of the target row, the
projection onto the support, the cross-entropy and its gradient in one row launch.  The train loop, the replay ring, the captured
hipGraph of the update, eval() and the checkpoint are DQNTrainer's.  There is no fused vector step and no one-launch episode
evaluator for this head: Config.fused_step raises, eval() keeps the step loop.  c51_per_cartpole.py puts the same head on the
double-Q + prioritised-replay trainer.
"""
import torch

from . import ops
from .dqn_cartpole import Config as _DQNConfig
from .dqn_cartpole import DQNTrainer, QNetwork


def default_support(env_name, gamma):
    """(v_min, v_max) covering the discounted returns of an env whose reward is +1 per step (CartPole-v1: [0, 1 / (1 - gamma)])
    or -1 per step (MountainCar-v0, Acrobot-v1: [-1 / (1 - gamma), 0]), rounded so that gamma = 0.99 gives 100 and not 100.00000000000009."""
    bound = round(1.0 / (1.0 - gamma), 6)
    return (0.0, bound) if env_name == "CartPole-v1" else (-bound, 0.0)


class Config(_DQNConfig):
    def __init__(self):
        super().__init__()
        self.num_atoms = 51                  # M, 2..64: one atom per lane of a wave64
        # CartPole-v1 pays +1 per step, so a discounted return lies in [0, sum_t gamma^t] = [0, 1 / (1 - gamma)] = [0, 100] at
        # gamma = 0.99; on MountainCar-v0 / Acrobot-v1 (-1 per step) set default_support(env_name, gamma) = [-100, 0]
        self.v_min, self.v_max = default_support(self.env_name, self.gamma)
        self.double_q = False                # a* from the online net's expected values (the target net's when off)


class DistributionalHead:
    """What a head of K values per action (C51's atoms, qrdqn_cartpole.py's quantiles) changes in a DQNTrainer-family trainer:
    the network's width, the values acting is greedy on (_q_values, the subclass's), and the refusal of the fused paths, which
    know scalar Q heads only.  A subclass names itself (head_name), its width (_per_action), its action limit, and refuses a bad
    Config in _check_head."""
    head_name, max_actions = None, 8

    def __init__(self, config):
        self._check_head(config)
        if getattr(config, "fused_step", False):
            raise ValueError(f"{type(self).__name__}: there is no fused vector step for the {self.head_name} head "
                             "(Config.fused_step must stay False)")
        super().__init__(config)
        if self.action_dim > self.max_actions:
            raise ValueError(f"{type(self).__name__}: at most {self.max_actions} actions, {config.env_name} has {self.action_dim}")

    def _make_network(self, state_dim, action_dim, hidden_dim):
        return QNetwork(state_dim, action_dim * self._per_action(self.cfg), hidden_dim)

    def _head(self, out):
        """f32[N, A * K] off the last layer -> f32[N, A, K] (a view)."""
        return out.view(out.shape[0], self.action_dim, self._per_action(self.cfg))

    def _fused_update_ok(self):
        return False

    def _eval_policy(self):
        return None


class C51Head(DistributionalHead):
    """The categorical head: M atoms per action on [v_min, v_max], acting on their expected values (gymrl_c51_q)."""
    head_name, max_actions = "categorical", ops.C51_MAX_ACTIONS

    def _check_head(self, config):
        M = config.num_atoms
        if not ops.c51_shape_ok(0, 1, M, config.v_min, config.v_max):
            raise ValueError(f"{type(self).__name__}: num_atoms in 2..{ops.C51_MAX_ATOMS} and v_min < v_max, not {M} atoms on "
                             f"[{config.v_min}, {config.v_max}]")

    @staticmethod
    def _per_action(config):
        return config.num_atoms

    def _q_values(self, state):
        cfg = self.cfg
        return ops.c51_q(self.policy_net(state), self.action_dim, cfg.num_atoms, cfg.v_min, cfg.v_max)


class C51Trainer(C51Head, DQNTrainer):
    def _update_body(self, indices, bias=None):
        """DQNTrainer._update_body with the projected cross-entropy in gymrl_dqn_td_loss's place."""
        cfg = self.cfg
        self._images_stale()
        states, actions, rewards, next_states, dones = self.memory.gather(indices)
        logits = self.policy_net(states)
        with torch.no_grad():
            next_online = self._head(self.policy_net(next_states)) if cfg.double_q else None
            next_target = self._head(self.target_net(next_states))
        self._loss.zero_()
        _, dlogits = ops.c51_loss(self._head(logits), next_target, actions.view(-1), rewards, dones, cfg.gamma, cfg.v_min, cfg.v_max,
                                  next_online=next_online, loss_sum=self._loss)
        self._sink.arm()
        logits.backward(dlogits.view_as(logits))
        self._sink.collect()
        self.optimizer.step(bias_dev=bias)
        return states.shape[0]


if __name__ == "__main__":       # python -m gymrl_amd.c51_cartpole [--<Config attribute> <value> ...]
    from .utils.cli import run_script
    run_script(Config, C51Trainer)
