"""Quantile-regression DQN (QR-DQN, Dabney et al. 2018) on dqn_cartpole.DQNTrainer's loop: the distributional learner that
needs no support.  The reference has none.

The network is DQN's trunk with a Linear(H, A * N) head: quant f32[B, A, N], quantile i of action a at a * N + i, the network's
estimate of the return's quantile at tau_i = (2 i + 1) / (2 N).  Acting takes the mean quantiles (gymrl_qr_q) to
gymrl_epsilon_greedy; the update replaces gymrl_dqn_td_loss with gymrl_qr_loss (csrc/qrdqn.hip): target selection, the Bellman
map of the target row's quantiles, the N x N quantile-Huber loss and its gradient in one row launch.  Nothing is configured
per env (no v_min / v_max, no projection, no clamp): the same Config runs on --env_name MountainCar-v0 and Acrobot-v1.  The train
loop, the replay ring, the captured hipGraph of the update, eval() and the checkpoint are DQNTrainer's.  As for the categorical
head (c51_cartpole.py, whose DistributionalHead this head is built on) there is no fused vector step and no one-launch episode
evaluator: Config.fused_step raises, eval() keeps the step loop.  qrdqn_per_cartpole.py puts the same head on the double-Q +
prioritised-replay trainer.
"""
import torch

from . import ops
from .c51_cartpole import DistributionalHead
from .dqn_cartpole import Config as _DQNConfig
from .dqn_cartpole import DQNTrainer


class Config(_DQNConfig):
    def __init__(self):
        super().__init__()
        self.num_quantiles = 51              # N, 1..64: one quantile per lane of a wave64
        self.kappa = 1.0                     # the Huber threshold: quadratic for |u| <= kappa, linear beyond
        self.double_q = False                # a* from the online net's mean quantiles (the target net's when off)


class QRHead(DistributionalHead):
    """The quantile head: N quantile locations per action, acting on their mean (gymrl_qr_q)."""
    head_name, max_actions = "quantile", ops.QR_MAX_ACTIONS

    def _check_head(self, config):
        if not ops.qr_shape_ok(0, 1, config.num_quantiles, config.kappa):
            raise ValueError(f"{type(self).__name__}: num_quantiles in 1..{ops.QR_MAX_QUANTILES} and a finite kappa > 0, not "
                             f"num_quantiles = {config.num_quantiles}, kappa = {config.kappa}")

    @staticmethod
    def _per_action(config):
        return config.num_quantiles

    def _q_values(self, state):
        return ops.qr_q(self.policy_net(state), self.action_dim, self.cfg.num_quantiles)


class QRDQNTrainer(QRHead, DQNTrainer):
    def _update_body(self, indices, bias=None):
        """C51Trainer._update_body with the quantile-Huber loss in the projected cross-entropy's place."""
        cfg = self.cfg
        self._images_stale()
        states, actions, rewards, next_states, dones = self.memory.gather(indices)
        quant = self.policy_net(states)
        with torch.no_grad():
            next_online = self._head(self.policy_net(next_states)) if cfg.double_q else None
            next_target = self._head(self.target_net(next_states))
        self._loss.zero_()
        _, dquant = ops.qr_loss(self._head(quant), next_target, actions.view(-1), rewards, dones, cfg.gamma, cfg.kappa,
                                next_online=next_online, loss_sum=self._loss)
        self._sink.arm()
        quant.backward(dquant.view_as(quant))
        self._sink.collect()
        self.optimizer.step(bias_dev=bias)
        return states.shape[0]


if __name__ == "__main__":       # python -m gymrl_amd.qrdqn_cartpole [--<Config attribute> <value> ...]
    from .utils.cli import run_script
    run_script(Config, QRDQNTrainer)
