"""QR-DQN with double-Q selection and prioritised replay, on ddqn_per_cartpole.DDQNPERTrainer's loop: qrdqn_cartpole's head and
acting, DDQN + PER's sum tree, stratified draw and importance weights.  The priority error of a row is its quantile-Huber loss
(gymrl_qr_loss's row_loss_out, unweighted), the choice c51_per_cartpole.py makes for the cross-entropy; the weights multiply the
gradient and the logged loss.
"""
import torch

from . import ops
from .ddqn_per_cartpole import Config as _PERConfig
from .ddqn_per_cartpole import DDQNPERTrainer
from .qrdqn_cartpole import QRHead


class Config(_PERConfig):
    def __init__(self):
        super().__init__()
        self.num_quantiles = 51              # N, 1..64: one quantile per lane of a wave64
        self.kappa = 1.0                     # the Huber threshold
        self.error_max = 0.0                 # no clip of the priority error: a quantile-Huber loss is not a TD error bounded by 1


class QRDQNPERTrainer(QRHead, DDQNPERTrainer):
    def _update_body(self, rows, w, bias=None):
        """C51PERTrainer._update_body with the quantile-Huber loss in the projected cross-entropy's place."""
        cfg, m = self.cfg, self.memory
        self._images_stale()
        states, actions, rewards, next_states, dones = m.gather(rows)
        quant = self.policy_net(states)
        with torch.no_grad():
            next_online = self._head(self.policy_net(next_states))
            next_target = self._head(self.target_net(next_states))
        self._loss.zero_()
        row_loss, dquant = ops.qr_loss(self._head(quant), next_target, actions.view(-1), rewards, dones, cfg.gamma, cfg.kappa,
                                       next_online=next_online, w=w, loss_sum=self._loss)
        self._last_td = row_loss                                               # (kept: the errors the tree has just taken)
        m.update_rows(rows, row_loss)
        self._sink.arm()
        quant.backward(dquant.view_as(quant))
        self._sink.collect()
        self.optimizer.step(bias_dev=bias)
        return states.shape[0]


if __name__ == "__main__":       # python -m gymrl_amd.qrdqn_per_cartpole [--<Config attribute> <value> ...]
    from .utils.cli import run_script
    run_script(Config, QRDQNPERTrainer)
