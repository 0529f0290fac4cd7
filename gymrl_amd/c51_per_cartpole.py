"""Categorical DQN with double-Q selection and prioritised replay, on ddqn_per_cartpole.DDQNPERTrainer's loop: c51_cartpole's
head and acting, DDQN + PER's sum tree, stratified draw and importance weights.  The priority error of a row is its
cross-entropy (gymrl_c51_loss's row_loss_out, unweighted), as in the Rainbow paper (Hessel et al. 2018, section "The
integrated agent"); the weights multiply the gradient and the logged loss.
"""
import torch

from . import ops
from .c51_cartpole import C51Head, default_support
from .ddqn_per_cartpole import Config as _PERConfig
from .ddqn_per_cartpole import DDQNPERTrainer


class Config(_PERConfig):
    def __init__(self):
        super().__init__()
        self.num_atoms = 51                  # M, 2..64: one atom per lane of a wave64
        # +1 per step: returns in [0, 1 / (1 - gamma)] = [0, 10] at this trainer's gamma = 0.9 (c51_cartpole.default_support)
        self.v_min, self.v_max = default_support(self.env_name, self.gamma)
        self.error_max = 0.0                 # no clip of the priority error: a cross-entropy is not a TD error bounded by 1


class C51PERTrainer(C51Head, DDQNPERTrainer):
    def _update_body(self, rows, w, bias=None):
        """DDQNPERTrainer._update_body with the projected cross-entropy in gymrl_dqn_td_loss's place."""
        cfg, m = self.cfg, self.memory
        self._images_stale()
        states, actions, rewards, next_states, dones = m.gather(rows)
        logits = self.policy_net(states)
        with torch.no_grad():
            next_online = self._head(self.policy_net(next_states))
            next_target = self._head(self.target_net(next_states))
        self._loss.zero_()
        row_loss, dlogits = ops.c51_loss(self._head(logits), next_target, actions.view(-1), rewards, dones, cfg.gamma, cfg.v_min,
                                         cfg.v_max, next_online=next_online, w=w, loss_sum=self._loss)
        self._last_td = row_loss                                               # (kept: the errors the tree has just taken)
        m.update_rows(rows, row_loss)
        self._sink.arm()
        logits.backward(dlogits.view_as(logits))
        self._sink.collect()
        self.optimizer.step(bias_dev=bias)
        return states.shape[0]


if __name__ == "__main__":       # python -m gymrl_amd.c51_per_cartpole [--<Config attribute> <value> ...]
    from .utils.cli import run_script
    run_script(Config, C51PERTrainer)
