"""PPO with a GRU (PSCN -> MLPRNN -> actor / critic heads, whole-episode recurrent updates, dual-clip objective) — MI355X
engine behind the reference's algorithms/ppo_rnn_lunarlander.py surface: Config :34-54, ActorCritic :141-166,
PPORNNTrainer :274-510 (update :317-370).  It is ppg_rnn_lunarlander.py without the aux head and the aux phase, and so is
this module: everything else (the acting launch gymrl_mlprnn_act, rounds of num_envs episodes, the GRU over whole episodes,
L5, the checkpoint) is gymrl_amd.ppg_rnn_lunarlander's.  Every parameter is in every loss, so all of them share one Adam
step count.
"""
from . import ppg_rnn_lunarlander as _ppg
from .ppg_rnn_lunarlander import MLP, MLPRNN, PSCN, initialize_weights  # noqa: F401  (part of this module's surface)


class Config:
    def __init__(self):
        self.env_name = "LunarLander-v2"
        self.seed = None
        self.max_episodes = 10000
        self.max_steps = 20000
        self.batch_size = 4
        self.epochs = 10
        self.clip = 0.2
        self.dual_clip = 3.0
        self.gamma = 0.99
        self.lamda = 0.95
        self.val_coef = 0.5
        self.ent_coef = 1e-2
        self.lr = 1e-3
        self.grad_clip = 0.5
        self.eval_freq = 10
        self.save_freq = 50
        self.device = "cuda"
        self.save_path = "./checkpoints/PPO_RNN_LunarLander.pth"
        # --- vectorised-engine additions ---
        self.num_envs = 1
        self.episodes_per_minibatch = 1
        self.fused_eval = False            # eval() as ONE launch (gymrl_lunar_mlprnn_eval), as in gymrl_amd.ppg_rnn_lunarlander
        self.fused_collect = False         # num_envs <= 16: a collection round as ONE launch (gymrl_lunar_mlprnn_collect), likewise


class ActorCritic(_ppg.ActorCriticPPG):
    """:141-166 — forward returns (prob, value)."""
    has_aux = False


class PPORNNTrainer(_ppg.PPGTrainer):
    net_cls = ActorCritic

    def _env_name(self):
        # the reference names LunarLander-v2; the v3 stepper is the only LunarLander here (same dynamics for this agent)
        return "LunarLander-v3" if self.cfg.env_name == "LunarLander-v2" else self.cfg.env_name

    def _update_print(self, metrics):
        print(f"  Update - Loss: {metrics['total_loss']:.4f}, Value: {metrics['value_loss']:.4f}")


if __name__ == "__main__":       # python -m gymrl_amd.ppo_rnn_lunarlander [--<Config attribute> <value> ...]  (:513-529)
    from .utils.cli import run_script
    run_script(Config, PPORNNTrainer)
