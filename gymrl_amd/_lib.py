"""Loader for libgymrl_hip.so (the C-ABI of include/gymrl.h).

The library is built in-tree by gymrl_amd/csrc/Makefile (hipcc --offload-arch=gfx950)
and lives next to this file so that it travels with the repo snapshot.  Loading
never silently degrades: a missing library raises at first use.
"""
import ctypes as C
import os
import subprocess

# PyTorch-ROCm owns device memory and streams; importing it FIRST makes the process use
# one HIP runtime (torch's bundled libamdhip64) for both torch and this library.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GYMRL_HIP_LIB") or os.path.join(_HERE, "libgymrl_hip.so")   # override: A/B builds
CSRC = os.path.join(_HERE, "csrc")

ABI_VERSION = 4      # == GYMRL_ABI_VERSION of the include/gymrl.h this front-end was written against

_lib = None

def build(force=False):
    """Compile the HIP library in-tree (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    return LIB_PATH


class LinItem(C.Structure):
    _c_name_ = "gymrl_lin_item"
    _fields_ = ([(n, C.c_void_p) for n in ("x", "x2", "w", "b", "y", "dy", "dx", "dx2", "dw", "db")] +
                [("act", C.c_int), ("lo", C.c_float), ("hi", C.c_float), ("argmax", C.c_void_p)])


class NoisyLayer(C.Structure):
    _c_name_ = "gymrl_noisy_layer"
    _fields_ = ([(n, C.c_void_p) for n in ("w_mu", "w_sigma", "w_eps", "b_mu", "b_sigma", "b_eps", "w_eps_copy", "b_eps_copy",
                                          "dw_mu", "dw_sigma", "db_mu", "db_sigma")] +
                [("seed", C.c_uint64), ("counter", C.c_uint64), ("counter_dev", C.c_void_p), ("draw", C.c_int),
                 ("eval", C.c_int), ("n_out", C.c_int)])


class MhcSub(C.Structure):
    _c_name_ = "gymrl_mhc_sub"
    _fields_ = [(n, C.c_void_p) for n in ("norm_w", "w", "alpha", "beta", "lin_w", "lin_b")]


class MhcHead(C.Structure):
    _c_name_ = "gymrl_mhc_head"
    _fields_ = [("w1", C.c_void_p), ("b1", C.c_void_p), ("norm_w", C.c_void_p), ("norm_eps", C.c_float), ("w2", C.c_void_p),
                ("b2", C.c_void_p)]


class MhcPolicy(C.Structure):
    _c_name_ = "gymrl_mhc_policy"
    _fields_ = [("obs_dim", C.c_int), ("n_sub", C.c_int), ("n_act", C.c_int), ("sk_it", C.c_int), ("in_w", C.c_void_p),
                ("in_b", C.c_void_p), ("sub", MhcSub * 8), ("final_norm_w", C.c_void_p), ("final_norm_eps", C.c_float),
                ("head", MhcHead * 2), ("image", C.c_void_p)]


class PPOCfg(C.Structure):
    _c_name_ = "gymrl_ppo_cfg"
    _fields_ = [("clip_eps", C.c_float), ("dual_clip", C.c_float), ("value_coef", C.c_float),
                ("entropy_coef", C.c_float)]


class GaeOnline(C.Structure):
    _c_name_ = "gymrl_gae_online"
    _fields_ = [("rew_prev", C.c_void_p), ("done_prev", C.c_void_p), ("val_prev", C.c_void_p),
                ("running", C.c_void_p), ("gae_workspace", C.c_void_p), ("t_prev", C.c_int), ("T", C.c_int),
                ("gamma", C.c_double), ("lam", C.c_double), ("lam2", C.c_double), ("running2", C.c_void_p)]


MLP_MAX_STAGES, MLP_MAX_WIDTH, MLP_MAX_INPUT = 8, 256, 64
ACT_NONE, ACT_TANH, ACT_RELU = 0, 1, 2


class MlpStage(C.Structure):
    _c_name_ = "gymrl_mlp_stage"
    _fields_ = [("W", C.c_void_p), ("b", C.c_void_p), ("out", C.c_void_p), ("in_dim", C.c_int),
                ("out_dim", C.c_int), ("act", C.c_int), ("src", C.c_int), ("dst", C.c_int), ("out_stride", C.c_int)]


class MlpDesc(C.Structure):
    _c_name_ = "gymrl_mlp_desc"
    _fields_ = [("n_stages", C.c_int), ("stage", MlpStage * MLP_MAX_STAGES)]


class MlpPackLayer(C.Structure):
    _c_name_ = "gymrl_mlp_pack_layer"
    _fields_ = [("out_dim", C.c_int), ("in_dim", C.c_int), ("w_off", C.c_int64), ("b_off", C.c_int64), ("w_at", C.c_int64),
                ("b_at", C.c_int64)]


class MlpPackStackArgs(C.Structure):
    _c_name_ = "gymrl_mlp_pack_stack_args"
    _fields_ = [("P", C.c_int), ("n_layers", C.c_int), ("params", C.c_void_p), ("params_stride", C.c_int64),
                ("packed", C.c_void_p), ("packed_stride", C.c_int64), ("layer", MlpPackLayer * MLP_MAX_STAGES)]


class RolloutLunarArgs(C.Structure):
    _c_name_ = "gymrl_rollout_lunar_args"
    _fields_ = [("env_state", C.c_void_p), ("n_envs", C.c_int), ("seed", C.c_uint64), ("env_id0", C.c_int64),
                ("counter0", C.c_uint64), ("obs", C.c_void_p), ("act", C.c_void_p), ("logp", C.c_void_p),
                ("val", C.c_void_p), ("rew", C.c_void_p), ("done", C.c_void_p), ("ep_ret", C.c_void_p),
                ("next_value", C.c_void_p), ("noise_exp", C.c_void_p), ("gae_running", C.c_void_p),
                ("gae_workspace", C.c_void_p), ("gamma", C.c_double), ("lam", C.c_double), ("ep_stats", C.c_void_p),
                ("wg_ticks", C.c_void_p), ("T", C.c_int), ("t0", C.c_int), ("nsteps", C.c_int),
                ("ent", C.c_void_p), ("lam2", C.c_double), ("gae_running2", C.c_void_p),   # gymrl_rollout_lunar_mhc only
                ("refill", C.c_int), ("gae_carry", C.c_int)]


class RolloutPendulumArgs(C.Structure):
    _c_name_ = "gymrl_rollout_pendulum_args"
    _fields_ = [("env_state", C.c_void_p), ("n_envs", C.c_int), ("seed", C.c_uint64), ("env_id0", C.c_int64),
                ("counter0", C.c_uint64), ("obs", C.c_void_p), ("act", C.c_void_p), ("logp", C.c_void_p),
                ("val", C.c_void_p), ("rew", C.c_void_p), ("done", C.c_void_p), ("ep_ret", C.c_void_p),
                ("next_value", C.c_void_p), ("log_std", C.c_void_p), ("noise_normal", C.c_void_p), ("reward_scale", C.c_float),
                ("gae_running", C.c_void_p), ("gae_workspace", C.c_void_p), ("gamma", C.c_double), ("lam", C.c_double),
                ("ep_stats", C.c_void_p), ("T", C.c_int), ("t0", C.c_int), ("nsteps", C.c_int)]


class LunarEvalArgs(C.Structure):
    _c_name_ = "gymrl_lunar_eval_args"
    _fields_ = [("P", C.c_int), ("E", C.c_int), ("cap", C.c_int), ("seed", C.c_uint64), ("stream_id0", C.c_int64),
                ("policy_stride", C.c_int64), ("returns", C.c_void_p), ("lengths", C.c_void_p), ("terminated", C.c_void_p),
                ("terminal_obs", C.c_void_p)]


class ClassicPpoEvalArgs(C.Structure):
    _c_name_ = "gymrl_classic_ppo_eval_args"
    _fields_ = [("P", C.c_int), ("E", C.c_int), ("cap", C.c_int), ("env_kind", C.c_int), ("seed", C.c_uint64),
                ("stream_id0", C.c_int64), ("policy_stride", C.c_int64), ("returns", C.c_void_p), ("lengths", C.c_void_p),
                ("terminated", C.c_void_p), ("final_obs", C.c_void_p)]


class PendulumPpoEvalArgs(C.Structure):
    _c_name_ = "gymrl_pendulum_ppo_eval_args"
    _fields_ = [("P", C.c_int), ("E", C.c_int), ("cap", C.c_int), ("seed", C.c_uint64), ("stream_id0", C.c_int64),
                ("policy_stride", C.c_int64), ("returns", C.c_void_p), ("lengths", C.c_void_p), ("terminated", C.c_void_p),
                ("final_obs", C.c_void_p)]


class LunarCollectArgs(C.Structure):
    _c_name_ = "gymrl_lunar_collect_args"
    _fields_ = ([("N", C.c_int), ("cap", C.c_int), ("seed", C.c_uint64), ("env_id0", C.c_int64), ("counter0", C.c_uint64),
                 ("gamma", C.c_double)] +
                [(n, C.c_void_p) for n in ("norm_stats", "reward_stats", "R", "states", "act", "logp", "value", "rew", "done",
                                          "dw", "live", "ep_ret", "lengths")])


class SacActorParams(C.Structure):
    _c_name_ = "gymrl_sac_actor_params"   # fc1, fc2, mean, log_std
    _fields_ = [("w", C.c_void_p * 4), ("b", C.c_void_p * 4)]


class SacCriticParams(C.Structure):
    _c_name_ = "gymrl_sac_critic_params"   # fc1..fc6
    _fields_ = [("w", C.c_void_p * 6), ("b", C.c_void_p * 6)]


class SacActArgs(C.Structure):
    _c_name_ = "gymrl_sac_act_args"
    _fields_ = [("N", C.c_int), ("D", C.c_int), ("A", C.c_int), ("H", C.c_int), ("env_kind", C.c_int),
                ("env_state", C.c_void_p), ("env_seed", C.c_uint64), ("env_id0", C.c_int64),
                ("obs", C.c_void_p), ("obs_out", C.c_void_p), ("eps", C.c_void_p),
                ("noise_seed", C.c_uint64), ("noise_counter", C.c_uint64), ("noise_counter_dev", C.c_void_p),
                ("bound", C.c_float), ("log_std_min", C.c_float), ("log_std_max", C.c_float),
                ("actor", SacActorParams),
                ("r_state", C.c_void_p), ("r_action", C.c_void_p), ("r_reward", C.c_void_p), ("r_next", C.c_void_p),
                ("r_flag", C.c_void_p), ("cap", C.c_int64), ("cursor", C.c_int64), ("cursor_dev", C.c_void_p),
                ("action_out", C.c_void_p), ("rew_out", C.c_void_p), ("done_out", C.c_void_p), ("ep_ret_out", C.c_void_p),
                ("ep_stats", C.c_void_p), ("images", C.c_void_p)]


class SacUpdateArgs(C.Structure):
    _c_name_ = "gymrl_sac_update_args"
    _fields_ = [("B", C.c_int), ("D", C.c_int), ("A", C.c_int), ("H", C.c_int),
                ("gamma", C.c_float), ("bound", C.c_float), ("log_std_min", C.c_float), ("log_std_max", C.c_float),
                ("target_entropy", C.c_float), ("tau", C.c_double),
                ("r_state", C.c_void_p), ("r_action", C.c_void_p), ("r_reward", C.c_void_p), ("r_next", C.c_void_p),
                ("r_flag", C.c_void_p),
                ("idx", C.c_void_p), ("idx_seed", C.c_uint64), ("idx_counter", C.c_uint64), ("idx_size", C.c_int64),
                ("idx_dev", C.c_void_p),
                ("eps_next", C.c_void_p), ("eps_cur", C.c_void_p),
                ("noise_seed", C.c_uint64), ("noise_counter", C.c_uint64), ("noise_counter_dev", C.c_void_p),
                ("actor", SacActorParams), ("critic", SacCriticParams), ("target", SacCriticParams),
                ("actor_p", C.c_void_p), ("actor_m", C.c_void_p), ("actor_v", C.c_void_p),
                ("critic_p", C.c_void_p), ("critic_m", C.c_void_p), ("critic_v", C.c_void_p),
                ("adam_critic", C.c_float * 4), ("adam_actor", C.c_float * 4),
                ("adam_critic_dev", C.c_void_p), ("adam_actor_dev", C.c_void_p),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps_adam", C.c_double),
                ("log_alpha", C.c_void_p), ("alpha_m", C.c_void_p), ("alpha_v", C.c_void_p), ("lr_alpha", C.c_double),
                ("alpha_bias", C.c_double * 2), ("alpha_bias_dev", C.c_void_p),
                ("sums", C.c_void_p), ("alpha_loss", C.c_void_p), ("workspace", C.c_void_p), ("images", C.c_void_p)]


class RainbowActArgs(C.Structure):
    _c_name_ = "gymrl_rainbow_act_args"
    _fields_ = [("N", C.c_int), ("D", C.c_int), ("A", C.c_int), ("H", C.c_int), ("env_kind", C.c_int),
                ("env_state", C.c_void_p), ("env_seed", C.c_uint64), ("env_id0", C.c_int64),
                ("obs", C.c_void_p), ("obs_out", C.c_void_p),
                ("fc1_w", C.c_void_p), ("fc1_b", C.c_void_p), ("fc2_w", C.c_void_p), ("fc2_b", C.c_void_p),
                ("head_w", C.c_void_p), ("head_b", C.c_void_p), ("max_episode_steps", C.c_int),
                ("w_state", C.c_void_p), ("w_action", C.c_void_p), ("w_reward", C.c_void_p), ("w_next", C.c_void_p),
                ("w_terminal", C.c_void_p), ("w_done", C.c_void_p),
                ("n_steps", C.c_int), ("pushes", C.c_int64), ("gamma", C.c_double),
                ("r_state", C.c_void_p), ("r_action", C.c_void_p), ("r_reward", C.c_void_p), ("r_next", C.c_void_p),
                ("r_flag", C.c_void_p), ("cap", C.c_int64), ("cursor", C.c_int64), ("push_dev", C.c_void_p),
                ("action_out", C.c_void_p), ("rew_out", C.c_void_p), ("done_out", C.c_void_p), ("ep_ret_out", C.c_void_p),
                ("ep_stats", C.c_void_p), ("fc2_img", C.c_void_p)]


class RainbowUpdateArgs(C.Structure):
    _c_name_ = "gymrl_rainbow_update_args"
    _fields_ = [("B", C.c_int), ("D", C.c_int), ("A", C.c_int), ("H", C.c_int), ("gamma_n", C.c_float),
                ("r_state", C.c_void_p), ("r_action", C.c_void_p), ("r_reward", C.c_void_p), ("r_next", C.c_void_p),
                ("r_flag", C.c_void_p), ("idx", C.c_void_p), ("is_weight", C.c_void_p),
                ("p_fc1_w", C.c_void_p), ("p_fc1_b", C.c_void_p), ("p_fc2_w", C.c_void_p), ("p_fc2_b", C.c_void_p),
                ("t_fc1_w", C.c_void_p), ("t_fc1_b", C.c_void_p), ("t_fc2_w", C.c_void_p), ("t_fc2_b", C.c_void_p),
                ("head_w", C.c_void_p), ("head_b", C.c_void_p), ("td_out", C.c_void_p), ("loss_sum", C.c_void_p),
                ("d_fc1_w", C.c_void_p), ("d_fc1_b", C.c_void_p), ("d_fc2_w", C.c_void_p), ("d_fc2_b", C.c_void_p),
                ("d_head_w", C.c_void_p), ("d_head_b", C.c_void_p), ("workspace", C.c_void_p),
                ("split_heads", C.c_int), ("dw_mu", C.c_void_p * 2), ("dw_sigma", C.c_void_p * 2), ("db_mu", C.c_void_p * 2),
                ("db_sigma", C.c_void_p * 2), ("w_eps", C.c_void_p * 2), ("b_eps", C.c_void_p * 2),
                ("p_fc2_img_f", C.c_void_p), ("p_fc2_img_b", C.c_void_p), ("t_fc2_img_f", C.c_void_p)]


class Td3ActorParams(C.Structure):
    _c_name_ = "gymrl_td3_actor_params"   # fc1, fc2, fc3
    _fields_ = [("w", C.c_void_p * 3), ("b", C.c_void_p * 3)]


class Td3ActArgs(C.Structure):
    _c_name_ = "gymrl_td3_act_args"
    _fields_ = [("N", C.c_int), ("D", C.c_int), ("A", C.c_int), ("H", C.c_int), ("env_kind", C.c_int),
                ("env_state", C.c_void_p), ("env_seed", C.c_uint64), ("env_id0", C.c_int64),
                ("obs", C.c_void_p), ("obs_out", C.c_void_p), ("eps", C.c_void_p),
                ("noise_seed", C.c_uint64), ("noise_counter", C.c_uint64), ("noise_counter_dev", C.c_void_p),
                ("bound", C.c_float), ("noise_std", C.c_double),
                ("actor", Td3ActorParams),
                ("r_state", C.c_void_p), ("r_action", C.c_void_p), ("r_reward", C.c_void_p), ("r_next", C.c_void_p),
                ("r_flag", C.c_void_p), ("cap", C.c_int64), ("cursor", C.c_int64), ("cursor_dev", C.c_void_p),
                ("action_out", C.c_void_p), ("rew_out", C.c_void_p), ("done_out", C.c_void_p), ("ep_ret_out", C.c_void_p),
                ("ep_stats", C.c_void_p), ("images", C.c_void_p)]


class Td3UpdateArgs(C.Structure):
    _c_name_ = "gymrl_td3_update_args"
    _fields_ = [("B", C.c_int), ("D", C.c_int), ("A", C.c_int), ("H", C.c_int), ("n_critics", C.c_int),
                ("gamma", C.c_float), ("bound", C.c_float), ("noise_clip", C.c_float),
                ("policy_noise", C.c_double), ("tau", C.c_double),
                ("r_state", C.c_void_p), ("r_action", C.c_void_p), ("r_reward", C.c_void_p), ("r_next", C.c_void_p),
                ("r_flag", C.c_void_p),
                ("idx", C.c_void_p), ("idx_seed", C.c_uint64), ("idx_counter", C.c_uint64), ("idx_size", C.c_int64),
                ("idx_dev", C.c_void_p), ("eps", C.c_void_p),
                ("noise_seed", C.c_uint64), ("noise_counter", C.c_uint64), ("noise_counter_dev", C.c_void_p),
                ("delayed", C.c_int), ("delayed_dev", C.c_void_p),
                ("actor", Td3ActorParams), ("actor_target", Td3ActorParams),
                ("critic", SacCriticParams), ("critic_target", SacCriticParams),
                ("actor_p", C.c_void_p), ("actor_m", C.c_void_p), ("actor_v", C.c_void_p),
                ("critic_p", C.c_void_p), ("critic_m", C.c_void_p), ("critic_v", C.c_void_p),
                ("adam_critic", C.c_float * 4), ("adam_actor", C.c_float * 4),
                ("adam_critic_dev", C.c_void_p), ("adam_actor_dev", C.c_void_p),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps_adam", C.c_double),
                ("sums", C.c_void_p), ("workspace", C.c_void_p), ("images", C.c_void_p)]


class DsacActArgs(C.Structure):
    _c_name_ = "gymrl_dsac_act_args"
    _fields_ = [("N", C.c_int), ("D", C.c_int), ("A", C.c_int), ("H", C.c_int), ("env_kind", C.c_int),
                ("env_state", C.c_void_p), ("env_seed", C.c_uint64), ("env_id0", C.c_int64),
                ("obs", C.c_void_p), ("obs_out", C.c_void_p), ("noise_exp", C.c_void_p),
                ("seed", C.c_uint64), ("counter", C.c_uint64), ("counter_dev", C.c_void_p),
                ("actor", Td3ActorParams),
                ("r_state", C.c_void_p), ("r_action", C.c_void_p), ("r_reward", C.c_void_p), ("r_next", C.c_void_p),
                ("r_flag", C.c_void_p), ("cap", C.c_int64), ("cursor", C.c_int64), ("cursor_dev", C.c_void_p),
                ("action_out", C.c_void_p), ("rew_out", C.c_void_p), ("done_out", C.c_void_p), ("ep_ret_out", C.c_void_p),
                ("ep_stats", C.c_void_p), ("images", C.c_void_p)]


class DsacUpdateArgs(C.Structure):
    _c_name_ = "gymrl_dsac_update_args"
    _fields_ = [("B", C.c_int), ("D", C.c_int), ("A", C.c_int), ("H", C.c_int),
                ("gamma", C.c_float), ("target_entropy", C.c_float), ("tau", C.c_double),
                ("r_state", C.c_void_p), ("r_action", C.c_void_p), ("r_reward", C.c_void_p), ("r_next", C.c_void_p),
                ("r_flag", C.c_void_p),
                ("idx", C.c_void_p), ("idx_seed", C.c_uint64), ("idx_counter", C.c_uint64), ("idx_size", C.c_int64),
                ("idx_dev", C.c_void_p),
                ("actor", Td3ActorParams), ("critic1", Td3ActorParams), ("critic2", Td3ActorParams),
                ("critic1_target", Td3ActorParams), ("critic2_target", Td3ActorParams),
                ("actor_p", C.c_void_p), ("actor_m", C.c_void_p), ("actor_v", C.c_void_p),
                ("critic1_p", C.c_void_p), ("critic1_m", C.c_void_p), ("critic1_v", C.c_void_p),
                ("critic2_p", C.c_void_p), ("critic2_m", C.c_void_p), ("critic2_v", C.c_void_p),
                ("adam_critic1", C.c_float * 4), ("adam_critic2", C.c_float * 4), ("adam_actor", C.c_float * 4),
                ("adam_critic1_dev", C.c_void_p), ("adam_critic2_dev", C.c_void_p), ("adam_actor_dev", C.c_void_p),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps_adam", C.c_double),
                ("log_alpha", C.c_void_p), ("alpha_m", C.c_void_p), ("alpha_v", C.c_void_p),
                ("lr_alpha", C.c_double), ("alpha_beta1", C.c_double), ("alpha_beta2", C.c_double), ("alpha_eps", C.c_double),
                ("alpha_t", C.c_int64), ("alpha_bias_dev", C.c_void_p),
                ("sums", C.c_void_p), ("alpha_loss", C.c_void_p), ("workspace", C.c_void_p), ("images", C.c_void_p)]


class DqnActArgs(C.Structure):
    _c_name_ = "gymrl_dqn_act_args"
    _fields_ = [("N", C.c_int), ("D", C.c_int), ("A", C.c_int), ("H", C.c_int), ("env_kind", C.c_int),
                ("env_state", C.c_void_p), ("env_seed", C.c_uint64), ("env_id0", C.c_int64),
                ("obs", C.c_void_p), ("obs_out", C.c_void_p), ("u", C.c_void_p),
                ("seed", C.c_uint64), ("counter", C.c_uint64), ("counter_dev", C.c_void_p),
                ("epsilon", C.c_float), ("epsilon_dev", C.c_void_p),
                ("policy", Td3ActorParams),
                ("r_state", C.c_void_p), ("r_action", C.c_void_p), ("r_reward", C.c_void_p), ("r_next", C.c_void_p),
                ("r_flag", C.c_void_p), ("cap", C.c_int64), ("cursor", C.c_int64), ("cursor_dev", C.c_void_p),
                ("action_out", C.c_void_p), ("rew_out", C.c_void_p), ("done_out", C.c_void_p), ("ep_ret_out", C.c_void_p),
                ("ep_stats", C.c_void_p), ("images", C.c_void_p)]


class DqnUpdateArgs(C.Structure):
    _c_name_ = "gymrl_dqn_update_args"
    _fields_ = [("B", C.c_int), ("D", C.c_int), ("A", C.c_int), ("H", C.c_int), ("gamma", C.c_float),
                ("r_state", C.c_void_p), ("r_action", C.c_void_p), ("r_reward", C.c_void_p), ("r_next", C.c_void_p),
                ("r_flag", C.c_void_p),
                ("idx", C.c_void_p), ("idx_seed", C.c_uint64), ("idx_counter", C.c_uint64), ("idx_size", C.c_int64),
                ("idx_dev", C.c_void_p),
                ("policy", Td3ActorParams), ("target", Td3ActorParams),
                ("policy_p", C.c_void_p), ("policy_m", C.c_void_p), ("policy_v", C.c_void_p),
                ("adam_policy", C.c_float * 4), ("adam_policy_dev", C.c_void_p),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps_adam", C.c_double),
                ("clamp_abs", C.c_float), ("loss_sum", C.c_void_p), ("workspace", C.c_void_p), ("images", C.c_void_p)]


class DdqnUpdateArgs(C.Structure):
    _c_name_ = "gymrl_ddqn_update_args"
    _fields_ = [("B", C.c_int), ("D", C.c_int), ("A", C.c_int), ("H", C.c_int), ("dueling", C.c_int), ("gamma", C.c_float),
                ("r_state", C.c_void_p), ("r_action", C.c_void_p), ("r_reward", C.c_void_p), ("r_next", C.c_void_p),
                ("r_flag", C.c_void_p), ("cap", C.c_int64), ("idx", C.c_void_p), ("is_weight", C.c_void_p),
                ("policy", Td3ActorParams), ("target", Td3ActorParams),
                ("policy_p", C.c_void_p), ("policy_m", C.c_void_p), ("policy_v", C.c_void_p),
                ("adam_policy", C.c_float * 4), ("adam_policy_dev", C.c_void_p),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps_adam", C.c_double),
                ("clamp_abs", C.c_float), ("td_out", C.c_void_p), ("loss_sum", C.c_void_p), ("workspace", C.c_void_p),
                ("images", C.c_void_p)]


class NdqnParams(C.Structure):
    _c_name_ = "gymrl_ndqn_params"   # fc1, fc2, value_stream, advantage_stream
    _fields_ = [("w_mu", C.c_void_p * 4), ("w_sigma", C.c_void_p * 4), ("b_mu", C.c_void_p * 4), ("b_sigma", C.c_void_p * 4)]


class NdqnCombineArgs(C.Structure):
    _c_name_ = "gymrl_ndqn_combine_args"
    _fields_ = [("D", C.c_int), ("A", C.c_int), ("H", C.c_int), ("policy", NdqnParams), ("seed", C.c_uint64 * 4),
                ("counter", C.c_uint64 * 3), ("counter_dev", C.c_void_p), ("raw", C.c_void_p * 3), ("workspace", C.c_void_p)]


class NdqnActArgs(C.Structure):
    _c_name_ = "gymrl_ndqn_act_args"
    _fields_ = [("N", C.c_int), ("D", C.c_int), ("A", C.c_int), ("H", C.c_int), ("env_kind", C.c_int),
                ("env_state", C.c_void_p), ("env_seed", C.c_uint64), ("env_id0", C.c_int64),
                ("obs", C.c_void_p), ("obs_out", C.c_void_p),
                ("r_state", C.c_void_p), ("r_action", C.c_void_p), ("r_reward", C.c_void_p), ("r_next", C.c_void_p),
                ("r_flag", C.c_void_p), ("cap", C.c_int64), ("cursor", C.c_int64), ("cursor_dev", C.c_void_p),
                ("action_out", C.c_void_p), ("rew_out", C.c_void_p), ("done_out", C.c_void_p), ("ep_ret_out", C.c_void_p),
                ("ep_stats", C.c_void_p), ("workspace", C.c_void_p)]


class NdqnUpdateArgs(C.Structure):
    _c_name_ = "gymrl_ndqn_update_args"
    _fields_ = [("B", C.c_int), ("D", C.c_int), ("A", C.c_int), ("H", C.c_int), ("gamma", C.c_float),
                ("r_state", C.c_void_p), ("r_action", C.c_void_p), ("r_reward", C.c_void_p), ("r_next", C.c_void_p),
                ("r_flag", C.c_void_p), ("cap", C.c_int64),
                ("idx", C.c_void_p), ("idx_seed", C.c_uint64), ("idx_counter", C.c_uint64), ("idx_size", C.c_int64),
                ("idx_dev", C.c_void_p),
                ("policy", NdqnParams), ("target", NdqnParams),
                ("policy_p", C.c_void_p), ("policy_m", C.c_void_p), ("policy_v", C.c_void_p),
                ("adam_policy", C.c_float * 4), ("adam_policy_dev", C.c_void_p),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps_adam", C.c_double),
                ("loss_sum", C.c_void_p), ("workspace", C.c_void_p)]


class EsNoiseArgs(C.Structure):
    _c_name_ = "gymrl_es_noise_args"
    _fields_ = [("n", C.c_int), ("k0", C.c_int), ("K", C.c_int), ("seed", C.c_uint64), ("generation", C.c_uint64), ("out", C.c_void_p)]


class EsPerturbArgs(C.Structure):
    _c_name_ = "gymrl_es_perturb_args"
    _fields_ = [("n", C.c_int), ("P", C.c_int), ("stride", C.c_int64), ("sigma", C.c_float), ("seed", C.c_uint64),
                ("generation", C.c_uint64), ("theta", C.c_void_p), ("params", C.c_void_p)]


class EsShapeGradArgs(C.Structure):
    _c_name_ = "gymrl_es_shape_grad_args"
    _fields_ = [("n", C.c_int), ("P", C.c_int), ("E", C.c_int), ("sigma", C.c_float), ("seed", C.c_uint64),
                ("generation", C.c_uint64), ("returns", C.c_void_p), ("grad", C.c_void_p), ("weights", C.c_void_p)]


class TabularTrainArgs(C.Structure):
    _c_name_ = "gymrl_tabular_train_args"
    _fields_ = [("rule", C.c_int), ("env_kind", C.c_int), ("is_slippery", C.c_int), ("shaped", C.c_int), ("Q", C.c_void_p),
                ("state", C.c_void_p), ("n_runs", C.c_int), ("restart", C.c_int), ("seed", C.c_uint64), ("run_id0", C.c_int64),
                ("eps_table", C.c_void_p), ("max_episodes", C.c_int), ("max_steps", C.c_int), ("max_iters", C.c_int),
                ("lr", C.c_double), ("gamma", C.c_double), ("episode_rewards", C.c_void_p), ("episode_lengths", C.c_void_p),
                ("k_out", C.c_void_p), ("episodes_out", C.c_void_p), ("Q2", C.c_void_p), ("eps_len", C.c_int64)]


class SnesPerturbArgs(C.Structure):
    _c_name_ = "gymrl_snes_perturb_args"
    _fields_ = [("n", C.c_int), ("P", C.c_int), ("stride", C.c_int64), ("seed", C.c_uint64), ("generation", C.c_uint64),
                ("mu", C.c_void_p), ("sigma", C.c_void_p), ("params", C.c_void_p)]


class SnesTellArgs(C.Structure):
    _c_name_ = "gymrl_snes_tell_args"
    _fields_ = [("n", C.c_int), ("P", C.c_int), ("E", C.c_int), ("eta_mu", C.c_float), ("eta_sigma", C.c_float),
                ("sigma_min", C.c_float), ("sigma_max", C.c_float), ("seed", C.c_uint64), ("generation", C.c_uint64),
                ("returns", C.c_void_p), ("returns64", C.c_void_p), ("mu", C.c_void_p), ("sigma", C.c_void_p),
                ("weights", C.c_void_p)]


class MountainCarNetEvalArgs(C.Structure):
    _c_name_ = "gymrl_mountaincar_net_eval_args"
    _fields_ = [("P", C.c_int), ("E", C.c_int), ("cap", C.c_int), ("net", C.c_int), ("n_hidden", C.c_int), ("H", C.c_int),
                ("w", C.c_void_p * 2), ("b", C.c_void_p * 2), ("head_w", C.c_void_p), ("head_b", C.c_void_p),
                ("value_w", C.c_void_p), ("value_b", C.c_void_p), ("policy_stride", C.c_int64), ("images", C.c_void_p),
                ("seed", C.c_uint64), ("stream_id0", C.c_int64), ("start", C.c_void_p), ("returns", C.c_void_p),
                ("lengths", C.c_void_p), ("terminated", C.c_void_p), ("final_obs", C.c_void_p)]


class AcrobotNetEvalArgs(C.Structure):
    _c_name_ = "gymrl_acrobot_net_eval_args"
    _fields_ = list(MountainCarNetEvalArgs._fields_)          # the same block: only the widths behind `start` / `final_obs` differ


class ClassicEvalArgs(C.Structure):
    _c_name_ = "gymrl_classic_eval_args"
    _fields_ = [("P", C.c_int), ("E", C.c_int), ("cap", C.c_int), ("env_kind", C.c_int), ("head", C.c_int), ("D", C.c_int),
                ("A", C.c_int), ("H", C.c_int), ("bound", C.c_float), ("w", C.c_void_p * 3), ("b", C.c_void_p * 3),
                ("policy_stride", C.c_int64), ("images", C.c_void_p), ("seed", C.c_uint64), ("stream_id0", C.c_int64),
                ("start", C.c_void_p), ("returns", C.c_void_p), ("lengths", C.c_void_p), ("terminated", C.c_void_p),
                ("final_obs", C.c_void_p)]


class ClassicDuelEvalArgs(C.Structure):
    _c_name_ = "gymrl_classic_duel_eval_args"
    _fields_ = [("P", C.c_int), ("E", C.c_int), ("cap", C.c_int), ("env_kind", C.c_int), ("n_hidden", C.c_int), ("D", C.c_int),
                ("A", C.c_int), ("H", C.c_int), ("w", C.c_void_p * 2), ("b", C.c_void_p * 2), ("value_w", C.c_void_p),
                ("value_b", C.c_void_p), ("adv_w", C.c_void_p), ("adv_b", C.c_void_p), ("policy_stride", C.c_int64),
                ("images", C.c_void_p), ("seed", C.c_uint64), ("stream_id0", C.c_int64), ("start", C.c_void_p),
                ("returns", C.c_void_p), ("lengths", C.c_void_p), ("terminated", C.c_void_p), ("final_obs", C.c_void_p)]


class MountainCarEvalArgs(C.Structure):
    _c_name_ = "gymrl_mountaincar_eval_args"
    _fields_ = [("P", C.c_int), ("E", C.c_int), ("cap", C.c_int), ("seed", C.c_uint64), ("stream_id0", C.c_int64),
                ("coefs", C.c_void_p), ("start", C.c_void_p), ("returns", C.c_void_p), ("lengths", C.c_void_p),
                ("reached", C.c_void_p), ("final_state", C.c_void_p)]


class WeightImage(C.Structure):
    _c_name_ = "gymrl_weight_image"
    _fields_ = [("W", C.c_void_p), ("H", C.c_int), ("img_fwd", C.c_void_p), ("img_bwd", C.c_void_p)]


class PPOFullCfg(C.Structure):
    _c_name_ = "gymrl_ppo_full_cfg"
    _fields_ = [("clip_eps_min", C.c_float), ("clip_eps_max", C.c_float), ("dual_clip", C.c_float),
                ("erc_beta_low", C.c_float), ("erc_beta_high", C.c_float), ("entropy_coef", C.c_float),
                ("entropy_coef_dev", C.c_void_p)]


class MlprnnParams(C.Structure):
    _c_name_ = "gymrl_mlprnn_params"
    _fields_ = ([("pscn_w", C.c_void_p * 4), ("pscn_b", C.c_void_p * 4), ("pscn_a", C.c_void_p * 4)] +
                [(n, C.c_void_p) for n in ("lin_w", "lin_b", "w_ih", "b_ih", "w_hh", "b_hh", "actor_w1", "actor_b1", "actor_a",
                                          "actor_w2", "actor_b2", "critic_w1", "critic_b1", "critic_a", "critic_w2",
                                          "critic_b2")])


_vp, _i, _i64, _u64, _f, _d, _sz, _P = (C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_size_t,
                                        C.POINTER)
# Every entry point of include/gymrl.h, in its order: name -> (restype, argtypes).  lib() applies it, so ctypes converts
# plain Python ints and floats and refuses an argument of another type; tests/test_abi.py holds each line to the header.
# A pointer to device memory or a stream is _vp; a HOST array the caller passes as a ctypes array is _P(<scalar>); a
# `const gymrl_x*` is _P(<its mirror above>), or _vp where callers also hand in an untyped NULL (gymrl_mhc_policy_pack,
# gymrl_mhc_policy_forward).
SIGNATURES = {
    "gymrl_abi_version": (_i, []),
    "gymrl_device_ok": (_i, []),
    "gymrl_env_obs_dim": (_i, [_i]),
    "gymrl_env_act_dim": (_i, [_i]),
    "gymrl_env_is_discrete": (_i, [_i]),
    "gymrl_env_max_steps": (_i, [_i]),
    "gymrl_env_state_bytes": (_sz, [_i, _i]),
    "gymrl_env_reset": (_i, [_i, _vp, _i, _u64, _i64, _vp, _vp]),
    "gymrl_env_step": (_i, [_i, _vp, _i, _u64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_env_abandon": (_i, [_i, _vp, _i, _u64, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_env_refill": (_i, [_i, _vp, _i, _u64, _i64, _vp]),
    "gymrl_categorical_sample": (_i, [_vp, _vp, _vp, _u64, _u64, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _P(GaeOnline), _vp]),
    "gymrl_gaussian_sample": (_i, [_vp, _vp, _vp, _vp, _u64, _u64, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _P(GaeOnline), _vp]),
    "gymrl_gae_online_flush": (_i, [_P(GaeOnline), _vp, _i, _vp]),
    "gymrl_gae_chunk": (_i, []),
    "gymrl_gae_workspace_bytes": (_sz, [_i, _i]),
    "gymrl_gae": (_i, [_vp, _vp, _vp, _vp, _i, _i, _d, _d, _vp, _vp, _vp, _i, _vp, _vp]),
    "gymrl_gae_dw": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _d, _d, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_gae_decoupled_workspace_bytes": (_sz, [_i, _i]),
    "gymrl_gae_decoupled": (_i, [_vp, _vp, _vp, _vp, _i, _i, _d, _d, _d, _vp, _vp, _i, _vp, _vp]),
    "gymrl_reduce_workspace_bytes": (_sz, []),
    "gymrl_moments": (_i, [_vp, _i64, _vp, _vp, _vp]),
    "gymrl_normalize": (_i, [_vp, _i64, _vp, _i, _d, _vp]),
    "gymrl_ppo_loss_fwd_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _P(PPOCfg), _vp, _vp, _vp, _vp, _vp]),
    "gymrl_ppo_gauss_loss_workspace_bytes": (_sz, [_i, _i]),
    "gymrl_ppo_gauss_loss_fwd_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _P(PPOCfg), _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "gymrl_loss_blocks": (_i, [_i]),
    "gymrl_reduce_rows": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "gymrl_ppo_full_loss_fwd_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _P(PPOFullCfg), _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_ppo_rnn_loss_fwd_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _P(PPOFullCfg), _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_gru_cell_fwd": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "gymrl_gru_cell_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "gymrl_rnd_reward": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "gymrl_gru_seq_fwd": (_i, [_vp, _vp, _vp, _vp, _P(C.c_int32), _i, _i, _i, _vp, _vp, _vp]),
    "gymrl_gru_seq_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(C.c_int32), _i, _i, _i, _vp, _vp, _vp, _vp]),
    "gymrl_lstm_cell_fwd": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "gymrl_lstm_cell_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "gymrl_lstm_seq_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _P(C.c_int32), _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_lstm_seq_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(C.c_int32), _i, _i, _i, _vp, _vp, _vp, _vp]),
    "gymrl_episode_gae": (_i, [_vp, _vp, _vp, _vp, _vp, _P(_i64), _i, _d, _d, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_ppg_policy_loss_fwd_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _P(_i64), _i, _i, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_ppg_aux_loss_fwd_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _P(_i64), _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_mlprnn_params_bytes": (_sz, []),
    "gymrl_mlprnn_act": (_i, [_vp, _vp, _P(MlprnnParams), _i, _i, _i, _vp, _vp, _u64, _u64, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_permutation": (_i, [_u64, _u64, _i64, _vp, _vp]),
    "gymrl_pack_rollout": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _vp, _vp]),
    "gymrl_gather_minibatch": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_gather_rows": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "gymrl_sqnorm": (_i, [_vp, _i64, _f, _vp, _vp, _vp]),
    "gymrl_adam_step": (_i, [_vp, _vp, _vp, _vp, _i64, _d, _vp, _d, _d, _d, _i64, _vp, _f, _f, _vp, _f, _i, _vp, _d, _vp]),
    "gymrl_clip_adam_step": (_i, [_vp, _vp, _vp, _vp, _i64, _d, _vp, _d, _d, _d, _i64, _vp, _f, _f, _vp, _f, _i, _vp, _d, _vp, _vp]),
    "gymrl_adam_bias": (_i, [_d, _d, _d, _i64, _P(_f)]),
    "gymrl_store_scalars": (_i, [_vp, _vp, _i, _vp]),
    "gymrl_soft_update": (_i, [_vp, _vp, _i64, _d, _vp]),
    "gymrl_mlp_packed_floats": (_sz, [_i, _i]),
    "gymrl_mlp_pack": (_i, [_vp, _i, _i, _vp, _vp]),
    "gymrl_mlp_forward": (_i, [_vp, _i, _i, _P(MlpDesc), _vp]),
    "gymrl_mlp_pack_stack_args_bytes": (_sz, []),
    "gymrl_mlp_pack_stack": (_i, [_P(MlpPackStackArgs), _vp]),
    "gymrl_rollout_lunar": (_i, [_P(RolloutLunarArgs), _P(MlpDesc), _vp]),
    "gymrl_rollout_cartpole": (_i, [_P(RolloutLunarArgs), _P(MlpDesc), _vp]),
    "gymrl_rollout_classic": (_i, [_i, _P(RolloutLunarArgs), _P(MlpDesc), _vp]),
    "gymrl_rollout_pendulum_args_bytes": (_sz, []),
    "gymrl_rollout_pendulum": (_i, [_P(RolloutPendulumArgs), _P(MlpDesc), _vp]),
    "gymrl_rollout_lunar_mhc": (_i, [_P(RolloutLunarArgs), _P(MhcPolicy), _vp]),
    "gymrl_lunar_eval_args_bytes": (_sz, []),
    "gymrl_lunar_policy_eval": (_i, [_P(LunarEvalArgs), _P(MlpDesc), _vp]),
    "gymrl_lunar_mhc_eval": (_i, [_P(LunarEvalArgs), _P(MhcPolicy), _vp]),
    "gymrl_lunar_mlprnn_eval": (_i, [_P(LunarEvalArgs), _P(MlprnnParams), _vp, _i64, _vp, _vp]),
    "gymrl_lunar_mlprnn_collect": (_i, [_P(LunarCollectArgs), _P(MlprnnParams), _vp]),
    "gymrl_lunar_collect_args_bytes": (_sz, []),
    "gymrl_classic_ppo_eval_args_bytes": (_sz, []),
    "gymrl_classic_ppo_eval": (_i, [_P(ClassicPpoEvalArgs), _P(MlpDesc), _vp]),
    "gymrl_pendulum_ppo_eval_args_bytes": (_sz, []),
    "gymrl_pendulum_ppo_eval": (_i, [_P(PendulumPpoEvalArgs), _P(MlpDesc), _vp]),
    "gymrl_lin_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "gymrl_lin_fwd": (_i, [_P(LinItem), _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "gymrl_lin_bwd_input": (_i, [_P(LinItem), _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "gymrl_lin_bwd_weight": (_i, [_P(LinItem), _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "gymrl_noisy_combine": (_i, [_P(NoisyLayer), _i, _i, _i, _vp, _vp, _vp]),
    "gymrl_noisy_split": (_i, [_P(NoisyLayer), _i, _i, _i, _vp, _vp, _i, _vp]),
    "gymrl_noisy_combine_images": (_i, [_P(NoisyLayer), _i, _i, _i, _vp, _vp, _P(WeightImage), _i, _vp]),
    "gymrl_dueling_bwd": (_i, [_vp, _i, _i, _vp, _vp]),
    "gymrl_mhc_gates": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_mhc_combine": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "gymrl_rmsnorm": (_i, [_vp, _vp, _i, _i, _i, _f, _i, _vp, _vp]),
    "gymrl_rmsnorm_bwd_workspace_bytes": (_sz, [_i]),
    "gymrl_rmsnorm_bwd": (_i, [_vp, _vp, _vp, _i, _i, _f, _i, _vp, _vp, _vp, _vp]),
    "gymrl_rmsnorm_sum_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp]),
    "gymrl_norm_proj_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp]),
    "gymrl_norm_proj_bwd_workspace_bytes": (_sz, [_i, _i]),
    "gymrl_norm_proj_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_sinkhorn": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "gymrl_mhc_gates_bwd_workspace_bytes": (_sz, [_i, _i]),
    "gymrl_mhc_gates_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_mhc_read_fwd": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "gymrl_mhc_read_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp]),
    "gymrl_mhc_combine_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_mhc_sub_forward": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_mhc_sub_backward": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                    _vp]),
    "gymrl_mhc_policy_image_floats": (_sz, [_i]),
    "gymrl_mhc_policy_pack": (_i, [_vp, _vp, _vp]),
    "gymrl_mhc_policy_forward": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "gymrl_mlp_train_workspace_bytes": (_sz, [_i, _i, _i]),
    "gymrl_linear_tanh_smallk": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp]),
    "gymrl_linear_smallk": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp]),
    "gymrl_tanh_inplace": (_i, [_vp, _i64, _vp, _i, _vp]),
    "gymrl_tanh_bwd_colsum": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _vp]),
    "gymrl_linear_smallk_bwd": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_heads_fwd_tanh": (_i, [_vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "gymrl_heads_bwd": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "gymrl_heads_loss_blocks": (_i, [_i64, _i]),
    "gymrl_ppo_update_shape_ok": (_i, [_i, _i, _i]),
    "gymrl_heads_loss_fwd_bwd": (_i, [_vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(PPOCfg), _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp]),
    "gymrl_ppo_gauss_update_shape_ok": (_i, [_i, _i, _i]),
    "gymrl_gauss_heads_loss_workspace_bytes": (_sz, [_i64, _i, _i]),
    "gymrl_gauss_heads_loss_fwd_bwd": (_i, [_vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(PPOCfg), _vp, _vp, _vp,
                                            _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "gymrl_gemm_workspace_bytes": (_sz, []),
    "gymrl_linear_fwd": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _vp, _vp]),
    "gymrl_linear_bwd_input": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp]),
    "gymrl_linear_bwd_input_add": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp]),
    "gymrl_linear_geometry": (_i, [_i, _i64, _i, _i, _P(_i), _P(_i)]),
    "gymrl_linear_bwd_weight_geometry": (_i, [_i64, _i, _P(_i), _P(_i64)]),
    "gymrl_linear_bwd_weight": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp]),
    "gymrl_update_finalize": (_i, [_i64, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_replay_append": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_replay_gather": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_uniform_indices": (_i, [_u64, _u64, _i64, _i, _vp, _vp, _vp]),
    "gymrl_nstep_push": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64,
                              _vp, _vp, _i, _vp]),
    "gymrl_per_workspace_bytes": (_sz, [_i]),
    "gymrl_per_update": (_i, [_vp, _i64, _vp, _i64, _i, _vp, _vp, _d, _i, _vp, _vp, _vp]),
    "gymrl_per_max_leaf": (_i, [_vp, _i64, _vp, _vp, _vp]),
    "gymrl_per_priorities": (_i, [_vp, _i, _d, _d, _d, _vp, _vp]),
    "gymrl_per_update_td": (_i, [_vp, _i64, _vp, _vp, _i, _d, _d, _d, _vp, _vp, _vp, _vp]),
    "gymrl_per_sample": (_i, [_vp, _i64, _vp, _u64, _u64, _i, _i64, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_noisy_noise": (_i, [_vp, _vp, _u64, _u64, _i, _i, _vp, _vp, _vp, _vp]),
    "gymrl_epsilon_greedy": (_i, [_vp, _vp, _u64, _u64, _i64, _i, _i, _f, _vp, _vp]),
    "gymrl_dqn_td_loss": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _d, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_c51_q": (_i, [_vp, _i, _i, _i, _f, _f, _vp, _vp, _vp]),
    "gymrl_c51_loss": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _d, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_qr_q": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "gymrl_qr_loss": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _d, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_sac_sample_fwd": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp]),
    "gymrl_sac_sample_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp]),
    "gymrl_sac_target": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _d, _vp, _vp]),
    "gymrl_sac_critic_loss": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_sac_actor_loss": (_i, [_vp, _vp, _vp, _vp, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_sac_alpha_step": (_i, [_vp, _vp, _vp, _vp, _i, _d, _d, _d, _d, _i64, _vp, _vp, _vp]),
    "gymrl_noisy_action": (_i, [_vp, _vp, _u64, _u64, _i64, _i, _d, _d, _d, _vp, _vp]),
    "gymrl_mse_loss": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "gymrl_neg_mean_loss": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "gymrl_dsac_target": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _d, _vp, _vp]),
    "gymrl_dsac_critic_loss": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_dsac_actor_loss": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "gymrl_dsac_alpha_step": (_i, [_vp, _vp, _vp, _vp, _i, _d, _d, _d, _d, _d, _i64, _vp, _vp, _vp]),
    "gymrl_running_norm": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp]),
    "gymrl_reward_scaling": (_i, [_vp, _vp, _i, _d, _vp, _vp, _vp, _vp]),
    "gymrl_running_norm_masked": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "gymrl_reward_scaling_masked": (_i, [_vp, _vp, _vp, _i, _d, _vp, _vp, _vp, _vp]),
    "gymrl_sac_update_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "gymrl_sac_pack_images": (_i, [_P(SacUpdateArgs), _vp]),
    "gymrl_sac_args_bytes": (_sz, [_i]),
    "gymrl_sac_act_step": (_i, [_P(SacActArgs), _vp]),
    "gymrl_sac_update": (_i, [_P(SacUpdateArgs), _vp]),
    "gymrl_rainbow_update_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "gymrl_rainbow_args_bytes": (_sz, [_i]),
    "gymrl_rainbow_act_step": (_i, [_P(RainbowActArgs), _vp]),
    "gymrl_rainbow_update": (_i, [_P(RainbowUpdateArgs), _i, _vp]),
    "gymrl_td3_update_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "gymrl_td3_pack_images": (_i, [_P(Td3UpdateArgs), _vp]),
    "gymrl_td3_args_bytes": (_sz, [_i]),
    "gymrl_td3_act_step": (_i, [_P(Td3ActArgs), _vp]),
    "gymrl_td3_update": (_i, [_P(Td3UpdateArgs), _vp]),
    "gymrl_dsac_update_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "gymrl_dsac_pack_images": (_i, [_P(DsacUpdateArgs), _vp]),
    "gymrl_dsac_args_bytes": (_sz, [_i]),
    "gymrl_dsac_act_step": (_i, [_P(DsacActArgs), _vp]),
    "gymrl_dsac_act_step_classic": (_i, [_P(DsacActArgs), _vp]),
    "gymrl_dsac_update": (_i, [_P(DsacUpdateArgs), _vp]),
    "gymrl_softmax_rows_fwd": (_i, [_vp, _i, _i, _vp, _vp]),
    "gymrl_softmax_rows_bwd": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "gymrl_es_pair_chunk": (_i, []),
    "gymrl_es_noise_args_bytes": (_sz, []),
    "gymrl_es_perturb_args_bytes": (_sz, []),
    "gymrl_es_shape_grad_args_bytes": (_sz, []),
    "gymrl_es_noise": (_i, [_P(EsNoiseArgs), _vp]),
    "gymrl_es_perturb": (_i, [_P(EsPerturbArgs), _vp]),
    "gymrl_es_shape_grad": (_i, [_P(EsShapeGradArgs), _vp]),
    "gymrl_qlearn_state_bytes": (_sz, [_i]),
    "gymrl_qlearn_train": (_i, [_i, _i, _i, _vp, _vp, _i, _i, _u64, _i64, _vp, _i, _i, _i, _d, _d, _vp, _vp, _vp, _vp, _vp]),
    "gymrl_qlearn_eval": (_i, [_i, _i, _vp, _i, _i, _u64, _i64, _i, _vp, _vp, _vp, _vp]),
    "gymrl_tabular_state_bytes": (_sz, [_i, _i]),
    "gymrl_tabular_args_bytes": (_sz, []),
    "gymrl_tabular_train": (_i, [_P(TabularTrainArgs), _vp]),
    "gymrl_snes_perturb_args_bytes": (_sz, []),
    "gymrl_snes_tell_args_bytes": (_sz, []),
    "gymrl_snes_perturb": (_i, [_P(SnesPerturbArgs), _vp]),
    "gymrl_snes_tell": (_i, [_P(SnesTellArgs), _vp]),
    "gymrl_acrobot_net_eval_args_bytes": (_sz, []),
    "gymrl_acrobot_net_eval": (_i, [_P(AcrobotNetEvalArgs), _vp]),
    "gymrl_dqn_update_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "gymrl_dqn_pack_images": (_i, [_P(DqnUpdateArgs), _vp]),
    "gymrl_dqn_args_bytes": (_sz, [_i]),
    "gymrl_dqn_act_step": (_i, [_P(DqnActArgs), _vp]),
    "gymrl_dqn_act_step_classic": (_i, [_P(DqnActArgs), _vp]),
    "gymrl_dqn_update": (_i, [_P(DqnUpdateArgs), _vp]),
    "gymrl_ddqn_update_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "gymrl_ddqn_pack_images": (_i, [_P(DdqnUpdateArgs), _vp]),
    "gymrl_ddqn_args_bytes": (_sz, [_i]),
    "gymrl_ddqn_update": (_i, [_P(DdqnUpdateArgs), _vp]),
    "gymrl_ddqn_duel_act_step": (_i, [_P(DqnActArgs), _vp]),
    "gymrl_ndqn_args_bytes": (_sz, [_i]),
    "gymrl_ndqn_combine": (_i, [_P(NdqnCombineArgs), _vp]),
    "gymrl_ndqn_act_step": (_i, [_P(NdqnActArgs), _vp]),
    "gymrl_ndqn_update_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "gymrl_ndqn_update": (_i, [_P(NdqnUpdateArgs), _vp]),
    "gymrl_mountaincar_net_eval_args_bytes": (_sz, []),
    "gymrl_mountaincar_net_eval": (_i, [_P(MountainCarNetEvalArgs), _vp]),
    "gymrl_classic_eval_args_bytes": (_sz, []),
    "gymrl_classic_policy_eval": (_i, [_P(ClassicEvalArgs), _vp]),
    "gymrl_classic_duel_eval_args_bytes": (_sz, []),
    "gymrl_classic_duel_eval": (_i, [_P(ClassicDuelEvalArgs), _vp]),
    "gymrl_mountaincar_rule_eval": (_i, [_P(MountainCarEvalArgs), _vp]),
}
SYMBOLS = list(SIGNATURES)


def lib():
    """The loaded C-ABI library, every function typed by SIGNATURES.  Raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C {CSRC}` (or __graft_entry__.build()). "
                "gymrl_amd has no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        got = L.gymrl_abi_version()
        if got != ABI_VERSION:       # a stale .so would take mis-aligned arguments silently
            raise RuntimeError(f"{LIB_PATH} reports ABI version {got}, this package needs {ABI_VERSION}: rebuild it "
                               f"with `make -C {CSRC}`")
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def lib_sha256():
    """sha256 of the library file that lib() loads — the identity of the binary a measurement was taken on
    (profiles/*_pmc_summary.json carry it; bench.py refuses a counter summary taken on another binary)."""
    import hashlib
    h = hashlib.sha256()
    with open(LIB_PATH, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with code {rc}" + (" (EINVAL)" if rc == -22 else ""))
