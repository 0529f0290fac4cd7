// eval_net.hip — whole evaluation episodes of MountainCar-v0 and Acrobot-v1 under a three-layer MLP or a dueling network,
// P policies x E episodes in ONE launch: two entry points on one set of argument fields, one launcher.
//
// Replaces the eval() loops of dqn_cartpole.py, ddqn_per_cartpole.py, sac_cartpole.py (three layers), ddqn_per_duel_cartpole.py,
// noisy_dqn_cartpole.py and rainbow_dqn_cartpole.py (dueling) with env_name = "MountainCar-v0" | "Acrobot-v1":
// select_action(deterministic=True) -> env.step, a TimeLimit of times over unless the policy already reaches the flag / swings the
// tip over the line.  The kernels are eval_kernels_device.hpp's — the ones eval_classic.hip and eval_duel.hip run on CartPole-v1 —
// instantiated per env kind on the entry point's own argument block; the episode loop is eval_episode_device.hpp's run_episodes on
// EpisodeEnv<KIND> (env_classic_device.hpp: the widths, the TimeLimit, the stepper's draw and advance).  One workgroup of
// slab::kThreads threads per 16 episodes of one policy, the float64 state in the lanes' registers, the uniform exit on one LDS
// word, at most `cap` <= TimeLimit trips, no atomics, global memory only read inside the loop.
//
// Acrobot-v1's env step is not a handful of flops: an RK4 step of the four-variable ODE, fourteen det_sincos and sixteen divisions
// in float64, on 16 lanes of wave 0 while the other fifteen waves wait at the next barrier (what that costs per step).
//
// Three actions is the first width at which the two dueling means differ: net 1 combines as torch does (duel_combine,
// sum * (1 / 3)), net 2 as gymrl_lin_fwd's GYMRL_ACT_DUELING epilogue does (dueling_row, sum / 3) — duel_device.hpp has both.
#include "eval_kernels_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::slab;

constexpr int kVariants = 5;      // (net, n_hidden): (0, 2), (1, 1), (1, 2), (2, 1), (2, 2)

// the instance of a variant: the ones built for the reference's hidden width where H is 256
template <int HC, int KIND, class Args>
auto pick(int variant) -> void (*)(const Args) {
  switch (variant) {
    case 0: return classic_eval_kernel<HC, KIND, Args>;
    case 1: return duel_eval_kernel<HC, 1, KIND, kCombineMean, Args>;
    case 2: return duel_eval_kernel<HC, 2, KIND, kCombineMean, Args>;
    case 3: return duel_eval_kernel<HC, 1, KIND, kCombineRow, Args>;
    default: return duel_eval_kernel<HC, 2, KIND, kCombineRow, Args>;
  }
}

template <int KIND, class Args>
int net_eval_launch(const Args* args, void* stream) {
  using Env = EpisodeEnv<KIND>;
  if (!args) return -22;
  const Args& a = *args;
  if (!episode_args_ok(a, Env::kMaxSteps)) return -22;
  if (a.net < 0 || a.net > 2) return -22;
  const bool duel = a.net != 0;
  if (duel ? (a.n_hidden != 1 && a.n_hidden != 2) : a.n_hidden != 2) return -22;
  if (!slab_shape_ok(1, 1, Env::kObs, Env::kActions, a.H)) return -22;
  const bool two = a.n_hidden == 2;
  // three layers have no value head; one hidden layer: no fc2, so no image of it
  if (!layers_ok({{a.w[0], a.b[0], true}, {a.w[1], a.b[1], two}, {a.head_w, a.head_b, true}, {a.value_w, a.value_b, duel}})) return -22;
  if (!fc2_image_ok(a.images, two, a.H)) return -22;
  static bool lds_set = false;
  return launch_episodes<kVariants>(a, stream, lds_set, duel ? 2 * a.net - 1 + (two ? 1 : 0) : 0, a.n_hidden,
                                    [](bool wide, int v) { return wide ? pick<256, KIND, Args>(v) : pick<0, KIND, Args>(v); });
}

}  // namespace

extern "C" {

size_t gymrl_mountaincar_net_eval_args_bytes(void) { return sizeof(gymrl_mountaincar_net_eval_args); }

int gymrl_mountaincar_net_eval(const gymrl_mountaincar_net_eval_args* args, void* stream) {
  return net_eval_launch<GYMRL_ENV_MOUNTAINCAR>(args, stream);
}

size_t gymrl_acrobot_net_eval_args_bytes(void) { return sizeof(gymrl_acrobot_net_eval_args); }

int gymrl_acrobot_net_eval(const gymrl_acrobot_net_eval_args* args, void* stream) {
  return net_eval_launch<GYMRL_ENV_ACROBOT>(args, stream);
}

}  // extern "C"
