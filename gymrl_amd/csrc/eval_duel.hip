// eval_duel.hip — whole evaluation episodes of CartPole-v1 under a DUELING network, P policies x E episodes in ONE launch.
//
// Replaces the eval() loops of ddqn_per_duel_cartpole.py, noisy_dqn_cartpole.py and rainbow_dqn_cartpole.py
// (select_action(deterministic=True) -> env.step until the episode is over).  In evaluation mode the three networks are the same
// function: a ReLU trunk of one (DuelingQNetwork) or two (NoisyDuelingQNetwork, DuelingNoisyNetwork) layers, a value head H -> 1
// and an advantage head H -> A, q = v + (a - mean a), the first maximum.  A noisy layer is read at its weight_mu / bias_mu.
//
// The episode loop is eval_episode_device.hpp's run_episodes, the one eval_classic.hip runs: one workgroup of slab::kThreads
// threads per 16 episodes of one policy, the env state in the lanes' registers, the uniform exit on one LDS word.  What is stated
// here is one step's policy forward —
//
//   trunk      fc1 (and fc2, from its forward image where one is given) as fwd_one stages: dqn_act_kernel's / ndqn_act_kernel's calls
//   heads      value (1 column) and advantage (A columns) as ONE two-item stage into L.Cq1 / L.Cq0: ndqn_act_kernel's /
//              ddqn_duel_act_kernel's stage, and the barrier behind it
//
// — and its action: duel_combine on the lane's row, then the first maximum (torch.argmax's rule).  Rainbow's layer path computes
// a stacked [A + 1]-column head and combines with sum / A; a tile's output column does not depend on its neighbours and at A = 2,
// the only width taken here, sum / 2 and sum * 0.5 are the same float, so its two weight_mu tensors pass as separate heads.
#include "eval_kernels_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::slab;

using Args = gymrl_classic_duel_eval_args;
using Env = EpisodeEnv<GYMRL_ENV_CARTPOLE>;
using Kernel = void (*)(const Args);

// NH: hidden layers of the trunk (1 | 2); HC: the hidden width the instance is built for (0: a.H).  One step's policy forward and
// its action: eval_kernels_device.hpp's duel_eval_kernel on this entry point's argument block, CartPole-v1, duel_combine.
template <int HC, int NH>
constexpr auto kernel = duel_eval_kernel<HC, NH, GYMRL_ENV_CARTPOLE, kCombineMean, Args>;
Kernel pick(bool wide, int two) { return two ? (wide ? kernel<256, 2> : kernel<0, 2>) : (wide ? kernel<256, 1> : kernel<0, 1>); }

}  // namespace

extern "C" {

size_t gymrl_classic_duel_eval_args_bytes(void) { return sizeof(gymrl_classic_duel_eval_args); }

int gymrl_classic_duel_eval(const gymrl_classic_duel_eval_args* args, void* stream) {
  if (!args) return -22;
  const Args& a = *args;
  // duel_combine's order is pinned for two actions
  if (a.env_kind != GYMRL_ENV_CARTPOLE || a.D != Env::kObs || a.A != Env::kActions) return -22;
  if (!episode_args_ok(a, Env::kMaxSteps)) return -22;
  if (a.n_hidden != 1 && a.n_hidden != 2) return -22;
  if (!slab_shape_ok(1, 1, a.D, a.A, a.H)) return -22;
  const bool two = a.n_hidden == 2;
  if (!layers_ok({{a.w[0], a.b[0], true}, {a.w[1], a.b[1], two}, {a.value_w, a.value_b, true}, {a.adv_w, a.adv_b, true}})) return -22;
  if (!fc2_image_ok(a.images, two, a.H)) return -22;
  static bool lds_set = false;
  return launch_episodes<2>(a, stream, lds_set, two ? 1 : 0, a.n_hidden, pick);
}

}  // extern "C"
