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

// NH: hidden layers of the trunk (1 | 2); HC: the hidden width the instance is built for (0: a.H).  One step's policy forward and
// its action: eval_kernels_device.hpp's duel_eval_kernel on this entry point's argument block, CartPole-v1, duel_combine.
template <int HC, int NH>
constexpr auto kernel = duel_eval_kernel<HC, NH, GYMRL_ENV_CARTPOLE, kCombineMean, gymrl_classic_duel_eval_args>;

}  // namespace

extern "C" {

size_t gymrl_classic_duel_eval_args_bytes(void) { return sizeof(gymrl_classic_duel_eval_args); }

int gymrl_classic_duel_eval(const gymrl_classic_duel_eval_args* args, void* stream) {
  if (!args) return -22;
  const gymrl_classic_duel_eval_args& a = *args;
  if (a.env_kind != GYMRL_ENV_CARTPOLE || a.D != 4 || a.A != 2) return -22;       // duel_combine's order is pinned for two actions
  if (!episode_args_ok(a, 500)) return -22;
  if (a.n_hidden != 1 && a.n_hidden != 2) return -22;
  if (!slab_shape_ok(1, 1, a.D, a.A, a.H)) return -22;
  const bool two = a.n_hidden == 2;
  if (!all_set({a.w[0], a.b[0], a.value_w, a.value_b, a.adv_w, a.adv_b})) return -22;
  if (two ? !all_set({a.w[1], a.b[1]}) : (a.w[1] || a.b[1] || a.images)) return -22;       // one hidden layer: no fc2, so no image of it
  if (a.images && (a.H & 15) != 0) return -22;
  for (const float* w : {a.w[0], a.w[1], a.value_w, a.adv_w})
    if (!aligned(w, 16)) return -22;
  for (const float* b : {a.b[0], a.b[1], a.value_b, a.adv_b})
    if (!aligned(b, 4)) return -22;
  static bool lds_set = false;
  if (const int rc = set_max_lds_once(lds_set, {(const void*)kernel<0, 1>, (const void*)kernel<256, 1>,
                                                (const void*)kernel<0, 2>, (const void*)kernel<256, 2>},
                                      (int)lds_bytes(256, 2)))
    return rc;
  const dim3 grid((unsigned)(a.P * ((a.E + 15) / 16))), block(kThreads);
  const size_t smem = lds_bytes(a.H, a.n_hidden);
  hipStream_t st = (hipStream_t)stream;
  const bool wide = a.H == 256;           // the instances built for the reference's hidden width
  if (two) hipLaunchKernelGGL((wide ? kernel<256, 2> : kernel<0, 2>), grid, block, smem, st, a);
  else hipLaunchKernelGGL((wide ? kernel<256, 1> : kernel<0, 1>), grid, block, smem, st, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
