// eval_mountaincar.hip — whole evaluation episodes of MountainCar-v0 under a three-layer MLP or a dueling network, P policies x E
// episodes in ONE launch.
//
// Replaces the eval() loops of dqn_cartpole.py, ddqn_per_cartpole.py, sac_cartpole.py (three layers), ddqn_per_duel_cartpole.py,
// noisy_dqn_cartpole.py and rainbow_dqn_cartpole.py (dueling) with env_name = "MountainCar-v0": select_action(deterministic=True)
// -> env.step, 200 times over unless the policy already reaches the flag.  The kernels are eval_kernels_device.hpp's — the ones
// eval_classic.hip and eval_duel.hip run on CartPole-v1 — instantiated for env kind 3, (D, A) = (2, 3), on this entry point's own
// argument block; the episode loop is eval_episode_device.hpp's run_episodes with mountaincar_draw / mountaincar_advance
// (env_classic_device.hpp: the stepper's and the rule baseline's).  One workgroup of slab::kThreads threads per 16 episodes of
// one policy, the float64 (position, velocity) in the lanes' registers, the uniform exit on one LDS word, at most `cap` <= 200
// trips, no atomics, global memory only read inside the loop.
//
// Three actions is the first width at which the two dueling means differ: net 1 combines as torch does (duel_combine,
// sum * (1 / 3)), net 2 as gymrl_lin_fwd's GYMRL_ACT_DUELING epilogue does (dueling_row, sum / 3) — duel_device.hpp has both.
#include "eval_kernels_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::slab;

constexpr int kCar = GYMRL_ENV_MOUNTAINCAR, kCap = 200;      // MountainCar-v0's TimeLimit
using Args = gymrl_mountaincar_net_eval_args;

template <int HC>
constexpr auto mlp_kernel = classic_eval_kernel<HC, kCar, Args>;
template <int HC, int NH, int COMBINE>
constexpr auto duel_kernel = duel_eval_kernel<HC, NH, kCar, COMBINE, Args>;

using Kernel = void (*)(const Args);

// the instance of a (net, n_hidden, H): the ones built for the reference's hidden width where H is 256
template <int HC>
Kernel pick(int net, bool two) {
  if (net == 0) return mlp_kernel<HC>;
  if (net == kCombineMean) return two ? duel_kernel<HC, 2, kCombineMean> : duel_kernel<HC, 1, kCombineMean>;
  return two ? duel_kernel<HC, 2, kCombineRow> : duel_kernel<HC, 1, kCombineRow>;
}

}  // namespace

extern "C" {

size_t gymrl_mountaincar_net_eval_args_bytes(void) { return sizeof(gymrl_mountaincar_net_eval_args); }

int gymrl_mountaincar_net_eval(const gymrl_mountaincar_net_eval_args* args, void* stream) {
  if (!args) return -22;
  const Args& a = *args;
  if (!episode_args_ok(a, kCap)) return -22;
  if (a.net < 0 || a.net > 2) return -22;
  const bool duel = a.net != 0;
  if (duel ? (a.n_hidden != 1 && a.n_hidden != 2) : a.n_hidden != 2) return -22;
  if (!slab_shape_ok(1, 1, EvalDims<kCar>::D, EvalDims<kCar>::A, a.H)) return -22;
  const bool two = a.n_hidden == 2;
  if (!all_set({a.w[0], a.b[0], a.head_w, a.head_b})) return -22;
  if (duel ? !all_set({a.value_w, a.value_b}) : (a.value_w || a.value_b)) return -22;       // three layers have no value head
  if (two ? !all_set({a.w[1], a.b[1]}) : (a.w[1] || a.b[1] || a.images)) return -22;        // one hidden layer: no fc2, so no image of it
  if (a.images && (a.H & 15) != 0) return -22;
  for (const float* w : {a.w[0], a.w[1], a.head_w, a.value_w})
    if (!aligned(w, 16)) return -22;
  for (const float* b : {a.b[0], a.b[1], a.head_b, a.value_b})
    if (!aligned(b, 4)) return -22;
  static bool lds_set = false;
  if (const int rc = set_max_lds_once(lds_set, {(const void*)pick<0>(0, true), (const void*)pick<256>(0, true),
                                                (const void*)pick<0>(1, false), (const void*)pick<256>(1, false),
                                                (const void*)pick<0>(1, true), (const void*)pick<256>(1, true),
                                                (const void*)pick<0>(2, false), (const void*)pick<256>(2, false),
                                                (const void*)pick<0>(2, true), (const void*)pick<256>(2, true)},
                                      (int)lds_bytes(256, 2)))
    return rc;
  const dim3 grid((unsigned)(a.P * ((a.E + 15) / 16))), block(kThreads);
  const size_t smem = lds_bytes(a.H, a.n_hidden);
  const Kernel k = a.H == 256 ? pick<256>(a.net, two) : pick<0>(a.net, two);
  hipLaunchKernelGGL(k, grid, block, smem, (hipStream_t)stream, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
