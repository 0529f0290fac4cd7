// eval_acrobot.hip — whole evaluation episodes of Acrobot-v1 under a three-layer MLP or a dueling network, P policies x E episodes
// in ONE launch.
//
// eval_mountaincar.hip for env kind 5: the same six trainers' eval() loops with env_name = "Acrobot-v1" — select_action(
// deterministic=True) -> env.step, 500 times over unless the policy swings the tip over the line.  The kernels are
// eval_kernels_device.hpp's, instantiated for (D, A) = (6, 3) on this entry point's own argument block; the episode loop is
// eval_episode_device.hpp's run_episodes with acrobot_draw / acrobot_advance (env_classic_device.hpp: the stepper's).  One
// workgroup of slab::kThreads threads per 16 episodes of one policy, the float64 (th1, th2, dth1, dth2) in the lanes' registers,
// the uniform exit on one LDS word, at most `cap` <= 500 trips, no atomics, global memory only read inside the loop.
//
// The env step is not a handful of flops here: an RK4 step of the four-variable ODE, fourteen det_sincos and sixteen divisions in
// float64, on 16 lanes of wave 0 while the other fifteen waves wait at the next barrier (what that costs per step).
// A row of three actions is where the two dueling means differ: net 1 is duel_combine, net 2 dueling_row (duel_device.hpp).
#include "eval_kernels_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::slab;

constexpr int kAcro = GYMRL_ENV_ACROBOT, kCap = 500;      // Acrobot-v1's TimeLimit
using Args = gymrl_acrobot_net_eval_args;

template <int HC>
constexpr auto mlp_kernel = classic_eval_kernel<HC, kAcro, Args>;
template <int HC, int NH, int COMBINE>
constexpr auto duel_kernel = duel_eval_kernel<HC, NH, kAcro, COMBINE, Args>;

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

size_t gymrl_acrobot_net_eval_args_bytes(void) { return sizeof(gymrl_acrobot_net_eval_args); }

int gymrl_acrobot_net_eval(const gymrl_acrobot_net_eval_args* args, void* stream) {
  if (!args) return -22;
  const Args& a = *args;
  if (!episode_args_ok(a, kCap)) return -22;
  if (a.net < 0 || a.net > 2) return -22;
  const bool duel = a.net != 0;
  if (duel ? (a.n_hidden != 1 && a.n_hidden != 2) : a.n_hidden != 2) return -22;
  if (!slab_shape_ok(1, 1, EvalDims<kAcro>::D, EvalDims<kAcro>::A, a.H)) return -22;
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
