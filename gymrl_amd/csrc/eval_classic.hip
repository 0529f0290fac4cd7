// eval_classic.hip — whole evaluation episodes of CartPole-v1 / Pendulum-v1 under a three-layer MLP policy, P policies x E
// episodes in ONE launch.
//
// Replaces the eval() loops of dqn_cartpole.py:214-235 and its siblings (ddqn_per_cartpole.py, sac_cartpole.py, td3_pendulum.py,
// ddpg_pendulum.py): select_action without exploration -> env.step until the episode is over.  An episode is a strictly serial
// chain of up to 500 policy forwards; stepped from the host, every link costs three layer launches, the pick, the env step and a
// read-back.  Here ONE workgroup of slab::kThreads threads carries 16 episodes of one policy from their reset to their end:
//
//   per step   lanes 0..15 of wave 0 put the float32 observation of their float64 REGISTER state into L.S
//              all 16 waves run fc1, fc2 (ReLU) and fc3 as the fused acting kernels' fwd_one stages (dqn_step.hip dqn_act_kernel,
//              td3_step.hip td3_act_kernel): the same tiles on the same operands, so the layer path's bits
//              the lanes take the action (the first maximum | tanh * bound) and call cartpole_advance / pendulum_advance
//
// A finished lane idles: its state, return and length are frozen (its slab row keeps its last observation and is computed along,
// unread).  The exit is uniform over the workgroup: wave 0 writes ONE LDS word ("is anybody still running") next to the
// observations, and every thread reads it behind the barrier that publishes them — a barrier every thread reaches in every
// iteration.  No __syncthreads() sits behind a per-lane or per-wave condition, nothing waits for another workgroup, there are no
// atomics, and inside the loop global memory is only READ (the weights, from L2 after the first step).  The loop runs at most
// `cap` <= TimeLimit times.
#include "eval_kernels_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::slab;

// KIND: GYMRL_ENV_CARTPOLE (head 0, D = 4, A = 2) or GYMRL_ENV_PENDULUM (head 1, D = 3, A = 1); HC: the hidden width the instance is built for (0: a.H)
// One step's policy forward and its action: eval_kernels_device.hpp's classic_eval_kernel, on this entry point's argument block.
template <int HC, int KIND>
constexpr auto kernel = classic_eval_kernel<HC, KIND, gymrl_classic_eval_args>;

}  // namespace

extern "C" {

size_t gymrl_classic_eval_args_bytes(void) { return sizeof(gymrl_classic_eval_args); }

int gymrl_classic_policy_eval(const gymrl_classic_eval_args* args, void* stream) {
  if (!args) return -22;
  const gymrl_classic_eval_args& a = *args;
  const bool cart = a.env_kind == GYMRL_ENV_CARTPOLE;
  if (!cart && a.env_kind != GYMRL_ENV_PENDULUM) return -22;
  if (!episode_args_ok(a, cart ? 500 : 200)) return -22;
  if (cart ? (a.head != kHeadArgmax || a.D != 4 || a.A != 2) : (a.head != kHeadTanh || a.D != 3 || a.A != 1)) return -22;
  if (!slab_shape_ok(1, 1, a.D, a.A, a.H)) return -22;
  if (!all_set({a.w[0], a.w[1], a.w[2], a.b[0], a.b[1], a.b[2]})) return -22;
  for (int k = 0; k < 3; ++k)
    if (!aligned(a.w[k], 16) || !aligned(a.b[k], 4)) return -22;
  static bool lds_set = false;
  if (const int rc = set_max_lds_once(lds_set, {(const void*)kernel<0, GYMRL_ENV_CARTPOLE>, (const void*)kernel<256, GYMRL_ENV_CARTPOLE>,
                                                (const void*)kernel<0, GYMRL_ENV_PENDULUM>, (const void*)kernel<256, GYMRL_ENV_PENDULUM>},
                                      (int)lds_bytes(256, 2)))
    return rc;
  const dim3 grid((unsigned)(a.P * ((a.E + 15) / 16))), block(kThreads);
  const size_t smem = lds_bytes(a.H, 2);
  hipStream_t st = (hipStream_t)stream;
  const bool wide = a.H == 256;           // the instances built for the reference's hidden width
  if (cart) hipLaunchKernelGGL((wide ? kernel<256, GYMRL_ENV_CARTPOLE> : kernel<0, GYMRL_ENV_CARTPOLE>), grid, block, smem, st, a);
  else hipLaunchKernelGGL((wide ? kernel<256, GYMRL_ENV_PENDULUM> : kernel<0, GYMRL_ENV_PENDULUM>), grid, block, smem, st, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
