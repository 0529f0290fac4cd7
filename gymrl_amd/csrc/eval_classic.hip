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

using Args = gymrl_classic_eval_args;
using Kernel = void (*)(const Args);

// KIND: GYMRL_ENV_CARTPOLE (head 0) or GYMRL_ENV_PENDULUM (head 1); wide: the instance built for hidden width 256 (else: a.H).
// One step's policy forward and its action: eval_kernels_device.hpp's classic_eval_kernel, on this entry point's argument block.
template <int KIND>
Kernel kernel(bool wide) { return wide ? classic_eval_kernel<256, KIND, Args> : classic_eval_kernel<0, KIND, Args>; }
Kernel pick(bool wide, int pendulum) { return pendulum ? kernel<GYMRL_ENV_PENDULUM>(wide) : kernel<GYMRL_ENV_CARTPOLE>(wide); }

// the block's cap, head and widths are the env's
template <int KIND>
bool shape_ok(const Args& a) {
  using Env = EpisodeEnv<KIND>;
  constexpr int head = std::is_same<typename Env::Action, int>::value ? kHeadArgmax : kHeadTanh;
  return episode_args_ok(a, Env::kMaxSteps) && a.head == head && a.D == Env::kObs && a.A == Env::kActions;
}

}  // namespace

extern "C" {

size_t gymrl_classic_eval_args_bytes(void) { return sizeof(gymrl_classic_eval_args); }

int gymrl_classic_policy_eval(const gymrl_classic_eval_args* args, void* stream) {
  if (!args) return -22;
  const Args& a = *args;
  const bool cart = a.env_kind == GYMRL_ENV_CARTPOLE;
  if (!cart && a.env_kind != GYMRL_ENV_PENDULUM) return -22;
  if (!(cart ? shape_ok<GYMRL_ENV_CARTPOLE>(a) : shape_ok<GYMRL_ENV_PENDULUM>(a))) return -22;
  if (!slab_shape_ok(1, 1, a.D, a.A, a.H)) return -22;
  if (!layers_ok({{a.w[0], a.b[0], true}, {a.w[1], a.b[1], true}, {a.w[2], a.b[2], true}})) return -22;
  static bool lds_set = false;
  return launch_episodes<2>(a, stream, lds_set, cart ? 0 : 1, 2, pick);
}

}  // extern "C"
