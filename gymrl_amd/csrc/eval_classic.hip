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
#include "policy_device.hpp"
#include "slab_step_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::slab;

constexpr int kHeadArgmax = 0, kHeadTanh = 1;

// KIND: GYMRL_ENV_CARTPOLE (head 0, D = 4, A = 2) or GYMRL_ENV_PENDULUM (head 1, D = 3, A = 1); HC: the hidden width the instance is built for (0: a.H)
template <int HC, int KIND>
__global__ __launch_bounds__(kThreads) void classic_eval_kernel(const gymrl_classic_eval_args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ int running;                 // the loop's exit word: written by wave 0, read by everybody behind the barrier
  const Lds L;
  constexpr bool cart = KIND == GYMRL_ENV_CARTPOLE;
  constexpr int D = cart ? 4 : 3, A = cart ? 2 : 1, NS = cart ? 4 : 2;
  const int H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int X0 = L.big, X1 = X0 + 16 * ld;
  const int groups = (a.E + 15) / 16;
  const int p = (int)blockIdx.x / groups, e0 = ((int)blockIdx.x - p * groups) * 16, nrows = min(16, a.E - e0);
  const int t = threadIdx.x;
  const size_t shift = (size_t)p * (size_t)a.policy_stride;
  const float *w0 = a.w[0] + shift, *w1 = a.w[1] + shift, *w2 = a.w[2] + shift;
  const float *b0 = a.b[0] + shift, *b1 = a.b[1] + shift, *b2 = a.b[2] + shift;
  const float* img = (a.images && (H & 15) == 0) ? a.images : nullptr;
  const int64_t i = (int64_t)p * a.E + e0 + t;       // this lane's episode (t < nrows)
  // ---- one lane per episode: the env state, the return and the length live in registers ----
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  double ret = 0.0;
  int len = 0;
  bool terminated = false, active = t < nrows;
  if (t < 16)
    for (int k = 0; k < kMaxD; ++k) lds[L.S + t * kMaxD + k] = 0.0f;     // rows beyond the episodes and columns beyond D stay zero
  if (active) {
    if (a.start) {
#pragma unroll
      for (int k = 0; k < NS; ++k) s[k] = a.start[i * NS + k];
    } else if constexpr (cart) {
      cartpole_draw(a.seed, (uint64_t)(a.stream_id0 + e0 + t), 0u, s);
    } else {
      pendulum_draw(a.seed, (uint64_t)(a.stream_id0 + e0 + t), 0u, s[0], s[1]);
    }
  }
  const int R = GYMRL_ACT_RELU, kD = kMaxD, kA = kMaxA;
  for (int it = 0; it < a.cap; ++it) {
    if (t < 64) {
      if (active) {
        float* o = lds + L.S + t * kMaxD;
        if constexpr (cart) {
          o[0] = (float)s[0]; o[1] = (float)s[1]; o[2] = (float)s[2]; o[3] = (float)s[3];
        } else {
          float ob[3];
          pendulum_obs(s[0], s[1], ob);
          o[0] = ob[0]; o[1] = ob[1]; o[2] = ob[2];
        }
      }
      const bool any = __ballot(active) != 0ull;
      if (t == 0) running = any ? 1 : 0;
    }
    __syncthreads();
    if (!running) break;                  // one word, the same for every thread of the workgroup
    // (the pointers pass through an empty asm: the stages' per-lane operand addresses are formed again in every iteration — hoisted
    // out of the loop they were 47 spilled registers, reloaded from scratch memory step by step)
    asm volatile("" : "+s"(w0), "+s"(w1), "+s"(w2), "+s"(b0), "+s"(b1), "+s"(b2), "+s"(img));
    fwd_one(lds, {fwd_item(L.S, kD, -1, 0, D, D, H, w0, b0, X0, ld, nullptr, 0, R)}, 0, nrows);
    fwd_one(lds, {fwd_item(X0, ld, -1, 0, H, H, H, w1, b1, X1, ld, nullptr, 0, R, 0.0f, 0.0f, img)}, 0, nrows);
    fwd_one(lds, {fwd_item(X1, ld, -1, 0, H, H, A, w2, b2, L.Mean, kA, nullptr, 0, cart ? GYMRL_ACT_NONE : GYMRL_ACT_TANH)}, 0, nrows);
    if (active) {
      if constexpr (cart) {
        // the greedy branch of epsilon_greedy_pick (u0 = 1 is never below epsilon = 0): the first maximum, no draw
        const float never[2] = {1.0f, 0.0f};
        const int act = epsilon_greedy_pick(lds + L.Mean + t * kMaxA, A, never, 0ull, 0ull, 0ull, 0.0f);
        terminated = cartpole_advance(s[0], s[1], s[2], s[3], act);
        ret = ret + 1.0;
      } else {
        const float mu = lds[L.Mean + t * kMaxA] * a.bound;
        ret = ret + (-pendulum_advance(s[0], s[1], mu));
      }
      len += 1;
      active = !terminated && len < a.cap;
    }
    // (the next iteration's stores to L.S and `running` follow fwd_one's closing barrier; their last readers sit in front of it)
  }
  if (t < nrows) {
    a.returns[i] = (float)ret; a.lengths[i] = len; a.terminated[i] = terminated;
    if (a.final_obs) {
      float* o = a.final_obs + i * D;
      if constexpr (cart) {
        o[0] = (float)s[0]; o[1] = (float)s[1]; o[2] = (float)s[2]; o[3] = (float)s[3];
      } else {
        float ob[3];
        pendulum_obs(s[0], s[1], ob);
        o[0] = ob[0]; o[1] = ob[1]; o[2] = ob[2];
      }
    }
  }
}

inline bool aligned(const void* p, size_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) == 0; }

}  // namespace

extern "C" {

size_t gymrl_classic_eval_args_bytes(void) { return sizeof(gymrl_classic_eval_args); }

int gymrl_classic_policy_eval(const gymrl_classic_eval_args* args, void* stream) {
  if (!args) return -22;
  const gymrl_classic_eval_args& a = *args;
  const bool cart = a.env_kind == GYMRL_ENV_CARTPOLE;
  if (!cart && a.env_kind != GYMRL_ENV_PENDULUM) return -22;
  if (a.P < 1 || a.E < 1 || a.cap < 1 || a.cap > (cart ? 500 : 200) || a.stream_id0 < 0) return -22;
  if (cart ? (a.head != kHeadArgmax || a.D != 4 || a.A != 2) : (a.head != kHeadTanh || a.D != 3 || a.A != 1)) return -22;
  if (!slab_shape_ok(1, 1, a.D, a.A, a.H)) return -22;
  if ((int64_t)a.P * a.E > 0x7fffffffLL) return -22;
  if (a.policy_stride < 0 || (a.policy_stride & 3) != 0 || (a.policy_stride == 0 && a.P != 1)) return -22;
  if (a.images && a.P != 1) return -22;
  if (!all_set({a.w[0], a.w[1], a.w[2], a.b[0], a.b[1], a.b[2], a.returns, a.lengths, a.terminated})) return -22;
  for (int k = 0; k < 3; ++k)
    if (!aligned(a.w[k], 16) || !aligned(a.b[k], 4)) return -22;
  if (!aligned(a.images, 16) || !aligned(a.start, 8) || !aligned(a.returns, 4) || !aligned(a.lengths, 4) || !aligned(a.final_obs, 4)) return -22;
  static bool lds_set = false;
  if (const int rc = set_max_lds_once(lds_set, {(const void*)classic_eval_kernel<0, GYMRL_ENV_CARTPOLE>, (const void*)classic_eval_kernel<256, GYMRL_ENV_CARTPOLE>,
                                                (const void*)classic_eval_kernel<0, GYMRL_ENV_PENDULUM>, (const void*)classic_eval_kernel<256, GYMRL_ENV_PENDULUM>},
                                      (int)lds_bytes(256, 2)))
    return rc;
  const dim3 grid((unsigned)(a.P * ((a.E + 15) / 16))), block(kThreads);
  const size_t smem = lds_bytes(a.H, 2);
  hipStream_t st = (hipStream_t)stream;
  const bool wide = a.H == 256;           // the instances built for the reference's hidden width
  if (cart) hipLaunchKernelGGL((wide ? classic_eval_kernel<256, GYMRL_ENV_CARTPOLE> : classic_eval_kernel<0, GYMRL_ENV_CARTPOLE>), grid, block, smem, st, a);
  else hipLaunchKernelGGL((wide ? classic_eval_kernel<256, GYMRL_ENV_PENDULUM> : classic_eval_kernel<0, GYMRL_ENV_PENDULUM>), grid, block, smem, st, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
