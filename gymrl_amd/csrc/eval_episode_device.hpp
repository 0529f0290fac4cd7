// eval_episode_device.hpp — the episode loop of the one-launch policy evaluation, stated once: eval_classic.hip (a three-layer MLP
// on CartPole-v1 / Pendulum-v1), eval_duel.hip (a dueling network on CartPole-v1), eval_mountaincar.hip and eval_acrobot.hip (either
// network on MountainCar-v0 / Acrobot-v1) instantiate it, through eval_kernels_device.hpp, with their own "policy forward" and "action" steps.
//
// ONE workgroup of slab::kThreads threads carries 16 episodes of one policy from their reset to their end.  Lane t < 16 of wave 0
// owns episode e0 + t: its float64 env state, its float64 return, its length and its flags live in registers.  Per iteration
//
//   wave 0       puts the float32 observation of every running lane's state into its row of the forward's input (the caller says
//                where the 16 rows lie: a pointer and a pitch) and writes ONE LDS word, "is anybody still running", beside them
//   everybody    meets at the barrier that publishes both and leaves on that word — the same for every thread of the workgroup
//   forward()    every thread: the policy's stages over the slab, each closed by a workgroup barrier, the last one included
//   action(t)    the running lanes: the greedy action of row t, then cartpole_advance / pendulum_advance / mountaincar_advance /
//                acrobot_advance in registers
//
// A finished lane idles with its registers frozen (its input row keeps its last observation and is computed along, unread).  No
// __syncthreads() sits behind a per-lane or per-wave condition, nothing waits for another workgroup, there are no atomics, inside
// the loop global memory is only READ, and the trip count is at most a.cap.
#pragma once
#include "policy_device.hpp"
#include "slab_step_device.hpp"

namespace gymrl {
namespace slab {
namespace {

// which 16 episodes of which policy this workgroup carries: the grid is P * ceil(E / 16)
struct EpisodeSlot {
  int p, e0, nrows;
  __device__ explicit EpisodeSlot(int E) {
    const int groups = (E + 15) / 16;
    p = (int)blockIdx.x / groups;
    e0 = ((int)blockIdx.x - p * groups) * 16;
    nrows = min(16, E - e0);
  }
};

// The float32 observation of the float64 state s: the cast (CartPole-v1, MountainCar-v0), (cos, sin, thdot) (Pendulum-v1) or
// the two links' (cos, sin) and the velocities (Acrobot-v1)
template <int KIND>
__device__ __forceinline__ void episode_obs(const double (&s)[4], float* o) {
  if constexpr (KIND == GYMRL_ENV_CARTPOLE) {
    o[0] = (float)s[0]; o[1] = (float)s[1]; o[2] = (float)s[2]; o[3] = (float)s[3];
  } else if constexpr (KIND == GYMRL_ENV_MOUNTAINCAR) {
    o[0] = (float)s[0]; o[1] = (float)s[1];
  } else if constexpr (KIND == GYMRL_ENV_ACROBOT) {
    float ob[6];
    acrobot_obs(s, ob);
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = ob[k];
  } else {
    float ob[3];
    pendulum_obs(s[0], s[1], ob);
    o[0] = ob[0]; o[1] = ob[1]; o[2] = ob[2];
  }
}

// An argument block's explicit starts f64[P][E][NS], or nullptr where the block has no such member (gymrl_classic_ppo_eval_args)
template <class Args>
__device__ __forceinline__ auto episode_starts(const Args& a, int) -> decltype(a.start) { return a.start; }
template <class Args>
__device__ __forceinline__ const double* episode_starts(const Args&, long) { return nullptr; }

// KIND: GYMRL_ENV_CARTPOLE, GYMRL_ENV_MOUNTAINCAR, GYMRL_ENV_ACROBOT (action(t) -> int) or GYMRL_ENV_PENDULUM (action(t) -> the torque, float).
// Args: an argument block with E, cap, seed, stream_id0, returns (float or double), lengths, terminated, final_obs and, optionally,
// start (include/gymrl.h).  obs_rows / pitch: the 16 rows the forward reads the observations from, `pitch` floats apart — the
// slab's L.S at kMaxD (eval_kernels_device.hpp) or mlp::forward_tile's input tile at mlp::kInStride (eval_classic_ppo.hip); all
// `pitch` columns of the 16 rows are zeroed here once.  `running` is the caller's __shared__ word.
template <int KIND, class Args, class Forward, class Action>
__device__ __forceinline__ void run_episodes(const Args& a, float* obs_rows, const int pitch, int& running, const int p, const int e0,
                                             const int nrows, Forward&& forward, Action&& action) {
  constexpr bool cart = KIND == GYMRL_ENV_CARTPOLE, car = KIND == GYMRL_ENV_MOUNTAINCAR, acro = KIND == GYMRL_ENV_ACROBOT;
  constexpr int D = cart ? 4 : car ? 2 : acro ? 6 : 3, NS = cart || acro ? 4 : 2;          // MountainCar-v0: (pos, vel)
  const int t = threadIdx.x;
  // ---- one lane per episode: the env state, the return and the length live in registers ----
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  double ret = 0.0;
  int len = 0;
  bool terminated = false, active = t < nrows;
  if (t < 16)
    for (int k = 0; k < pitch; ++k) obs_rows[t * pitch + k] = 0.0f;      // rows beyond the episodes and columns beyond D stay zero
  if (active) {
    if (const double* start = episode_starts(a, 0)) {
#pragma unroll
      for (int k = 0; k < NS; ++k) s[k] = start[((int64_t)p * a.E + e0 + t) * NS + k];
    } else if constexpr (cart) {
      cartpole_draw(a.seed, (uint64_t)(a.stream_id0 + e0 + t), 0u, s);
    } else if constexpr (car) {
      mountaincar_draw(a.seed, (uint64_t)(a.stream_id0 + e0 + t), 0u, s[0], s[1]);
    } else if constexpr (acro) {
      acrobot_draw(a.seed, (uint64_t)(a.stream_id0 + e0 + t), 0u, s);
    } else {
      pendulum_draw(a.seed, (uint64_t)(a.stream_id0 + e0 + t), 0u, s[0], s[1]);
    }
  }
  for (int it = 0; it < a.cap; ++it) {
    if (t < 64) {
      if (active) episode_obs<KIND>(s, obs_rows + t * pitch);
      const bool any = __ballot(active) != 0ull;
      if (t == 0) running = any ? 1 : 0;
    }
    __syncthreads();
    if (!running) break;                  // one word, the same for every thread of the workgroup
    forward();
    if (active) {
      if constexpr (cart) {
        terminated = cartpole_advance(s[0], s[1], s[2], s[3], action(t));
        ret = ret + 1.0;
      } else if constexpr (car) {
        terminated = mountaincar_advance(s[0], s[1], action(t));
        ret = ret + (-1.0);                 // every step, the terminating one included
      } else if constexpr (acro) {
        terminated = acrobot_advance(s, action(t));
        ret = ret + (terminated ? 0.0 : -1.0);  // every step but the terminating one
      } else {
        ret = ret + (-pendulum_advance(s[0], s[1], action(t)));
      }
      len += 1;
      active = !terminated && len < a.cap;
    }
    // (the next iteration's stores to the input rows and `running` follow forward()'s closing barrier; their last readers sit in front of it)
  }
  if (t < nrows) {
    const int64_t i = (int64_t)p * a.E + e0 + t;
    a.returns[i] = (decltype(+a.returns[i]))ret; a.lengths[i] = len; a.terminated[i] = terminated;
    if (a.final_obs) episode_obs<KIND>(s, a.final_obs + i * D);
  }
}

inline bool aligned(const void* p, size_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) == 0; }

// What the entry points refuse alike, before the first HIP call: the sizes, the stride, the streams, the outputs and their alignment
template <class Args>
inline bool episode_args_ok(const Args& a, int max_cap) {
  if (a.P < 1 || a.E < 1 || a.cap < 1 || a.cap > max_cap || a.stream_id0 < 0) return false;
  if ((int64_t)a.P * a.E > 0x7fffffffLL) return false;
  if (a.policy_stride < 0 || (a.policy_stride & 3) != 0 || (a.policy_stride == 0 && a.P != 1)) return false;
  if (a.images && a.P != 1) return false;
  if (!all_set({a.returns, a.lengths, a.terminated})) return false;
  return aligned(a.images, 16) && aligned(a.start, 8) && aligned(a.returns, 4) && aligned(a.lengths, 4) && aligned(a.final_obs, 4);
}

}  // namespace
}  // namespace slab
}  // namespace gymrl
