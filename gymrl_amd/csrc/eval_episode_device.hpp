// eval_episode_device.hpp — the episode loop of the one-launch policy evaluation, stated once: eval_classic.hip (a three-layer MLP
// on CartPole-v1 / Pendulum-v1), eval_duel.hip (a dueling network on CartPole-v1) and eval_net.hip (either network on
// MountainCar-v0 / Acrobot-v1) instantiate it, through eval_kernels_device.hpp, with their own "policy forward" and "action" steps;
// eval_classic_ppo.hip with PPO's.  What an env is comes from EpisodeEnv<KIND> (env_classic_device.hpp) alone.
//
// ONE workgroup of slab::kThreads threads carries 16 episodes of one policy from their reset to their end.  Lane t < 16 of wave 0
// owns episode e0 + t: its float64 env state, its float64 return, its length and its flags live in registers.  Per iteration
//
//   wave 0       puts the float32 observation of every running lane's state into its row of the forward's input (the caller says
//                where the 16 rows lie: a pointer and a pitch) and writes ONE LDS word, "is anybody still running", beside them
//   everybody    meets at the barrier that publishes both and leaves on that word — the same for every thread of the workgroup
//   forward()    every thread: the policy's stages over the slab, each closed by a workgroup barrier, the last one included
//   action(t)    the running lanes: the greedy action of row t, then EpisodeEnv<KIND>::advance in registers
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

// An argument block's explicit starts f64[P][E][NS], or nullptr where the block has no such member (gymrl_classic_ppo_eval_args)
template <class Args>
__device__ __forceinline__ auto episode_starts(const Args& a, int) -> decltype(a.start) { return a.start; }
template <class Args>
__device__ __forceinline__ const double* episode_starts(const Args&, long) { return nullptr; }

// KIND: an env kind with an EpisodeEnv (env_classic_device.hpp); action(t) -> its Action, an index or Pendulum-v1's torque.
// Args: an argument block with E, cap, seed, stream_id0, returns (float or double), lengths, terminated, final_obs and, optionally,
// start (include/gymrl.h).  obs_rows / pitch: the 16 rows the forward reads the observations from, `pitch` floats apart — the
// slab's L.S at kMaxD (eval_kernels_device.hpp) or mlp::forward_tile's input tile at mlp::kInStride (eval_classic_ppo.hip); all
// `pitch` columns of the 16 rows are zeroed here once.  `running` is the caller's __shared__ word.
template <int KIND, class Args, class Forward, class Action>
__device__ __forceinline__ void run_episodes(const Args& a, float* obs_rows, const int pitch, int& running, const int p, const int e0,
                                             const int nrows, Forward&& forward, Action&& action) {
  using Env = EpisodeEnv<KIND>;
  constexpr int D = Env::kObs, NS = Env::kState;
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
    } else {
      Env::draw(a.seed, (uint64_t)(a.stream_id0 + e0 + t), s);
    }
  }
  for (int it = 0; it < a.cap; ++it) {
    if (t < 64) {
      if (active) Env::obs(s, obs_rows + t * pitch);
      const bool any = __ballot(active) != 0ull;
      if (t == 0) running = any ? 1 : 0;
    }
    __syncthreads();
    if (!running) break;                  // one word, the same for every thread of the workgroup
    forward();
    if (active) {
      terminated = Env::advance(s, action(t), ret);
      len += 1;
      active = !terminated && len < a.cap;
    }
    // (the next iteration's stores to the input rows and `running` follow forward()'s closing barrier; their last readers sit in front of it)
  }
  if (t < nrows) {
    const int64_t i = (int64_t)p * a.E + e0 + t;
    a.returns[i] = (decltype(+a.returns[i]))ret; a.lengths[i] = len; a.terminated[i] = terminated;
    if (a.final_obs) Env::obs(s, a.final_obs + i * D);
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

// One layer of policy 0 as an argument block names it.  A layer the network has is both tensors, the weight on 16 bytes and the
// bias on 4; one it has not (a second hidden layer, a value head) is neither.
struct EvalLayer { const float *w, *b; bool present; };
inline bool layers_ok(std::initializer_list<EvalLayer> layers) {
  for (const EvalLayer& l : layers)
    if (l.present ? !(l.w && l.b && aligned(l.w, 16) && aligned(l.b, 4)) : (l.w || l.b)) return false;
  return true;
}
// `images` is fc2's forward image: of a trunk that has an fc2, at a width that has an image
inline bool fc2_image_ok(const float* images, bool two, int H) { return !images || (two && (H & 15) == 0); }

// The launch of the checked block `a`.  pick(wide, v) -> the kernel instance of variant v (which network, on which env: the
// entry point's own numbering, N_VARIANTS of them) built for hidden width 256 (wide) or for any a.H.  The first call raises the
// dynamic-LDS ceiling of EVERY instance pick can answer with, so the list cannot fall behind the launch.
template <int N_VARIANTS, class Args, class Pick>
inline int launch_episodes(const Args& a, void* stream, bool& lds_set, int variant, int n_hidden, Pick&& pick) {
  if (!lds_set) {
    const void* all[2 * N_VARIANTS];
    for (int v = 0; v < N_VARIANTS; ++v) {
      all[2 * v] = (const void*)pick(false, v);
      all[2 * v + 1] = (const void*)pick(true, v);
    }
    if (const int rc = set_max_lds_once(lds_set, all, all + 2 * N_VARIANTS, (int)lds_bytes(256, 2))) return rc;
  }
  const dim3 grid((unsigned)(a.P * ((a.E + 15) / 16))), block(kThreads);
  const bool wide = a.H == 256;           // the instances built for the reference's hidden width
  hipLaunchKernelGGL(pick(wide, variant), grid, block, lds_bytes(a.H, n_hidden), (hipStream_t)stream, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // namespace
}  // namespace slab
}  // namespace gymrl
