// eval_lunar_device.hpp — the episode loop of the one-launch LunarLander evaluation, stated once: eval_lunar.hip's two kernels
// (PPO's Linear + Tanh network, PPO-full's mHC network) and eval_lunar_rnn.hip's (the PPG / PPO-RNN recurrent network)
// instantiate it with their own policy: its forward, its greedy pick, what it reads of an observation, and what it keeps of an
// episode at its end.
//
// ONE workgroup of THREADS threads (mlp::kWaves * 64 in eval_lunar.hip) carries 16 episodes of one policy from their reset to their end, laid out like
// rollout_lunar_kernel: every wave runs the policy forward on the 16 observations, wave 0 then steps the 16 envs four lanes
// per env (env_lunar_device.hpp).  What the rollout has and this loop has not: no slab, no draw, no GAE state, no next episode
// (so no spare world, no refill wave and no env_state buffer) — the worlds are built in the kernel and never touch HBM.
//
//   iteration 0   wave 0 builds episode 0 of its envs: init_episode + env_step_once(action 0), VecEnv.reset()'s arithmetic
//                 (lunar_reset_kernel), parks the worlds in LDS and puts the observations into the forward's input tile
//   iteration t   everybody: the forward of the 16 observations, closed by a barrier; wave 0: the policy's pick (LogitsPolicy:
//                 the FIRST maximum of the four logits, categorical_pick's deterministic scan), un-park, env_step_once with step_idx = len,
//                 ret = ret + (double)reward, park, next observation -> input tile; an episode that ended writes its
//                 results, once, and its quad idles from then on (its input row keeps its last observation and is computed
//                 along, unread)
//
// Every iteration opens with wave 0 writing ONE LDS word, "is anybody still running", in front of a barrier every thread
// reaches; everybody reads the word behind it, so the exit is uniform.  No __syncthreads() sits behind a per-lane or per-wave
// condition, nothing waits for another workgroup, there are no atomics and no global flags, global memory is only written
// where an episode ends, and the loop runs at most cap + 1 times (the reset pass and cap steps).
#pragma once
#include "env_lunar_device.hpp"
#include "mlp_device.hpp"
#include "policy_device.hpp"

namespace gymrl {
namespace lunar {
namespace {

constexpr int kEvalThreads = mlp::kWaves * 64;
constexpr int kEvalActions = 4, kEvalObs = 8;

// which 16 episodes of which policy this workgroup carries: the grid is P * ceil(E / 16)
struct EpisodeSlot {
  int p, e0;
  __device__ explicit EpisodeSlot(int E) {
    const int groups = (E + 15) / 16;
    p = (int)blockIdx.x / groups;
    e0 = ((int)blockIdx.x - p * groups) * 16;
  }
};

// One pass of the solver for the episode of this quad — the ONE call site of env_step_once in an evaluation kernel.
//   start   (wave-uniform) reset(): the world is built here and stepped with action 0 under the reset draw's force; the reward
//           is dropped, len = 0, ret = 0
//   else    step(): the world comes from the parking area, step_idx = len, ret = ret + (double)reward (lunar_step_quad's order)
// Either way the world goes back to the parking area and `o` is the observation after the pass.  Returns whether the episode is
// over: terminated by the env, or cut at `cap` steps (terminated = false).  Call with a quad-uniform `active`; an idle quad
// touches nothing.
__device__ __forceinline__ bool eval_step_quad(const Lds& lds, int role, bool active, bool start, int action, uint64_t seed,
                                               uint64_t env, int cap, float (&o)[8], int& len, double& ret, bool& terminated) {
  bool done = false;
  if (active) {
    World W;
    uint32_t episode = 0u;
    float fx = 0.0f, fy = 0.0f, reward;
    bool term;
    int act = action < 0 ? 0 : (action > 3 ? 3 : action);
    len = 0; ret = 0.0;
    if (start) { init_episode(W, lds, seed, env, 0u, fx, fy); act = 0; }
    else world_park(W, lds, false, episode, len, ret);
    env_step_once(W, lds, role, act, seed, env, 0u, (uint32_t)len, fx, fy, o, reward, term);
    if (!start) {
      len += 1;
      ret = ret + (double)reward;
      terminated = term;
      done = term || len >= cap;
    }
    world_park(W, lds, true, episode, len, ret);
  }
  return done;
}

// The policy of the two feed-forward kernels: the first maximum of the four logits in head [16][mlp::kHeadStride] (columns 0..3),
// the raw observation as the input, nothing kept at an episode's end.
template <class Forward>
struct LogitsPolicy {
  const float* head;
  Forward fwd;
  __device__ __forceinline__ void forward() { fwd(); }
  __device__ __forceinline__ int pick(int row) const {
    float z[kEvalActions], lp, H;
#pragma unroll
    for (int k = 0; k < kEvalActions; ++k) z[k] = head[row * mlp::kHeadStride + k];
    return categorical_pick<kEvalActions>(z, nullptr, 0ull, 0ull, 0ull, 1, lp, H);
  }
  __device__ __forceinline__ float input(int, float x) const { return x; }
  __device__ __forceinline__ void episode_end(int64_t, int, int) const {}
};
template <class Forward>
__device__ __forceinline__ LogitsPolicy<Forward> logits_policy(const float* head, Forward fwd) { return LogitsPolicy<Forward>{head, fwd}; }

// THREADS: the workgroup's size (wave 0 steps the envs whatever it is).  xin: the forward's input tile [16][xstride] (columns 0..7
// are written here, the rest is zeroed once).  `running`: the caller's __shared__ word.  The policy supplies
//   forward()                  every thread: the forward of the input tile, closed by a workgroup barrier
//   pick(row) -> action        wave 0: the greedy action of the tile's row `row`, read from the forward's output
//   input(k, x) -> float       wave 0: what the input tile takes for component k of an observation, x itself or x normalised
//   episode_end(i, row, role)  wave 0, the four lanes of the quad: episode i = p * E + e has just ended
template <int THREADS, class Policy>
__device__ __forceinline__ void run_lunar_episodes(const gymrl_lunar_eval_args& a, uint32_t* lds_words, uint32_t* lds_park, int& running,
                                                   float* xin, const int xstride, const int p, const int e0, Policy&& policy) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int role = lane & 3, row = lane >> 2, e = e0 + row;        // wave 0's view: four lanes per env
#ifdef GYMRL_LUNAR_PROF
  const Lds slds{lds_words + lane, nullptr, lds_park + lane};
#else
  const Lds slds{lds_words + lane, lds_park + lane};
#endif
  const uint64_t env = (uint64_t)(a.stream_id0 + e);
  bool active = wave == 0 && e < a.E;                               // quad-uniform; rows beyond the episodes never start
  for (int i = tid; i < mlp::kRows * xstride; i += THREADS) xin[i] = 0.0f;
  for (int it = 0; it <= a.cap; ++it) {
    if (wave == 0) {
      const bool any = __ballot(active) != 0ull;
      if (lane == 0) running = any ? 1 : 0;
    }
    __syncthreads();                      // the word, the input tile of this step (at it == 0: its zeroes)
    if (!running) break;                  // one word, the same for every thread of the workgroup
    if (it > 0) policy.forward();         // (uniform: `it` is the loop counter)
    else __syncthreads();                 // everybody has read the word before wave 0 comes round to write it again
    if (wave == 0) {
      int act = 0;
      if (it > 0) act = policy.pick(row);
      float o[8];
      int len = 0;
      double ret = 0.0;
      bool terminated = false;
      const bool done = eval_step_quad(slds, role, active, it == 0, act, a.seed, env, a.cap, o, len, ret, terminated);
      if (active) {
        if (role < 2) {                   // next policy input: straight into the forward's LDS tile
#pragma unroll
          for (int k = 0; k < 4; ++k) xin[row * xstride + 4 * role + k] = policy.input(4 * role + k, o[4 * role + k]);
        }
        if (done) policy.episode_end((int64_t)p * a.E + e, row, role);
        if (done && role == 0) {
          const int64_t i = (int64_t)p * a.E + e;
          a.returns[i] = ret; a.lengths[i] = len; a.terminated[i] = terminated ? 1 : 0;
          if (a.terminal_obs) {
            float4* t = reinterpret_cast<float4*>(a.terminal_obs) + 2 * i;
            t[0] = make_float4(o[0], o[1], o[2], o[3]); t[1] = make_float4(o[4], o[5], o[6], o[7]);
          }
        }
        active = !done;
      }
    }
    // (the next iteration's stores to `running` and the input tile's last readers sit in front of forward()'s barriers)
  }
}

inline bool eval_aligned(const void* p, size_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) == 0; }

// What both entry points refuse alike, before the first HIP call
inline bool eval_args_ok(const gymrl_lunar_eval_args* a) {
  if (!a || !a->returns || !a->lengths || !a->terminated) return false;
  if (a->P < 1 || a->E < 1 || a->cap < 1 || a->cap > kMaxSteps || a->stream_id0 < 0) return false;
  if ((int64_t)a->P * a->E > 0x7fffffffLL) return false;
  if (a->policy_stride < 0 || (a->policy_stride & 3) != 0 || (a->policy_stride == 0 && a->P != 1)) return false;
  return eval_aligned(a->returns, 8) && eval_aligned(a->lengths, 4) && eval_aligned(a->terminal_obs, 16);
}

}  // namespace
}  // namespace lunar
}  // namespace gymrl
