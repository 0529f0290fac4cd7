// collect_lunar_rnn.hip — one collection round of the PPG-RNN / PPO-RNN LunarLander trainers in ONE launch of ONE workgroup.
//
// Replaces the step loop of collect_round() (ppg_rnn_lunarlander.py) as the trainers run it: per vector step an env-step launch,
// a gymrl_running_norm_masked launch, a gymrl_reward_scaling_masked launch, a gymrl_mlprnn_act launch, four elementwise ops and
// every sixteenth step a blocking read-back, up to 1001 times.  The workgroup is laid out like lunar_eval_mlprnn_kernel
// (eval_lunar_rnn.hip): all four waves run the forward of the 16 rows (mlprnn_device.hpp's forward_tile), wave 0 steps the envs
// four lanes per env (env_lunar_device.hpp); the worlds and the GRU states stay in LDS from the reset to the round's end.
//
//   iteration 0    wave 0: VecEnv.reset()'s arithmetic for envs env_id0 + i (episode 0), the running-norm update over the first
//                  observations -> states[0] and the input tile; everybody: the forward; wave 0: the draw under counter0
//                  -> act / logp / value[0]
//   iteration t+1  wave 0: env_step_once under act[t] for the envs live at t; done[t], dw[t], ep_ret, the length; the running-norm
//                  update over the step's observations (the terminal one where an episode ended) -> states[t + 1] and the input
//                  tile; reward scaling -> rew[t]; everybody: the forward; wave 0: the draw under counter0 + t + 1 for the envs
//                  live at t (NOT t + 1: an env whose episode just ended gets this one forward on its terminal state, whose
//                  value is its stored next value) -> act / logp / value[t + 1]; live[t + 1] = live[t] & !done[t]
//
// The two running statistics consume their rows one after the other in env order (running_norm_kernel: one lane per feature;
// reward_scaling_kernel: one lane), so they are sequential here too: every lane of wave 0 carries the statistics of feature
// lane & 7 and of the reward in registers from the launch's start to its end, env i's values reach it by a wave shuffle, lanes
// 0..7 store.  One workgroup can keep that order and several cannot, hence N <= 16.
//
// Exit discipline, eval_lunar_device.hpp's: every iteration wave 0 writes ONE LDS word, "is any env live", in front of a barrier
// every thread reaches, and everybody reads it behind that barrier.  No __syncthreads() sits behind a per-lane or per-wave
// condition, there are no atomics and no global flags, nothing waits for another workgroup (there is none), and the loop runs at
// most cap + 1 times.
#include "clamped_policy_device.hpp"
#include "eval_lunar_device.hpp"
#include "mlprnn_device.hpp"
#include "running_norm_device.hpp"

using namespace gymrl;
using namespace gymrl::lunar;
namespace R = gymrl::mlprnn;

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kMaxEnvs = 16;                         // one workgroup's rows
constexpr int kParamPtrs = sizeof(gymrl_mlprnn_params) / sizeof(const float*);
static_assert(sizeof(gymrl_mlprnn_params) == kParamPtrs * sizeof(const float*), "the table is an array of float pointers");
// dynamic LDS: the forward's tiles, then the input tile [16][LD_X]
constexpr int kDynBytes = (R::kTileFloats + R::kRows * R::LD_X) * 4;
static_assert(R::kTileFloats % 4 == 0 && R::kRows == kMaxEnvs && R::LD_X >= kEvalObs && kEnvsPerBlock == kMaxEnvs, "LDS carve-up");

// One pass of the solver for the env of this quad, eval_step_quad with the step's own reward handed out (collect_round() sums
// it in float32) and no cut: reset() at `start` (the world is built here and stepped with action 0 under the reset draw's
// force, len = 0), else step() of the parked world with step_idx = len.  The world goes back to the parking area.  Call with a
// quad-uniform `active`; an idle quad touches nothing.
__device__ __forceinline__ void collect_step_quad(const Lds& lds, int role, bool active, bool start, int action, uint64_t seed,
                                                  uint64_t env, float (&o)[8], int& len, float& reward, bool& terminated) {
  if (active) {
    World W;
    uint32_t episode = 0u;
    double unused = 0.0;
    float fx = 0.0f, fy = 0.0f;
    int act = action < 0 ? 0 : (action > 3 ? 3 : action);
    len = 0;
    if (start) { init_episode(W, lds, seed, env, 0u, fx, fy); act = 0; }
    else world_park(W, lds, false, episode, len, unused);
    env_step_once(W, lds, role, act, seed, env, 0u, (uint32_t)len, fx, fy, o, reward, terminated);
    if (!start) len += 1;
    world_park(W, lds, true, episode, len, unused);
  }
}

__global__ __launch_bounds__(kThreads) void lunar_collect_mlprnn_kernel(const gymrl_lunar_collect_args a,
                                                                        const gymrl_mlprnn_params P0) {
  extern __shared__ __attribute__((aligned(16))) float dyn_lds[];
  __shared__ uint32_t lds_words[kLdsWords * kEnvBlock];            // the solver's per-lane columns (wave 0)
  __shared__ uint32_t lds_park[kParkWords * kEnvBlock];            // wave 0's worlds between the steps
  __shared__ gymrl_mlprnn_params pp;                               // the parameter table: the forward reads it from LDS
  __shared__ float zl[R::kRows][kEvalActions + 1];
  __shared__ int running;                                          // the loop's exit word
  const R::Tiles t = R::carve(dyn_lds);
  float* xin = dyn_lds + R::kTileFloats;
  float* const hs = t.hs;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int role = lane & 3, row = lane >> 2, feat = lane & 7;     // wave 0's views: four lanes per env; a feature per lane
  const int N = a.N;
#ifdef GYMRL_LUNAR_PROF
  const Lds slds{lds_words + lane, nullptr, lds_park + lane};
#else
  const Lds slds{lds_words + lane, lds_park + lane};
#endif
  const uint64_t env = (uint64_t)(a.env_id0 + row);
  // (all of this is published by the loop's first barrier)
  if (tid < kParamPtrs) reinterpret_cast<const float**>(&pp)[tid] = reinterpret_cast<const float* const*>(&P0)[tid];
  for (int i = tid; i < R::kRows * R::LD_H; i += kThreads) hs[i] = 0.0f;     // every episode starts from h = 0
  for (int i = tid; i < R::kRows * R::LD_X; i += kThreads) xin[i] = 0.0f;
  // wave 0's statistics, in registers for the whole round: feature `feat` of the observations, the reward's, this quad's R
  double on = 0.0, oS = 0.0, ostd = 0.0, rn = 0.0, rS = 0.0, rstd = 0.0, Rq = 0.0;
  float omean = 0.0f, rmean = 0.0f;
  if (wave == 0) {
    on = a.norm_stats[0];
    omean = running_norm_mean(a.norm_stats, feat);
    oS = a.norm_stats[2 + kEvalObs + feat];
    ostd = running_norm_std(a.norm_stats, kEvalObs, feat);
    rn = a.reward_stats[0];
    rmean = running_norm_mean(a.reward_stats, 0);
    rS = a.reward_stats[3];
    rstd = running_norm_std(a.reward_stats, 1, 0);
    if (row < N) Rq = a.R[row];
  }
  bool active = wave == 0 && row < N;                               // quad-uniform: live at the step this iteration plays
  int act = 0, len = 0;
  float ret = 0.0f;
  for (int it = 0; it <= a.cap; ++it) {
    bool done = false;
    if (wave == 0) {
      const unsigned long long livemask = __ballot(active);
      if (lane == 0) running = livemask != 0ull ? 1 : 0;
      float o[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, reward = 0.0f;
      bool terminated = false;
      collect_step_quad(slds, role, active, it == 0, act, a.seed, env, o, len, reward, terminated);
      if (it > 0 && active) {
        done = terminated || len >= kMaxSteps;                      // truncated: the env's own limit, as gymrl_env_step reports it
        ret = ret + reward;                                         // float32, collect_round()'s ep_ret
        if (role == 0) {
          a.done[(size_t)(it - 1) * N + row] = done ? 1 : 0;
          a.dw[(size_t)(it - 1) * N + row] = terminated ? 1 : 0;
        }
      }
      // the statistics, live rows in env order: lane 4i + r holds o[r] and o[4 + r] of env i
      const float lo = role == 0 ? o[0] : (role == 1 ? o[1] : (role == 2 ? o[2] : o[3]));
      const float hi = role == 0 ? o[4] : (role == 1 ? o[5] : (role == 2 ? o[6] : o[7]));
      for (int i = 0; i < N; ++i) {
        if (!((livemask >> (4 * i)) & 1ull)) continue;              // (wave-uniform)
        const float xl = __shfl(lo, 4 * i + (lane & 3)), xh = __shfl(hi, 4 * i + (lane & 3));
        const float xv = (lane & 4) ? xh : xl;                      // component `feat` of env i's observation
        running_norm_update(xv, on, omean, oS, ostd);
        const float y = running_norm_point(xv, omean, ostd);
        if (lane < kEvalObs) {
          a.states[((size_t)it * N + i) * kEvalObs + lane] = y;
          xin[i * R::LD_X + lane] = y;                              // the forward's input tile
        }
        if (it > 0) {                                               // (uniform: `it` is the loop counter)
          const float rw = __shfl(reward, 4 * i);
          double Ri = __shfl(Rq, 4 * i);
          const float ys = reward_scaling_step(rw, a.gamma, Ri, rn, rmean, rS, rstd);
          if (row == i) Rq = Ri;
          if (lane == 0) a.rew[(size_t)(it - 1) * N + i] = ys;
        }
      }
    }
    __syncthreads();                      // the word, the input tile of this step
    if (!running) break;                  // one word, the same for every thread of the workgroup
    // the new hidden state replaces the old one in the tile: each thread overwrites the element it read
    R::forward_tile<kWaves, kEvalActions>(pp, kEvalObs, xin, t, zl, [hs](int rr, int u, float hn) { hs[rr * R::LD_H + u] = hn; });
    if (wave == 0) {
      if (active) {                       // gymrl_mlprnn_act's sampling branch, masked by live at the step just played
        float z[kEvalActions], p[kEvalActions], lp;
#pragma unroll
        for (int k = 0; k < kEvalActions; ++k) z[k] = zl[row][k];
        act = clamped_policy_act<kEvalActions>(z, nullptr, a.seed, env, a.counter0 + (uint64_t)it, 0, lp, p);
        if (role == 0) {
          a.act[(size_t)it * N + row] = act;
          a.logp[(size_t)it * N + row] = lp;
          a.value[(size_t)it * N + row] = zl[row][kEvalActions];
        }
      }
      if (it > 0) active = active && !done;
      if (role == 0 && row < N) a.live[(size_t)it * N + row] = active ? 1 : 0;
    }
    // (the next iteration's stores to `running` and the input tile sit behind forward_tile's barriers, its last readers in
    // front of them)
  }
  if (wave == 0) {                        // the statistics as the loop's kernels leave them
    if (lane < kEvalObs) {
      a.norm_stats[2 + lane] = (double)omean;
      a.norm_stats[2 + kEvalObs + lane] = oS;
      a.norm_stats[2 + 2 * kEvalObs + lane] = ostd;
    }
    if (lane == 0) {
      a.norm_stats[0] = on;
      a.reward_stats[0] = rn; a.reward_stats[2] = (double)rmean; a.reward_stats[3] = rS; a.reward_stats[4] = rstd;
    }
    if (role == 0 && row < N) { a.R[row] = Rq; a.ep_ret[row] = ret; a.lengths[row] = len; }
  }
}

// What the entry point refuses before the first HIP call
inline bool collect_args_ok(const gymrl_lunar_collect_args* a) {
  if (!a) return false;
  if (a->N < 1 || a->N > kMaxEnvs || a->cap < 1 || a->cap > kMaxSteps || a->env_id0 < 0) return false;
  const void* f64[] = {a->norm_stats, a->reward_stats, a->R};
  for (const void* p : f64)
    if (!p || !eval_aligned(p, 8)) return false;
  const void* w32[] = {a->act, a->logp, a->value, a->rew, a->ep_ret, a->lengths};
  for (const void* p : w32)
    if (!p || !eval_aligned(p, 4)) return false;
  if (!a->done || !a->dw || !a->live) return false;
  return a->states && eval_aligned(a->states, 16);               // rows of 8 floats
}

}  // namespace

extern "C" {

size_t gymrl_lunar_collect_args_bytes(void) { return sizeof(gymrl_lunar_collect_args); }

int gymrl_lunar_mlprnn_collect(const gymrl_lunar_collect_args* a, const gymrl_mlprnn_params* policy, void* stream) {
  if (!collect_args_ok(a) || !R::params_ok(policy)) return -22;
  static bool attr_set = false;
  if (const int rc = set_max_lds_once(attr_set, {(const void*)lunar_collect_mlprnn_kernel}, kDynBytes)) return rc;
  hipLaunchKernelGGL(lunar_collect_mlprnn_kernel, dim3(1), dim3(kThreads), kDynBytes, (hipStream_t)stream, *a, *policy);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
