// tabular.hip — tabular Q-learning on FrozenLake-v1 / CliffWalking-v0 for a POPULATION of independent runs.
//
// Replaces QLearningTrainer.train() / eval() of qlearning_frozenlake.py:96-153 and qlearning_cliffwalking.py:71-124, R runs at
// a time.  One run is a strictly serial chain (500 episodes of at most 200 steps on a 16 x 4 or 48 x 4 float64 table) and
// gains nothing from a GPU; R runs are independent, so one LANE is one run and the whole population trains in one launch
// with no host round trip.  A wave's 64 tables live in LDS as [s * A + a][lane] for the whole launch, so that every
// table access of the wave is one conflict-free 8-byte-per-lane row whatever states the lanes are in.
#include "tabular_device.hpp"

using namespace gymrl;
using namespace gymrl::tabular;

namespace {

enum { kFrozen = GYMRL_TABULAR_FROZENLAKE, kCliff = GYMRL_TABULAR_CLIFFWALKING };

template <int KIND> struct Env;
template <> struct Env<kFrozen> { static constexpr int S = kFrozenStates, start = kFrozenStart; };
template <> struct Env<kCliff> { static constexpr int S = kCliffStates, start = kCliffStart; };
constexpr size_t table_lds_bytes(int S) { return sizeof(double) * (size_t)S * kActions * kEnvBlock; }

template <int KIND, bool kSlippery>
__device__ __forceinline__ TabStep env_step(int s, int a, uint32_t slip_word, int len_before) {
  if constexpr (KIND == kFrozen) return frozenlake_step_one<kSlippery>(s, a, slip_word, len_before);
  else return cliffwalking_step_one(s, a);
}

struct TrainArgs {
  double* Q; void* state; int R, restart;
  uint64_t seed; int64_t run_id0;
  const double* eps; int max_episodes, max_steps, max_iters;
  double lr, gamma;
  double* ep_rewards; int32_t* ep_lengths; int32_t* k_out; int32_t* episodes_out;
};

// the wave's 64 tables between HBM Q[R][S][A] (one contiguous block per wave, read and written in whole lines) and LDS
template <int S, bool kLoad>
__device__ __forceinline__ void copy_tables(double* lds, double* Q, int run0, int nvalid, int lane) {
  constexpr int E = S * kActions;
  double* g = Q + (size_t)run0 * E;
  for (int f = lane; f < nvalid * E; f += kEnvBlock) {
    const int run = f / E, e = f - run * E;
    if (kLoad) lds[e * kEnvBlock + run] = g[f];
    else g[f] = lds[e * kEnvBlock + run];
  }
}

template <int KIND, bool kSlippery, bool kShaped>
__global__ __launch_bounds__(kEnvBlock) void qlearn_train_kernel(const TrainArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int S = Env<KIND>::S;
  const int lane = threadIdx.x, run0 = blockIdx.x * kEnvBlock, r = run0 + lane;
  const int nvalid = min(kEnvBlock, a.R - run0);
  const bool valid = lane < nvalid;
  copy_tables<S, true>(lds, a.Q, run0, nvalid, lane);
  __syncthreads();

  const RunState st(a.state, a.R);
  int s = Env<KIND>::start, episode = 0, step = 0, k = 0;
  double ret = 0.0;
  if (valid && !a.restart) { s = st.state[r]; episode = st.episode[r]; step = st.step[r]; k = st.k[r]; ret = st.ep_ret[r]; }
  const uint64_t stream = (uint64_t)(a.run_id0 + r);
  double* q = lds + lane;                                    // entry (s, act) of this lane's table: q[(s * A + act) * 64]
  // a record this library did not write (restart never asked for) leaves its run idle rather than index anything with it
  bool active = valid && episode >= 0 && episode < a.max_episodes && (unsigned)s < (unsigned)S && step >= 0 && step < a.max_steps && k >= 0 &&
                k < a.max_episodes * a.max_steps;
  // eps_k does not depend on the step before it: its load is issued one step ahead of its use
  double eps_next = active ? a.eps[k] : 0.0;

  for (int it = 0; it < a.max_iters; ++it) {
    if (__ballot(active) == 0ull) break;
    if (active) {
      k += 1;
      const double eps = eps_next;
      if (k < a.max_episodes * a.max_steps) eps_next = a.eps[k];
      const StepDraw d = step_draw(a.seed, stream, (uint32_t)k);
      const double* row = q + s * (kActions * kEnvBlock);
      const double q0 = row[0], q1 = row[kEnvBlock], q2 = row[2 * kEnvBlock], q3 = row[3 * kEnvBlock];
      const int act = d.u < eps ? draw_below(d.action_word, kActions) : argmax4(q0, q1, q2, q3);
      const TabStep e = env_step<KIND, kSlippery>(s, act, d.slip_word, step);
      const bool done = e.terminated || e.truncated;
      const double rew = (KIND == kFrozen && kShaped) ? frozenlake_shaped_reward(s, e.next) : e.reward;
      const double* nrow = q + e.next * (kActions * kEnvBlock);
      const double mx = max4(nrow[0], nrow[kEnvBlock], nrow[2 * kEnvBlock], nrow[3 * kEnvBlock]);
      const double predict = act == 0 ? q0 : (act == 1 ? q1 : (act == 2 ? q2 : q3));
      const double target = done ? rew : rew + a.gamma * mx;
      q[(s * kActions + act) * kEnvBlock] = predict + a.lr * (target - predict);
      ret = ret + rew;
      step += 1;
      s = e.next;
      if (done || step >= a.max_steps) {                     // `for step in range(max_steps)` runs out without a done flag
        a.ep_rewards[(size_t)r * a.max_episodes + episode] = ret;
        a.ep_lengths[(size_t)r * a.max_episodes + episode] = step;
        episode += 1; step = 0; ret = 0.0; s = Env<KIND>::start;
        active = episode < a.max_episodes;
      }
    }
  }

  if (valid) {
    st.state[r] = s; st.episode[r] = episode; st.step[r] = step; st.k[r] = k; st.ep_ret[r] = ret;
    a.k_out[r] = k; a.episodes_out[r] = episode;
  }
  __syncthreads();
  copy_tables<S, false>(lds, a.Q, run0, nvalid, lane);
}

struct EvalArgs {
  const double* Q; int R, E;
  uint64_t seed; int64_t stream_id0; int cap;
  double* returns; int32_t* lengths; uint8_t* flags;
};

// One lane = one (run, evaluation episode): greedy on the run's final table (read-only, from HBM), the env's raw reward summed
template <int KIND, bool kSlippery>
__global__ __launch_bounds__(kEnvBlock) void qlearn_eval_kernel(const EvalArgs a) {
  constexpr int S = Env<KIND>::S;
  const int64_t i = (int64_t)blockIdx.x * kEnvBlock + threadIdx.x;
  if (i >= (int64_t)a.R * a.E) return;
  const double* Q = a.Q + (size_t)(i / a.E) * (S * kActions);
  const uint64_t stream = (uint64_t)(a.stream_id0 + i);
  int s = Env<KIND>::start, t = 0;
  double ret = 0.0;
  bool reached = false;
  while (t < a.cap) {
    const double* row = Q + s * kActions;
    const int act = argmax4(row[0], row[1], row[2], row[3]);
    uint32_t slip_word = 0u;
    if constexpr (KIND == kFrozen && kSlippery) slip_word = step_draw(a.seed, stream, (uint32_t)(t + 1)).slip_word;
    const TabStep e = env_step<KIND, kSlippery>(s, act, slip_word, t);
    ret = ret + e.reward;
    t += 1;
    s = e.next;
    if (e.terminated || e.truncated) {
      reached = e.terminated && (KIND == kCliff || e.reward > 0.0);
      break;
    }
  }
  a.returns[i] = ret; a.lengths[i] = t; a.flags[i] = reached;
}

inline int cdiv64(int64_t n) { return (int)((n + kEnvBlock - 1) / kEnvBlock); }
inline bool aligned(const void* p, size_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) == 0; }
inline bool all_set(std::initializer_list<const void*> ps) {
  for (const void* p : ps) if (!p) return false;
  return true;
}
inline bool kind_ok(int kind) { return kind == kFrozen || kind == kCliff; }

template <int KIND, bool kSlippery, bool kShaped>
inline void launch_train(const TrainArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((qlearn_train_kernel<KIND, kSlippery, kShaped>), dim3(cdiv64(a.R)), dim3(kEnvBlock), table_lds_bytes(Env<KIND>::S), s, a);
}

}  // namespace

extern "C" {

size_t gymrl_qlearn_state_bytes(int n_runs) { return n_runs > 0 ? RunState(nullptr, n_runs).bytes : 0; }

int gymrl_qlearn_train(int env_kind, int is_slippery, int shaped, double* Q, void* state, int n_runs, int restart, uint64_t seed,
                       int64_t run_id0, const double* eps_table, int max_episodes, int max_steps, int max_iters, double lr, double gamma,
                       double* episode_rewards, int32_t* episode_lengths, int32_t* k_out, int32_t* episodes_out, void* stream) {
  if (!kind_ok(env_kind) || n_runs <= 0 || max_episodes <= 0 || max_steps <= 0 || max_iters < 0 || run_id0 < 0) return -22;
  if ((int64_t)max_episodes * max_steps > 0x7fffffffLL) return -22;                     // k and the eps table's index are int32
  if (!all_set({Q, state, eps_table, episode_rewards, episode_lengths, k_out, episodes_out})) return -22;
  if (!aligned(Q, 8) || !aligned(state, 256) || !aligned(eps_table, 8) || !aligned(episode_rewards, 8) || !aligned(episode_lengths, 4) ||
      !aligned(k_out, 4) || !aligned(episodes_out, 4)) return -22;
  if (max_iters == 0 && !restart) return 0;
  // the tables of one workgroup: 32 KB (FrozenLake) / 96 KB (CliffWalking, above the 64 KB a kernel gets unasked)
  static bool attr_set = false;
  if (const int rc = set_max_lds_once(attr_set, {(const void*)qlearn_train_kernel<kCliff, false, false>}, (int)table_lds_bytes(kCliffStates))) return rc;
  const TrainArgs a{Q, state, n_runs, restart != 0, seed, run_id0, eps_table, max_episodes, max_steps, max_iters, lr, gamma,
                    episode_rewards, episode_lengths, k_out, episodes_out};
  hipStream_t s = (hipStream_t)stream;
  if (env_kind == kCliff) launch_train<kCliff, false, false>(a, s);
  else if (is_slippery) { if (shaped) launch_train<kFrozen, true, true>(a, s); else launch_train<kFrozen, true, false>(a, s); }
  else { if (shaped) launch_train<kFrozen, false, true>(a, s); else launch_train<kFrozen, false, false>(a, s); }
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_qlearn_eval(int env_kind, int is_slippery, const double* Q, int n_runs, int n_episodes, uint64_t seed, int64_t stream_id0, int cap,
                      double* returns, int32_t* lengths, uint8_t* flags, void* stream) {
  if (!kind_ok(env_kind) || n_runs <= 0 || n_episodes <= 0 || cap <= 0 || stream_id0 < 0) return -22;
  if ((int64_t)n_runs * n_episodes > 0x7fffffffLL) return -22;
  if (!all_set({Q, returns, lengths, flags})) return -22;
  if (!aligned(Q, 8) || !aligned(returns, 8) || !aligned(lengths, 4)) return -22;
  const EvalArgs a{Q, n_runs, n_episodes, seed, stream_id0, cap, returns, lengths, flags};
  const dim3 grid(cdiv64((int64_t)n_runs * n_episodes)), block(kEnvBlock);
  hipStream_t s = (hipStream_t)stream;
  if (env_kind == kCliff) hipLaunchKernelGGL((qlearn_eval_kernel<kCliff, false>), grid, block, 0, s, a);
  else if (is_slippery) hipLaunchKernelGGL((qlearn_eval_kernel<kFrozen, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((qlearn_eval_kernel<kFrozen, false>), grid, block, 0, s, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
