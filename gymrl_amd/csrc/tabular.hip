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

// the wave's 64 tables between HBM Q[R][S][A] (one contiguous block per wave, read and written in whole lines) and LDS;
// kRuns: the runs a workgroup carries = the LDS row's length
template <int S, bool kLoad, int kRuns = kEnvBlock>
__device__ __forceinline__ void copy_tables(double* lds, double* Q, int run0, int nvalid, int lane) {
  constexpr int E = S * kActions;
  double* g = Q + (size_t)run0 * E;
  for (int f = lane; f < nvalid * E; f += kEnvBlock) {
    const int run = f / E, e = f - run * E;
    if (kLoad) lds[e * kRuns + run] = g[f];
    else g[f] = lds[e * kRuns + run];
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

// ---- SARSA, Expected SARSA, Double Q-learning (include/gymrl.h states the three loops) --------------------------------------
enum { kSarsa = GYMRL_TABULAR_RULE_SARSA, kExpectedSarsa = GYMRL_TABULAR_RULE_EXPECTED_SARSA, kDoubleQ = GYMRL_TABULAR_RULE_DOUBLE_Q };

// runs per workgroup: Double Q-learning's two CliffWalking tables are 2 x 96 KB for 64 runs and a compute unit has 160 KB, so
// that instance deals 32 runs to a workgroup (lanes 32..63 idle; the [entry][32] row still puts lane l on banks 2l, 2l + 1)
constexpr int td_runs(int rule, int kind) { return rule == kDoubleQ && kind == kCliff ? 32 : kEnvBlock; }
constexpr size_t td_lds_bytes(int rule, int kind) {
  return sizeof(double) * (size_t)(rule == kDoubleQ ? 2 : 1) * (kind == kCliff ? kCliffStates : kFrozenStates) * kActions * td_runs(rule, kind);
}

struct TdArgs {
  TrainArgs t;
  double* Q2;      // Double Q-learning's QB
  int k_limit;     // draws a run can take = entries of eps the kernel may read
};

// One iteration = one draw.  Expected SARSA and Double Q-learning: Q-learning's loop, an iteration is a step.  SARSA: an
// iteration takes the step of the pending action (where there is one) and draws the action that follows it from the SAME
// call site, so a wave whose lanes sit at different points of their episodes still pays one Philox call per iteration:
//   a step that does not end its episode    a2 = select(s2) on the table before the write, target = r + gamma Q[s2, a2]
//   a step that ends it with done            target = r, write, then select(start) of the next episode (the row is read before
//                                            the write and patched with the written value where s is the start state)
//   a step that runs out at max_steps        a2 as in the first line, used by the target and dropped; the next iteration is
//   no pending action (run start, run-out)   select(start) alone: no step, no write
// The slip word of a step is the draw's that chose its action: after a launch seam it is drawn again from k.
template <int RULE, int KIND, bool kSlippery, bool kShaped, int kRuns>
__global__ __launch_bounds__(kEnvBlock) void td_train_kernel(const TdArgs ta) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int S = Env<KIND>::S, kRow = kActions * kRuns, kTable = S * kRow;
  const TrainArgs& a = ta.t;
  const int lane = threadIdx.x, run0 = blockIdx.x * kRuns, r = run0 + lane;
  const int nvalid = min(kRuns, a.R - run0);
  const bool valid = lane < nvalid;
  copy_tables<S, true, kRuns>(lds, a.Q, run0, nvalid, lane);
  if constexpr (RULE == kDoubleQ) copy_tables<S, true, kRuns>(lds + kTable, ta.Q2, run0, nvalid, lane);
  __syncthreads();

  const TdRunState st(a.state, a.R);
  int s = Env<KIND>::start, episode = 0, step = 0, k = 0, act = -1;
  double ret = 0.0;
  if (valid && !a.restart) {
    s = st.state[r]; episode = st.episode[r]; step = st.step[r]; k = st.k[r]; ret = st.ep_ret[r];
    if constexpr (RULE == kSarsa) act = st.pending[r];
  }
  const uint64_t stream = (uint64_t)(a.run_id0 + r);
  double* q = lds + lane;                                    // entry (s, act) of this lane's table: q[(s * A + act) * kRuns]
  bool active = valid && episode >= 0 && episode < a.max_episodes && (unsigned)s < (unsigned)S && step >= 0 && step < a.max_steps && k >= 0 &&
                k < ta.k_limit && act >= -1 && act < kActions && (act < 0 || k > 0);
  double eps_next = active ? a.eps[k] : 0.0;
  uint32_t slip = 0u;
  if constexpr (RULE == kSarsa && KIND == kFrozen && kSlippery) {
    if (active && act >= 0) slip = step_draw(a.seed, stream, (uint32_t)k).slip_word;
  }

  for (int it = 0; it < a.max_iters; ++it) {
    if (__ballot(active) == 0ull) break;
    if (active) {
      const double eps = eps_next;
      const StepDraw d = step_draw(a.seed, stream, (uint32_t)(k + 1));
      if constexpr (RULE == kSarsa) {
        const bool pending = act >= 0;
        const TabStep e = env_step<KIND, kSlippery>(s, pending ? act : 0, slip, step);
        const bool done = pending && (e.terminated || e.truncated);
        const bool over = pending && (done || step + 1 >= a.max_steps);
        const double rew = (KIND == kFrozen && kShaped) ? frozenlake_shaped_reward(s, e.next) : e.reward;
        double* cell = q + (s * kActions + (pending ? act : 0)) * kRuns;
        const double predict = *cell;
        const double end_value = predict + a.lr * (rew - predict);           // what a done step writes
        const int x = pending ? (done ? Env<KIND>::start : e.next) : s;      // the state the draw acts in
        const double* row = q + x * kRow;
        double x0 = row[0], x1 = row[kRuns], x2 = row[2 * kRuns], x3 = row[3 * kRuns];
        if (done && x == s) {                                                // the next episode starts on the row being written
          x0 = act == 0 ? end_value : x0; x1 = act == 1 ? end_value : x1; x2 = act == 2 ? end_value : x2; x3 = act == 3 ? end_value : x3;
        }
        const int a2 = d.u < eps ? draw_below(d.action_word, kActions) : argmax4(x0, x1, x2, x3);
        bool drew = true;
        if (pending) {
          const double target = rew + a.gamma * pick4(a2, x0, x1, x2, x3);
          *cell = done ? end_value : predict + a.lr * (target - predict);
          ret = ret + rew;
          step += 1;
          s = x;
          if (over) {
            a.ep_rewards[(size_t)r * a.max_episodes + episode] = ret;
            a.ep_lengths[(size_t)r * a.max_episodes + episode] = step;
            episode += 1; step = 0; ret = 0.0; s = Env<KIND>::start;
            active = episode < a.max_episodes;
            drew = !done || active;                                          // the last episode's done step draws nothing
          }
        }
        act = (over && !done) ? -1 : a2;                                     // run out: the drawn action is dropped
        slip = d.slip_word;
        if (drew) k += 1;
      } else {
        k += 1;
        const double* row = q + s * kRow;
        const double q0 = row[0], q1 = row[kRuns], q2 = row[2 * kRuns], q3 = row[3 * kRuns];
        double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
        if constexpr (RULE == kDoubleQ) { b0 = row[kTable]; b1 = row[kTable + kRuns]; b2 = row[kTable + 2 * kRuns]; b3 = row[kTable + 3 * kRuns]; }
        const int greedy = RULE == kDoubleQ ? argmax4(q0 + b0, q1 + b1, q2 + b2, q3 + b3) : argmax4(q0, q1, q2, q3);
        act = d.u < eps ? draw_below(d.action_word, kActions) : greedy;
        const TabStep e = env_step<KIND, kSlippery>(s, act, d.slip_word, step);
        const bool done = e.terminated || e.truncated;
        const double rew = (KIND == kFrozen && kShaped) ? frozenlake_shaped_reward(s, e.next) : e.reward;
        const double* nrow = q + e.next * kRow;
        const double n0 = nrow[0], n1 = nrow[kRuns], n2 = nrow[2 * kRuns], n3 = nrow[3 * kRuns];
        double boot, predict;
        int table = 0;
        if constexpr (RULE == kExpectedSarsa) {
          boot = eps * 0.25 * (((n0 + n1) + n2) + n3) + (1.0 - eps) * max4(n0, n1, n2, n3);
          predict = pick4(act, q0, q1, q2, q3);
        } else {
          const double m0 = nrow[kTable], m1 = nrow[kTable + kRuns], m2 = nrow[kTable + 2 * kRuns], m3 = nrow[kTable + 3 * kRuns];
          const bool coin = (d.action_word & 1u) != 0u;                      // 0: QA learns from QB, 1: QB from QA
          const int best = coin ? argmax4(m0, m1, m2, m3) : argmax4(n0, n1, n2, n3);
          boot = coin ? pick4(best, n0, n1, n2, n3) : pick4(best, m0, m1, m2, m3);
          predict = coin ? pick4(act, b0, b1, b2, b3) : pick4(act, q0, q1, q2, q3);
          table = coin ? kTable : 0;
        }
        const double target = done ? rew : rew + a.gamma * boot;
        q[table + (s * kActions + act) * kRuns] = predict + a.lr * (target - predict);
        ret = ret + rew;
        step += 1;
        s = e.next;
        if (done || step >= a.max_steps) {
          a.ep_rewards[(size_t)r * a.max_episodes + episode] = ret;
          a.ep_lengths[(size_t)r * a.max_episodes + episode] = step;
          episode += 1; step = 0; ret = 0.0; s = Env<KIND>::start;
          active = episode < a.max_episodes;
        }
      }
      if (k < ta.k_limit) eps_next = a.eps[k];
    }
  }

  if (valid) {
    st.state[r] = s; st.episode[r] = episode; st.step[r] = step; st.k[r] = k; st.ep_ret[r] = ret;
    st.pending[r] = RULE == kSarsa ? act : -1;
    a.k_out[r] = k; a.episodes_out[r] = episode;
  }
  __syncthreads();
  copy_tables<S, false, kRuns>(lds, a.Q, run0, nvalid, lane);
  if constexpr (RULE == kDoubleQ) copy_tables<S, false, kRuns>(lds + kTable, ta.Q2, run0, nvalid, lane);
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

template <int RULE, int KIND, bool kSlippery, bool kShaped>
inline void launch_td(const TdArgs& a, hipStream_t s) {
  constexpr int kRuns = td_runs(RULE, KIND);
  hipLaunchKernelGGL((td_train_kernel<RULE, KIND, kSlippery, kShaped, kRuns>), dim3((a.t.R + kRuns - 1) / kRuns), dim3(kEnvBlock),
                     td_lds_bytes(RULE, KIND), s, a);
}
template <int RULE>
inline void launch_td_rule(int env_kind, bool is_slippery, bool shaped, const TdArgs& a, hipStream_t s) {
  if (env_kind == kCliff) launch_td<RULE, kCliff, false, false>(a, s);
  else if (is_slippery) { if (shaped) launch_td<RULE, kFrozen, true, true>(a, s); else launch_td<RULE, kFrozen, true, false>(a, s); }
  else { if (shaped) launch_td<RULE, kFrozen, false, true>(a, s); else launch_td<RULE, kFrozen, false, false>(a, s); }
}
template <int RULE, int KIND, bool kSlippery, bool kShaped>
inline const void* td_kernel() { return (const void*)td_train_kernel<RULE, KIND, kSlippery, kShaped, td_runs(RULE, KIND)>; }

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

size_t gymrl_tabular_state_bytes(int rule, int n_runs) {
  return rule >= GYMRL_TABULAR_RULE_QLEARNING && rule <= kDoubleQ && n_runs > 0 ? TdRunState(nullptr, n_runs).bytes : 0;
}

size_t gymrl_tabular_args_bytes(void) { return sizeof(gymrl_tabular_train_args); }

int gymrl_tabular_train(const gymrl_tabular_train_args* p, void* stream) {
  if (!p) return -22;
  const int rule = p->rule;
  if (rule < GYMRL_TABULAR_RULE_QLEARNING || rule > kDoubleQ || !kind_ok(p->env_kind)) return -22;
  if (p->n_runs <= 0 || p->max_episodes <= 0 || p->max_steps <= 0 || p->max_iters < 0 || p->run_id0 < 0) return -22;
  // draws a run can take: SARSA's episode that runs out has drawn the action of a step it never takes
  const int64_t draws = (int64_t)p->max_episodes * (p->max_steps + (rule == kSarsa ? 1 : 0));
  if (draws > 0x7fffffffLL || p->eps_len < draws) return -22;                             // k and the eps table's index are int32
  if ((rule == kDoubleQ) != (p->Q2 != nullptr)) return -22;
  if (!all_set({p->Q, p->state, p->eps_table, p->episode_rewards, p->episode_lengths, p->k_out, p->episodes_out})) return -22;
  if (!aligned(p->Q, 8) || !aligned(p->Q2, 8) || !aligned(p->state, 256) || !aligned(p->eps_table, 8) || !aligned(p->episode_rewards, 8) ||
      !aligned(p->episode_lengths, 4) || !aligned(p->k_out, 4) || !aligned(p->episodes_out, 4)) return -22;
  if (rule == GYMRL_TABULAR_RULE_QLEARNING)                                               // the same kernel, the same bits
    return gymrl_qlearn_train(p->env_kind, p->is_slippery, p->shaped, p->Q, p->state, p->n_runs, p->restart, p->seed, p->run_id0, p->eps_table,
                              p->max_episodes, p->max_steps, p->max_iters, p->lr, p->gamma, p->episode_rewards, p->episode_lengths, p->k_out,
                              p->episodes_out, stream);
  if (p->max_iters == 0 && !p->restart) return 0;
  // above the 64 KB a kernel gets unasked: one CliffWalking table of 64 runs, two of 32, two FrozenLake tables of 64 (64 KB sharp)
  static bool attr_set = false;
  if (const int rc = set_max_lds_once(attr_set, {td_kernel<kSarsa, kCliff, false, false>(), td_kernel<kExpectedSarsa, kCliff, false, false>(),
                                                 td_kernel<kDoubleQ, kCliff, false, false>(), td_kernel<kDoubleQ, kFrozen, true, true>(),
                                                 td_kernel<kDoubleQ, kFrozen, true, false>(), td_kernel<kDoubleQ, kFrozen, false, true>(),
                                                 td_kernel<kDoubleQ, kFrozen, false, false>()}, (int)td_lds_bytes(kSarsa, kCliff))) return rc;
  const TdArgs a{{p->Q, p->state, p->n_runs, p->restart != 0, p->seed, p->run_id0, p->eps_table, p->max_episodes, p->max_steps, p->max_iters,
                  p->lr, p->gamma, p->episode_rewards, p->episode_lengths, p->k_out, p->episodes_out}, p->Q2, (int)draws};
  hipStream_t s = (hipStream_t)stream;
  const bool slippery = p->is_slippery != 0, shaped = p->shaped != 0;
  if (rule == kSarsa) launch_td_rule<kSarsa>(p->env_kind, slippery, shaped, a, s);
  else if (rule == kExpectedSarsa) launch_td_rule<kExpectedSarsa>(p->env_kind, slippery, shaped, a, s);
  else launch_td_rule<kDoubleQ>(p->env_kind, slippery, shaped, a, s);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
