// tabular_device.hpp — FrozenLake-v1 (4x4) / CliffWalking-v0: ONE env's step, the per-step draw and the per-run loop record
// as device functions.
//
// The arithmetic of gym.make("FrozenLake-v1", map_name="4x4" | "CliffWalking-v0").step() (gymnasium toy_text, third-party:
// SURVEY.md 8c.2) for one env = one lane, integer state, branch-free selects; include/gymrl.h states the rules.  Shared by the
// population trainer and the greedy evaluator (tabular.hip), so both step the same env.
#pragma once
#include "env_common.hpp"

namespace gymrl {
namespace tabular {

// ---- the draw: ONE Philox4x32-10 call per (stream, k) -------------------------------------------------------------------------
// key = seed; counter = (stream & 0xffffffff, stream >> 32, k, RNG_TABULAR).  stream: cfg.run_id0 + r while training, a disjoint
// range (the trainers' 1 << 40 habit) while evaluating; k: the run's training action (the reference's sample_count, from 1) or
// the evaluation episode's step (from 1).  Words:
//   x, y -> u = u01d(x, y), explore iff u < eps_k        z -> exploring action (z * A) >> 32        w -> slip choice (w * 3) >> 32
// (tests/tabular_ref.py restates this layout once, through oracle.philox.)
constexpr uint32_t RNG_TABULAR = 0x70000000u;
struct StepDraw { double u; uint32_t action_word, slip_word; };
__device__ __forceinline__ StepDraw step_draw(uint64_t seed, uint64_t stream, uint32_t k) {
  const u32x4 r = philox4x32(seed, (uint32_t)stream, (uint32_t)(stream >> 32), k, RNG_TABULAR);
  return StepDraw{u01d(r.x, r.y), r.z, r.w};
}
__device__ __forceinline__ int draw_below(uint32_t word, uint32_t n) { return (int)(((uint64_t)word * n) >> 32); }

struct TabStep { int next; double reward; bool terminated, truncated; };

// FrozenLake-v1 4x4, SFFF / FHFH / FFFH / HFFG, state = row * 4 + col, start 0.  Actions 0 LEFT, 1 DOWN, 2 RIGHT, 3 UP, clipped
// at the border; slippery: the executed direction is (a - 1) % 4, a, (a + 1) % 4 by the slip choice 0, 1, 2.  Reward 1 on
// entering the goal (15), terminated on a hole {5, 7, 11, 12} or the goal, truncated when the episode's step count (len_before +
// 1) reaches the env's own 100.
constexpr int kFrozenStates = 16, kFrozenStart = 0, kFrozenGoal = 15, kFrozenLimit = 100;
constexpr uint32_t kFrozenHoles = (1u << 5) | (1u << 7) | (1u << 11) | (1u << 12);
template <bool kSlippery>
__device__ __forceinline__ TabStep frozenlake_step_one(int s, int a, uint32_t slip_word, int len_before) {
  const int dir = kSlippery ? ((a + 3 + draw_below(slip_word, 3u)) & 3) : a;
  int row = s >> 2, col = s & 3;
  col = dir == 0 ? (col > 0 ? col - 1 : 0) : (dir == 2 ? (col < 3 ? col + 1 : 3) : col);
  row = dir == 1 ? (row < 3 ? row + 1 : 3) : (dir == 3 ? (row > 0 ? row - 1 : 0) : row);
  TabStep r;
  r.next = row * 4 + col;
  const bool goal = r.next == kFrozenGoal, hole = ((kFrozenHoles >> r.next) & 1u) != 0u;
  r.reward = goal ? 1.0 : 0.0;
  r.terminated = goal || hole;
  r.truncated = len_before + 1 >= kFrozenLimit;
  return r;
}
// qlearning_frozenlake.py:63-79 _shape_reward, in its order: hole, goal, stayed in place, any other move
__device__ __forceinline__ double frozenlake_shaped_reward(int s, int next) {
  const bool hole = ((kFrozenHoles >> next) & 1u) != 0u;
  return hole ? -10.0 : (next == kFrozenGoal ? 100.0 : (next == s ? -5.0 : -1.0));
}

// CliffWalking-v0, 4 x 12, state = row * 12 + col, start 36, goal 47, cliff 37..46.  Actions 0 UP, 1 RIGHT, 2 DOWN, 3 LEFT,
// clipped at the border; entering the cliff costs -100 and puts the agent back on 36 without terminating, every other step
// costs -1; terminated at the goal only; no time limit of its own.
constexpr int kCliffStates = 48, kCliffStart = 36, kCliffGoal = 47;
__device__ __forceinline__ TabStep cliffwalking_step_one(int s, int a) {
  int row = s / 12, col = s - row * 12;
  row = a == 0 ? (row > 0 ? row - 1 : 0) : (a == 2 ? (row < 3 ? row + 1 : 3) : row);
  col = a == 1 ? (col < 11 ? col + 1 : 11) : (a == 3 ? (col > 0 ? col - 1 : 0) : col);
  const bool cliff = row == 3 && col >= 1 && col <= 10;
  TabStep r;
  r.next = cliff ? kCliffStart : row * 12 + col;
  r.reward = cliff ? -100.0 : -1.0;
  r.terminated = r.next == kCliffGoal;
  r.truncated = false;
  return r;
}

// np.argmax / np.max over one table row of four actions: the FIRST maximum
__device__ __forceinline__ int argmax4(double q0, double q1, double q2, double q3) {
  int a = 0; double m = q0;
  if (q1 > m) { m = q1; a = 1; }
  if (q2 > m) { m = q2; a = 2; }
  if (q3 > m) { a = 3; }
  return a;
}
__device__ __forceinline__ double max4(double q0, double q1, double q2, double q3) {
  double m = q0;
  m = q1 > m ? q1 : m; m = q2 > m ? q2 : m; m = q3 > m ? q3 : m;
  return m;
}
// entry a of a row held in four registers, by selects (a runtime-indexed register array would go to scratch)
__device__ __forceinline__ double pick4(int a, double q0, double q1, double q2, double q3) {
  return a == 0 ? q0 : (a == 1 ? q1 : (a == 2 ? q2 : q3));
}

constexpr int kActions = 4;

// Per-run loop state between launches, SoA over the runs: what train() of qlearning_*.py keeps in locals
struct RunState {
  double* ep_ret;      // episode_reward so far
  int32_t* state;      // env state
  int32_t* episode;    // episodes finished = index of the running one
  int32_t* step;       // steps taken in the running episode
  int32_t* k;          // training actions taken (sample_count)
  size_t bytes;
  __host__ __device__ RunState(void* buf, int n) {
    Carver c(buf, n);
    ep_ret = c.take<double>(); state = c.take<int32_t>(); episode = c.take<int32_t>(); step = c.take<int32_t>(); k = c.take<int32_t>();
    bytes = c.off;
  }
};
// gymrl_tabular_train's record: RunState (so rule 0 hands it to the Q-learning kernel as it is) and, behind it, SARSA's pending
// action — the one select(s) drew for the step not yet taken, -1 where the next iteration draws afresh
struct TdRunState : RunState {
  int32_t* pending;
  __host__ __device__ TdRunState(void* buf, int n) : RunState(buf, n) {
    Carver c(buf, n);
    c.off = bytes;
    pending = c.take<int32_t>();
    bytes = c.off;
  }
};

}  // namespace tabular
}  // namespace gymrl
