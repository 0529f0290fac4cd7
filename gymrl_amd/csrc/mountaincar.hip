// mountaincar.hip — the rule-based MountainCar-v0 baseline for a POPULATION of policies and episodes.
//
// Replaces RuleBasedAgent.select_action() / run_episode() / eval() of mountaincar_baseline.py:35-84, P policies x E episodes at
// a time.  One episode is a strictly serial chain (at most 200 steps of six float64 operations and one cos) and gains nothing
// from a GPU; P * E episodes are independent, so one LANE is one (policy, episode) pair and they all run to their end in one
// launch with no host round trip.  Position, velocity, step count and the policy's nine coefficients live in registers: no
// LDS, no atomics, no workgroup waits for another.  The env arithmetic is env_classic_device.hpp's mountaincar_advance, the one
// the stepper (env_classic.hip) calls, so an episode here and the first episode of a stepped env are the same bits.
#include "env_classic_device.hpp"

using namespace gymrl;

namespace {

constexpr int kCoefs = 9;
constexpr int kMaxSteps = 200;                     // MountainCar-v0's TimeLimit

struct EvalArgs {
  int P, E, cap;
  uint64_t seed; int64_t stream_id0;
  const double* coefs; const double* start;
  double* returns; int32_t* lengths; uint8_t* reached; double* final_state;
};

// select_action (mountaincar_baseline.py:35-45) in float64 on the float32 observation, powers as products
__device__ __forceinline__ int rule_action(const double (&k)[kCoefs], double pos, double vel) {
  const double p = (double)(float)pos, v = (double)(float)vel;
  const double a = p + k[1];
  const double l1 = k[0] * (a * a) + k[2];
  const double b = p + k[4];
  const double b2 = b * b;
  const double l2 = k[3] * (b2 * b2) - k[5];
  const double lb = l1 < l2 ? l1 : l2;
  const double c = p + k[7];
  const double ub = k[6] * (c * c) + k[8];
  return (lb < v && v < ub) ? 2 : 0;
}

__global__ __launch_bounds__(kEnvBlock) void mountaincar_rule_eval_kernel(const EvalArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kEnvBlock + threadIdx.x;
  const bool valid = i < (int64_t)a.P * a.E;
  double k[kCoefs] = {-0.09, 0.25, 0.03, 0.3, 0.9, 0.008, -0.07, 0.38, 0.07};
  double pos = 0.0, vel = 0.0;
  if (valid) {
    if (a.coefs) {
      const double* src = a.coefs + (size_t)(i / a.E) * kCoefs;
#pragma unroll
      for (int j = 0; j < kCoefs; ++j) k[j] = src[j];
    }
    if (a.start) { pos = a.start[2 * i]; vel = a.start[2 * i + 1]; }
    else mountaincar_draw(a.seed, (uint64_t)(a.stream_id0 + i), 0u, pos, vel);
  }
  int t = 0;
  double ret = 0.0;
  bool reached = false, active = valid;
  for (int it = 0; it < a.cap; ++it) {
    if (__ballot(active) == 0ull) break;
    if (active) {
      reached = mountaincar_advance(pos, vel, rule_action(k, pos, vel));
      ret = ret + (-1.0);
      t += 1;
      active = !reached;
    }
  }
  if (valid) {
    a.returns[i] = ret; a.lengths[i] = t; a.reached[i] = reached;
    if (a.final_state) { a.final_state[2 * i] = pos; a.final_state[2 * i + 1] = vel; }
  }
}

inline bool aligned(const void* p, size_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) == 0; }

}  // namespace

extern "C" {

int gymrl_mountaincar_rule_eval(const gymrl_mountaincar_eval_args* args, void* stream) {
  if (!args) return -22;
  const gymrl_mountaincar_eval_args& g = *args;
  if (g.P < 1 || g.E < 1 || g.cap < 1 || g.cap > kMaxSteps || g.stream_id0 < 0) return -22;
  if (!g.coefs && g.P != 1) return -22;
  const int64_t n = (int64_t)g.P * g.E;
  if (n > 0x7fffffffLL) return -22;
  if (!g.returns || !g.lengths || !g.reached) return -22;
  if (!aligned(g.coefs, 8) || !aligned(g.start, 8) || !aligned(g.returns, 8) || !aligned(g.lengths, 4) || !aligned(g.final_state, 8)) return -22;
  const EvalArgs a{g.P, g.E, g.cap, g.seed, g.stream_id0, g.coefs, g.start, g.returns, g.lengths, g.reached, g.final_state};
  hipLaunchKernelGGL(mountaincar_rule_eval_kernel, dim3((unsigned)((n + kEnvBlock - 1) / kEnvBlock)), dim3(kEnvBlock), 0, (hipStream_t)stream, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
