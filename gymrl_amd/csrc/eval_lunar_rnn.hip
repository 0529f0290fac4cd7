// eval_lunar_rnn.hip — whole evaluation episodes of LunarLander-v3 under the recurrent PPG / PPO-RNN policy (PSCN -> MLPRNN
// (GRU) -> heads), P policies x E episodes in ONE launch.
//
// Replaces the eval() loop of ppg_rnn_lunarlander.py:501-524 / ppo_rnn_lunarlander.py as the trainers run it: per env step a
// gymrl_mlprnn_act launch, an env-step launch, two elementwise ops, a gymrl_running_norm_masked launch and every sixteenth step a
// blocking read-back, up to 1001 times.  Here a workgroup carries 16 episodes of one policy from their reset to their end:
//
//   lunar_eval_mlprnn_kernel   the loop is eval_lunar_device.hpp's run_lunar_episodes, the forward mlprnn_device.hpp's forward_tile
//                              (the acting kernel's P1-P8), the observation's way into the input tile running_norm_device.hpp's
//                              point, the pick gymrl_mlprnn_act's deterministic branch: clamped_policy<4> on the logits and the
//                              FIRST maximum of the probabilities (two different logits can round to equal probabilities, so
//                              the maximum of the logits is another pick).
//
// What no other evaluation kernel has is per-episode policy state carried from step to step: the hidden state hs[16][64] starts at
// zero and stays in LDS for the whole episode (after the GRU cell each thread overwrites the element it read); it reaches global
// memory only where an episode ends, and only if h_final is asked for.  Rows e >= E and ended episodes are computed along, unread.
// Policy p reads every pointer of gymrl_mlprnn_params p * policy_stride floats behind policy 0's: the workgroup shifts the table
// once, into LDS, and the forward reads it from there, so that no operand address is hoisted out of the episode loop.
#include "clamped_policy_device.hpp"
#include "eval_lunar_device.hpp"
#include "mlprnn_device.hpp"
#include "running_norm_device.hpp"

using namespace gymrl;
using namespace gymrl::lunar;
namespace R = gymrl::mlprnn;

namespace {

// waves per workgroup: 4 (the product build) or 8 (-DGYMRL_EVAL_RNN_WAVES=8, the variant DESIGN §4s reports beside it)
#ifndef GYMRL_EVAL_RNN_WAVES
#define GYMRL_EVAL_RNN_WAVES 4
#endif
constexpr int kRnnWaves = GYMRL_EVAL_RNN_WAVES;
static_assert(kRnnWaves == 4 || kRnnWaves == 8, "forward_tile's P1 deals whole rows of 256 columns");
constexpr int kParamPtrs = sizeof(gymrl_mlprnn_params) / sizeof(const float*);
static_assert(sizeof(gymrl_mlprnn_params) == kParamPtrs * sizeof(const float*), "the table is an array of float pointers");
// dynamic LDS: the forward's tiles, then the input tile [16][LD_X].  With the solver's columns and parking: > 80 KB, one
// workgroup per CU
constexpr int kDynFloatsRnn = R::kTileFloats + R::kRows * R::LD_X;
constexpr int kDynBytesRnn = kDynFloatsRnn * 4;
static_assert(R::kTileFloats % 4 == 0 && R::kRows == 16 && R::LD_X >= kEvalObs, "LDS carve-up");

struct RnnPolicy {
  const gymrl_mlprnn_params& pp;     // this workgroup's policy (LDS)
  const R::Tiles t;
  const float* xin;
  float (*zl)[kEvalActions + 1];
  const float* nmean;                // LDS [8], [8]; read only with `normed`
  const double* nstd;
  const bool normed;
  float* h_final;

  // the new hidden state replaces the old one in the tile: each thread overwrites the element it read
  __device__ __forceinline__ void forward() {
    float* const hs = t.hs;
    R::forward_tile<kRnnWaves, kEvalActions>(pp, kEvalObs, xin, t, zl, [hs](int rr, int u, float hn) { hs[rr * R::LD_H + u] = hn; });
  }
  // gymrl_mlprnn_act with deterministic = 1: probs.argmax(), the first maximum
  __device__ __forceinline__ int pick(int row) const {
    float z[kEvalActions], pr[kEvalActions], S, p2[kEvalActions], L[kEvalActions], c[kEvalActions];
    bool inb[kEvalActions];
#pragma unroll
    for (int k = 0; k < kEvalActions; ++k) z[k] = zl[row][k];
    clamped_policy<kEvalActions>(z, pr, S, p2, L, c, inb);
    int act = 0;
    float best = pr[0];
#pragma unroll
    for (int k = 1; k < kEvalActions; ++k) if (pr[k] > best) { best = pr[k]; act = k; }
    return act;
  }
  // gymrl_running_norm_masked(update = 0) on the observation, or the observation itself
  __device__ __forceinline__ float input(int k, float x) const { return normed ? running_norm_point(x, nmean[k], nstd[k]) : x; }
  // the hidden state after the episode's last forward: a quarter of the row per lane of the quad
  __device__ __forceinline__ void episode_end(int64_t i, int row, int role) const {
    if (!h_final) return;
    const float4* src = reinterpret_cast<const float4*>(t.hs + row * R::LD_H + 16 * role);
    float4* dst = reinterpret_cast<float4*>(h_final + i * R::kH + 16 * role);
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[j] = src[j];
  }
};

__global__ __launch_bounds__(64 * kRnnWaves) void lunar_eval_mlprnn_kernel(const gymrl_lunar_eval_args a, const gymrl_mlprnn_params P0,
                                                                           const double* __restrict__ norm_stats,
                                                                           const int64_t norm_stride, float* __restrict__ h_final) {
  constexpr int kThreads = 64 * kRnnWaves;
  extern __shared__ __attribute__((aligned(16))) float dyn_lds[];
  __shared__ uint32_t lds_words[kLdsWords * kEnvBlock];            // the solver's per-lane columns (wave 0)
  __shared__ uint32_t lds_park[kParkWords * kEnvBlock];            // wave 0's worlds between the steps
  __shared__ gymrl_mlprnn_params pp;                               // the parameter table of this workgroup's policy
  __shared__ double nstd[kEvalObs];
  __shared__ float nmean[kEvalObs];
  __shared__ float zl[R::kRows][kEvalActions + 1];
  __shared__ int running;                                          // the loop's exit word
  const R::Tiles t = R::carve(dyn_lds);
  float* xin = dyn_lds + R::kTileFloats;
  const int tid = threadIdx.x;
  const EpisodeSlot slot(a.E);
  // (all of this is published by the loop's first barrier)
  if (tid < kParamPtrs)
    reinterpret_cast<const float**>(&pp)[tid] =
        reinterpret_cast<const float* const*>(&P0)[tid] + (size_t)slot.p * (size_t)a.policy_stride;
  if (norm_stats && tid >= 64 && tid < 64 + kEvalObs) {
    const double* s = norm_stats + (size_t)slot.p * (size_t)norm_stride;
    nmean[tid - 64] = running_norm_mean(s, tid - 64);
    nstd[tid - 64] = running_norm_std(s, kEvalObs, tid - 64);
  }
  for (int i = tid; i < R::kRows * R::LD_H; i += kThreads) t.hs[i] = 0.0f;   // every episode starts from h = 0
  run_lunar_episodes<kThreads>(a, lds_words, lds_park, running, xin, R::LD_X, slot.p, slot.e0,
                               RnnPolicy{pp, t, xin, zl, nmean, nstd, norm_stats != nullptr, h_final});
}

}  // namespace

extern "C" {

int gymrl_lunar_mlprnn_eval(const gymrl_lunar_eval_args* a, const gymrl_mlprnn_params* policy, const double* norm_stats,
                            int64_t norm_stride, float* h_final, void* stream) {
  if (!eval_args_ok(a) || !R::params_ok(policy)) return -22;
  if (norm_stride < 0 || (norm_stride != 0 && norm_stride < 2 + 3 * kEvalObs)) return -22;
  if (!eval_aligned(norm_stats, 8) || !eval_aligned(h_final, 16)) return -22;
  static bool attr_set = false;
  if (const int rc = set_max_lds_once(attr_set, {(const void*)lunar_eval_mlprnn_kernel}, kDynBytesRnn)) return rc;
  const dim3 grid((unsigned)(a->P * ((a->E + 15) / 16)));
  hipLaunchKernelGGL(lunar_eval_mlprnn_kernel, grid, dim3(64 * kRnnWaves), kDynBytesRnn, (hipStream_t)stream, *a, *policy,
                     norm_stats, norm_stride, h_final);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
