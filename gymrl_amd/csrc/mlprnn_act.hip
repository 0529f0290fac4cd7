// mlprnn_act.hip — the acting step of the PPG / PPO-RNN LunarLander trainers as ONE launch per vector step
// (ppg_rnn_lunarlander.py:311-320 choose_action / :322-328 evaluate_action over ActorCriticPPG.forward :165-176;
// ppo_rnn_lunarlander.py the same without the aux head, which acting never reads).
//
//   gymrl_mlprnn_act   PSCN(D, 256) (:92-122) -> MLPRNN(256, 256) = cat(rnn_linear(x), GRU step(x, h)) (:125-140)
//                      -> actor_fc / critic_fc (:156-157) -> softmax -> Categorical draw, log-prob, value
//
// Layout.  A workgroup of 8 waves owns a tile of 16 envs and carries it through the whole chain alone (rows never interact):
//   P0  inputs -> LDS   P1-P8  the network (mlprnn_device.hpp forward_tile, stated once for this kernel and the one-launch
//   evaluation)   P9  Categorical (clamped_policy_device.hpp) + draw
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gymrl.h"
#include "clamped_policy_device.hpp"
#include "mlprnn_device.hpp"

using namespace gymrl;
using namespace gymrl::mlprnn;

namespace {

constexpr int kWaves = 8;
constexpr int kThreads = 64 * kWaves;
constexpr int kMaxN = 1 << 24;

template <int A>
__global__ __launch_bounds__(kThreads) void mlprnn_act_kernel(const float* __restrict__ x, const float* __restrict__ h_in,
                                                              gymrl_mlprnn_params P, int N, int D,
                                                              const uint8_t* __restrict__ live,
                                                              const float* __restrict__ noise_exp, uint64_t seed,
                                                              uint64_t counter, int64_t env_id0, int deterministic,
                                                              float* __restrict__ h_out, int32_t* __restrict__ act_out,
                                                              float* __restrict__ logp_out, float* __restrict__ value_out,
                                                              float* __restrict__ probs_out) {
  __shared__ __attribute__((aligned(16))) float feat[kRows * LD_F];   // PSCN output (the MLPRNN input)
  __shared__ __attribute__((aligned(16))) float outs[kRows * LD_F];   // MLPRNN output (the heads' input)
  __shared__ __attribute__((aligned(16))) float hs[kRows * LD_H];
  __shared__ __attribute__((aligned(16))) float gh[kRows * LD_G];
  __shared__ __attribute__((aligned(16))) float scr[kScr];
  __shared__ float zl[kRows][A + 1];

  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;

  // P0: inputs (rows past N and features past D are zero)
  float* xs = scr;
  for (int i = tid; i < kRows * kMaxD; i += kThreads) {
    const int rr = i / kMaxD, k = i % kMaxD;
    const int64_t row = row0 + rr;
    xs[rr * LD_X + k] = (row < N && k < D) ? x[row * D + k] : 0.0f;
  }
  for (int i = tid; i < kRows * kH; i += kThreads) {
    const int rr = i / kH, u = i % kH;
    const int64_t row = row0 + rr;
    hs[rr * LD_H + u] = row < N ? h_in[row * kH + u] : 0.0f;
  }
  __syncthreads();

  // P1-P8: the network; the GRU cell's output goes to h_out as it is computed
  forward_tile<kWaves, A>(P, D, xs, Tiles{feat, outs, hs, gh, scr}, zl, [&](int rr, int u, float hn) {
    const int64_t row = row0 + rr;
    if (row < N && (!live || live[row])) h_out[row * kH + u] = hn;
  });

  // P9: Categorical(softmax(logits)) — draw, log-prob, value
  if (tid < kRows) {
    const int64_t row = row0 + tid;
    if (row >= N || (live && !live[row])) return;
    float z[A], p[A], lp;
#pragma unroll
    for (int k = 0; k < A; ++k) z[k] = zl[tid][k];
    const int a = clamped_policy_act<A>(z, noise_exp ? noise_exp + row * A : nullptr, seed, (uint64_t)(env_id0 + row), counter,
                                        deterministic, lp, p);
    act_out[row] = a;
    logp_out[row] = lp;
    value_out[row] = zl[tid][A];
    if (probs_out) {
#pragma unroll
      for (int k = 0; k < A; ++k) probs_out[row * A + k] = p[k];
    }
  }
}

}  // namespace

extern "C" {

size_t gymrl_mlprnn_params_bytes(void) { return sizeof(gymrl_mlprnn_params); }

int gymrl_mlprnn_act(const float* x, const float* h_in, const gymrl_mlprnn_params* params, int N, int D, int A,
                     const uint8_t* live, const float* noise_exp, uint64_t seed, uint64_t counter, int64_t env_id0,
                     int deterministic, float* h_out, int32_t* act, float* logp, float* value, float* probs,
                     void* stream_) {
  if (!x || !h_in || !h_out || !act || !logp || !value) return -22;
  if (N < 0 || N > kMaxN || D < 1 || D > kMaxD || A < 2 || A > 8) return -22;
  if (!params_ok(params)) return -22;      // a NULL member, a misaligned 16-byte weight
  const gymrl_mlprnn_params& P = *params;
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream_;
  const dim3 grid((N + kRows - 1) / kRows), block(kThreads);
#define MLPRNN_CASE(AA)                                                                                                   \
  case AA:                                                                                                                \
    hipLaunchKernelGGL(mlprnn_act_kernel<AA>, grid, block, 0, s, x, h_in, P, N, D, live, noise_exp, seed, counter,      \
                       env_id0, deterministic, h_out, act, logp, value, probs);                                           \
    break;
  switch (A) {
    MLPRNN_CASE(2) MLPRNN_CASE(3) MLPRNN_CASE(4) MLPRNN_CASE(5) MLPRNN_CASE(6) MLPRNN_CASE(7) MLPRNN_CASE(8)
    default: return -22;
  }
#undef MLPRNN_CASE
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
