// clamped_policy_device.hpp — torch's Categorical(probs) over probs = softmax(logits), shared by the PPG / PPO-RNN losses
// (ppg.hip, L5 / L6) and the acting step (mlprnn_act.hip), so that the log-prob an action is stored with and the one the
// update recomputes for it are the same expression (they agree on saturated probabilities, where the clamp bites).
//
// probs are renormalised p / sum(p) and every log is log(clamp(p, eps, 1 - eps)) with eps = FLT_EPSILON
// (ppg_rnn_lunarlander.py:317-319, :339-340: Categorical(prob).log_prob).
#pragma once
#include "gymrl_device.hpp"

namespace gymrl {

constexpr float kCatEps = 1.1920928955078125e-07f;       // torch.finfo(torch.float32).eps
constexpr float kCatOneMinusEps = 0.99999988079071044921875f;

// p: softmax, S = sum p, p2 = p / S, L = log(clamp(p2, eps, 1 - eps)); c = the clamped p2, inb = p2 inside [eps, 1 - eps].
template <int A>
__device__ __forceinline__ void clamped_policy(const float (&z)[A], float (&p)[A], float& S, float (&p2)[A], float (&L)[A],
                                               float (&c)[A], bool (&inb)[A]) {
  float m = z[0];
#pragma unroll
  for (int k = 1; k < A; ++k) m = fmaxf(m, z[k]);
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < A; ++k) { p[k] = det_expf(z[k] - m); s += p[k]; }
#pragma unroll
  for (int k = 0; k < A; ++k) p[k] = p[k] / s;
  S = 0.0f;
#pragma unroll
  for (int k = 0; k < A; ++k) S += p[k];
#pragma unroll
  for (int k = 0; k < A; ++k) {
    p2[k] = p[k] / S;
    inb[k] = p2[k] >= kCatEps && p2[k] <= kCatOneMinusEps;
    c[k] = fminf(fmaxf(p2[k], kCatEps), kCatOneMinusEps);
    L[k] = det_logf(c[k]);
  }
}

}  // namespace gymrl
