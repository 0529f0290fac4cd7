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

// Categorical(softmax(z)) of the acting step, stated once for gymrl_mlprnn_act and the one-launch recurrent collection
// (collect_lunar_rnn.hip) -> the action; lp = its log-prob, p = softmax(z).
//   deterministic   probs.argmax(): the first maximum
//   else            torch.multinomial(probs / sum, 1): argmax p2 / q with the first maximum winning, q ~ Exp(1) — `noise_row`
//                   (A explicit draws) or, without one, Philox under the keys of gymrl_categorical_sample (policy_device.hpp):
//                   (seed, env, counter, RNG_POLICY | ...), q = -log(u) with u in (0, 1]
template <int A>
__device__ __forceinline__ int clamped_policy_act(const float (&z)[A], const float* __restrict__ noise_row, uint64_t seed,
                                                  uint64_t env, uint64_t counter, int deterministic, float& lp, float (&p)[A]) {
  float S, p2[A], L[A], c[A];
  bool inb[A];
  clamped_policy<A>(z, p, S, p2, L, c, inb);
  int a = 0;
  if (deterministic) {
    float best = p[0];
#pragma unroll
    for (int k = 1; k < A; ++k) if (p[k] > best) { best = p[k]; a = k; }
  } else {
    float qv[A];
    if (noise_row) {
#pragma unroll
      for (int k = 0; k < A; ++k) qv[k] = noise_row[k];
    } else {
#pragma unroll
      for (int blk = 0; blk < (A + 3) / 4; ++blk) {
        const u32x4 rn = philox4x32(seed, (uint32_t)env, (uint32_t)(env >> 32), (uint32_t)counter,
                                    RNG_POLICY | ((uint32_t)((counter >> 32) & 0x3FFFFFu) << 2) | (uint32_t)blk);
        const uint32_t wv[4] = {rn.x, rn.y, rn.z, rn.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (blk * 4 + k < A) qv[blk * 4 + k] = -det_logf(u01f_open0(wv[k]));
      }
    }
    float best = p2[0] / qv[0];
#pragma unroll
    for (int k = 1; k < A; ++k) {
      const float cand = p2[k] / qv[k];
      if (cand > best) { best = cand; a = k; }
    }
  }
  lp = L[0];
#pragma unroll
  for (int k = 1; k < A; ++k) if (a == k) lp = L[k];
  return a;
}

}  // namespace gymrl
