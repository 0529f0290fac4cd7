// gauss_policy_device.hpp — the diagonal-Gaussian policy head (include/gymrl.h "Gaussian policy"): the draw with its
// log-probability and entropy, and one row of the clipped-surrogate loss with its gradients.  gaussian_pick is shared by
// gaussian_sample_kernel (ppo.hip) and the persistent Pendulum rollout (rollout_classic.hip), so both produce the same bits;
// tests/gauss_policy_ref.py restates every line on the host in float32 (no contraction, the grouping as written).
#pragma once
#include "gymrl_device.hpp"
#include "../../include/gymrl.h"

namespace gymrl {

constexpr float kHalfLog2Pi = 0.918938533f;          // log(sqrt(2 pi))
constexpr float kGaussEntropy0 = 1.418938533f;       // 1/2 + log(sqrt(2 pi))

// eps_k ~ N(0, 1) for k < A: Philox keyed as categorical_pick keys its words (seed, env, counter, RNG_POLICY | block); block
// k / 2 yields the pairs (x, y) -> eps_{2j}, (z, w) -> eps_{2j+1}, each turned into a normal as box_muller does.
template <int A>
__device__ __forceinline__ void gaussian_noise(uint64_t seed, uint64_t env, uint64_t counter, float (&eps)[A]) {
#pragma unroll
  for (int blk = 0; blk < (A + 1) / 2; ++blk) {
    const u32x4 r = philox4x32(seed, (uint32_t)env, (uint32_t)(env >> 32), (uint32_t)counter,
                               RNG_POLICY | ((uint32_t)((counter >> 32) & 0x3FFFFFu) << 2) | (uint32_t)blk);
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (2 * blk + h < A) {
        const float u1 = u01f_open0(w[2 * h]), u2 = u01f(w[2 * h + 1]);
        float s, c;
        det_sincosf(6.28318530717958647692f * u2, &s, &c);
        eps[2 * blk + h] = sqrtf(-2.0f * det_logf(u1)) * c;
      }
    }
  }
}

// a_k = mu_k + exp(log_std_k) * eps_k with eps from `noise_row` (explicit draws, parity mode) or Philox; deterministic: a = mu
// and eps = 0.  lp = sum_k ((-0.5 eps_k^2 - log_std_k) - log sqrt(2 pi)), H = sum_k (1/2 + log sqrt(2 pi) + log_std_k), ascending k.
template <int A>
__device__ __forceinline__ void gaussian_pick(const float (&mu)[A], const float* __restrict__ log_std,
                                              const float* __restrict__ noise_row, uint64_t seed, uint64_t env, uint64_t counter,
                                              int deterministic, float (&act)[A], float& lp, float& H) {
  float eps[A];
  if (deterministic) {
#pragma unroll
    for (int k = 0; k < A; ++k) eps[k] = 0.0f;
  } else if (noise_row) {
#pragma unroll
    for (int k = 0; k < A; ++k) eps[k] = noise_row[k];
  } else {
    gaussian_noise<A>(seed, env, counter, eps);
  }
  lp = 0.0f; H = 0.0f;
#pragma unroll
  for (int k = 0; k < A; ++k) {
    const float ls = log_std[k];
    act[k] = deterministic ? mu[k] : mu[k] + det_expf(ls) * eps[k];
    lp += (-0.5f * (eps[k] * eps[k]) - ls) - kHalfLog2Pi;
    H += kGaussEntropy0 + ls;
  }
}

// gymrl_ppo_loss_fwd_bwd's terms (policy_device.hpp ppo_loss_row) for ONE sample under the Gaussian head: the log-probability of
// the stored action a at (mu, log_std), the clipped surrogate with dual clip, value and entropy terms, the gradients to mu and v,
// this row's share of the gradient to log_std (dls), and the five metric terms.
template <int A>
__device__ __forceinline__ void ppo_gauss_loss_row(const float (&mu)[A], const float (&ls)[A], float v, const float (&a)[A], float lpo,
                                                   float ad, float rt, float invB, const gymrl_ppo_cfg& cfg, float (&dmu)[A],
                                                   float (&dls)[A], float& dv, float& m_obj, float& m_val, float& m_ent,
                                                   float& m_clip, float& m_kl) {
  float z[A], inv_std[A], lp = 0.0f, H = 0.0f;
#pragma unroll
  for (int k = 0; k < A; ++k) {
    inv_std[k] = det_expf(-ls[k]);
    z[k] = (a[k] - mu[k]) * inv_std[k];
    lp += (-0.5f * (z[k] * z[k]) - ls[k]) - kHalfLog2Pi;
    H += kGaussEntropy0 + ls[k];
  }
  const float lo = 1.0f - cfg.clip_eps, hi = 1.0f + cfg.clip_eps;
  const float ratio = det_expf(lp - lpo);
  const float s1 = ratio * ad;
  const float rc = fminf(fmaxf(ratio, lo), hi);
  const float s2 = rc * ad;
  const float inr = (ratio >= lo && ratio <= hi) ? 1.0f : 0.0f;   // clamp passes grad on [lo, hi]
  const float w1 = s1 < s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);     // torch.min tie: 1/2, 1/2
  // a NaN advantage must reach the metrics: fminf / fmaxf drop a single NaN operand, here both operands carry it
  const float ms = fminf(s1, s2);
  float dms_dr = w1 * ad + (1.0f - w1) * ad * inr;
  float obj = ms;
  if (ad < 0.0f) {
    const float dc = cfg.dual_clip * ad;
    obj = fmaxf(ms, dc);
    const float wm = ms > dc ? 1.0f : (ms == dc ? 0.5f : 0.0f);   // torch.max tie
    dms_dr *= wm;
  }
  const float g_lp = -invB * dms_dr * ratio;                      // dL/dlp = -(1/B) * dobj/dr * r
  const float g_H = -cfg.entropy_coef * invB;
#pragma unroll
  for (int k = 0; k < A; ++k) {
    dmu[k] = g_lp * (z[k] * inv_std[k]);                          // dlp/dmu_k = z_k / std_k
    dls[k] = g_lp * (z[k] * z[k] - 1.0f) + g_H;                   // dlp/dlog_std_k = z_k^2 - 1, dH/dlog_std_k = 1
  }
  const float dvr = v - rt;
  dv = cfg.value_coef * 2.0f * dvr * invB;
  m_obj = obj;
  m_val = cfg.value_coef * (dvr * dvr);
  m_ent = H;
  m_clip = (ratio < lo || ratio > hi) ? 1.0f : 0.0f;
  m_kl = lpo - lp;
}

}  // namespace gymrl
