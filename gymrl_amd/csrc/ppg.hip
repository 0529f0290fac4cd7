// ppg.hip — the per-episode pieces of the whole-episode recurrent trainers (ppg_rnn_lunarlander.py,
// ppo_rnn_lunarlander.py).  Episodes are stored back to back; segment e is rows [off[e], off[e+1]).
//
//   gymrl_episode_gae              EpisodeBuffer.compute_advantage (ppg_rnn_lunarlander.py:198-215): the f32 td-error, the
//                                  G2 recursion (gymrl_gae_dw's arithmetic), v_target = adv + values, and the per-episode
//                                  normalisation (adv - mean) / (std + 1e-8) with the unbiased std — one workgroup per episode
//   gymrl_ppg_policy_loss_fwd_bwd  L5, the policy phase (:330-370): dual-clip surrogate, F.mse_loss value, entropy
//   gymrl_ppg_aux_loss_fwd_bwd     L6, the aux phase (:372-393): mse(v_target, aux) + beta * mse(log pi(a), old_logp)
//
// The policy is torch's Categorical(probs) over probs = softmax(logits): probs are renormalised p / sum(p) and every log is
// log(clamp(p, eps, 1 - eps)) with eps = FLT_EPSILON (log_prob and entropy alike; clamped_policy_device.hpp, shared with
// the acting step gymrl_mlprnn_act).  clamp passes the gradient on its closed
// interval and blocks it outside, so a saturated probability gets no gradient through its log (a log-softmax form would).
// torch.min / torch.max ties split the gradient in half, as in the L1 kernel (policy_device.hpp ppo_loss_row).
// A minibatch of G episodes has loss = mean over episodes of each episode's mean: at G = 1 the reference's loss exactly.
//
// Segment offsets are host arrays (validated before any HIP call) and reach the kernels by value, 255 segments per launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gymrl.h"
#include "clamped_policy_device.hpp"

using namespace gymrl;

namespace {

constexpr int kBlock = 256;
constexpr int kSegs = 255;                  // segments per launch (2 KB of offsets by value)
constexpr int kChunk = 2048;                // GAE steps staged in LDS at a time

struct SegOffsets {
  int64_t off[kSegs + 1];
};

__device__ __forceinline__ double block_sum(double v, double* sm) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  v = wave_sum(v);
  __syncthreads();                          // sm may still be read by the previous call
  if (lane == 0) sm[wid] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) s += sm[w];
  return s;
}

// ------------------------------------------------------------ episode GAE ---
__global__ __launch_bounds__(kBlock) void episode_gae_kernel(const float* __restrict__ rew, const float* __restrict__ val,
                                                             const float* __restrict__ next_val, const uint8_t* __restrict__ done,
                                                             const uint8_t* __restrict__ dw, SegOffsets S, float gamma, float gl,
                                                             float* __restrict__ adv_raw, float* __restrict__ adv_norm,
                                                             float* __restrict__ v_target, double* __restrict__ ep_moments,
                                                             int seg0) {
  __shared__ float sd[kChunk];
  __shared__ float sm_keep[kChunk];
  __shared__ double red[kBlock / 64];
  const int e = blockIdx.x;
  const int64_t a = S.off[e], n = S.off[e + 1] - a;
  float carry = 0.0f;
  double s1 = 0.0;
  // backwards over chunks of the episode: deltas in parallel, the recursion on one lane, the writes in parallel
  for (int64_t c1 = n; c1 > 0; c1 -= kChunk) {
    const int64_t c0 = c1 > kChunk ? c1 - kChunk : 0;
    const int m = (int)(c1 - c0);
    for (int i = threadIdx.x; i < m; i += kBlock) {
      const int64_t o = a + c0 + i;
      sd[i] = (rew[o] + (gamma * next_val[o]) * (1.0f - (float)(dw[o] != 0))) - val[o];
      sm_keep[i] = 1.0f - (float)(done[o] != 0);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float g = carry;
      for (int i = m - 1; i >= 0; --i) {
        g = (gl * g) * sm_keep[i] + sd[i];
        sd[i] = g;
      }
      carry = g;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < m; i += kBlock) {
      const int64_t o = a + c0 + i;
      const float g = sd[i];
      if (adv_raw) adv_raw[o] = g;
      v_target[o] = g + val[o];
      adv_norm[o] = g;
      s1 += (double)g;
    }
    __syncthreads();
  }
  const double mean = block_sum(s1, red) / (double)n;
  double s2 = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) {
    const double d = (double)adv_norm[a + i] - mean;
    s2 += d * d;
  }
  const double var = block_sum(s2, red) / (double)(n - 1);     // n == 1: 0 / 0 = NaN, as torch's unbiased std
  const double sd64 = sqrt(var);
  const float mf = (float)mean, den = (float)sd64 + 1e-8f;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) adv_norm[a + i] = (adv_norm[a + i] - mf) / den;
  if (ep_moments && threadIdx.x == 0) { ep_moments[2 * (seg0 + e)] = mean; ep_moments[2 * (seg0 + e) + 1] = sd64; }
}

// ------------------------------------------------------------ L5 / L6 -------
struct LossCfg {
  float clip, dual_clip, val_coef, ent_coef, beta;
  float inv_G;
};

// gradients wrt (L, p2 directly) -> wrt the logits; the forward half is clamped_policy (clamped_policy_device.hpp)
template <int A>
__device__ __forceinline__ void clamped_policy_bwd(const float (&p)[A], float S, const float (&c)[A], const bool (&inb)[A],
                                                   const float (&gL)[A], const float (&gp2d)[A], float (&gz)[A]) {
  float gp2[A], gp[A];
  float gS = 0.0f;
#pragma unroll
  for (int k = 0; k < A; ++k) {
    gp2[k] = gp2d[k] + (inb[k] ? gL[k] / c[k] : 0.0f);
    gS -= gp2[k] * p[k] / (S * S);
  }
  float dot = 0.0f;
#pragma unroll
  for (int k = 0; k < A; ++k) { gp[k] = gp2[k] / S + gS; dot += gp[k] * p[k]; }
#pragma unroll
  for (int k = 0; k < A; ++k) gz[k] = p[k] * (gp[k] - dot);
}

// per episode: AUX == false -> metrics_ep[e][5] = (total, clip_loss, value_loss, entropy_loss, adv mean)
//              AUX == true  -> metrics_ep[e][3] = (aux_value_loss, clone_loss, joint)
template <int A, bool AUX>
__global__ __launch_bounds__(kBlock) void ppg_loss_kernel(const float* __restrict__ logits, const float* __restrict__ value,
                                                          const int32_t* __restrict__ act, const float* __restrict__ old_logp,
                                                          const float* __restrict__ adv, const float* __restrict__ v_target,
                                                          SegOffsets S, LossCfg cfg, float* __restrict__ dlogits,
                                                          float* __restrict__ dvalue, double* __restrict__ metrics_ep, int seg0) {
  __shared__ double red[kBlock / 64];
  const int e = blockIdx.x;
  const int64_t a0 = S.off[e], n = S.off[e + 1] - a0;
  const float w = cfg.inv_G / (float)n;
  double m0 = 0.0, m1 = 0.0, m2 = 0.0;
  for (int64_t i = a0 + threadIdx.x; i < a0 + n; i += kBlock) {
    float z[A], p[A], p2[A], L[A], c[A], gL[A], gp2d[A], gz[A];
    bool inb[A];
    float Ssum;
#pragma unroll
    for (int k = 0; k < A; ++k) z[k] = logits[i * A + k];
    clamped_policy<A>(z, p, Ssum, p2, L, c, inb);
    const int ac = act[i];
    // an action outside [0, A) (torch's gather would raise) makes its log-prob NaN, so the loss, the metrics and every
    // gradient of the episode turn NaN instead of training quietly on L[0]
    float lp = __builtin_nanf("");
#pragma unroll
    for (int k = 0; k < A; ++k) if (ac == k) lp = L[k];
    const float lpo = old_logp[i], vt = v_target[i], v = value[i];
    if (!AUX) {
      const float ad = adv[i];
      const float lo = 1.0f - cfg.clip, hi = 1.0f + cfg.clip;
      const float ratio = det_expf(lp - lpo);
      const float s1 = ratio * ad;
      const float s2 = fminf(fmaxf(ratio, lo), hi) * ad;
      const float inr = (ratio >= lo && ratio <= hi) ? 1.0f : 0.0f;  // clamp passes grad on [lo, hi]
      const float w1 = s1 < s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);      // torch.min tie: 1/2, 1/2
      const float ms = fminf(s1, s2);
      float dms_dr = w1 * ad + (1.0f - w1) * ad * inr;
      float obj = ms;
      if (ad < 0.0f) {                                                // torch.where(adv < 0, max(min_surr, dual * adv), min_surr)
        const float dc = cfg.dual_clip * ad;
        obj = fmaxf(ms, dc);
        const float wm = ms > dc ? 1.0f : (ms == dc ? 0.5f : 0.0f);    // torch.max tie
        dms_dr *= wm;
      }
      const float g_lp = -w * dms_dr * ratio;
      float H = 0.0f;
#pragma unroll
      for (int k = 0; k < A; ++k) H -= L[k] * p2[k];
#pragma unroll
      for (int k = 0; k < A; ++k) {
        gL[k] = (ac == k ? g_lp : 0.0f) + cfg.ent_coef * w * p2[k];     // entropy_loss = -mean H: dH/dL_k = -p2_k
        gp2d[k] = cfg.ent_coef * w * L[k];                             //                         dH/dp2_k = -L_k
      }
      const float dv = v - vt;
      dvalue[i] = cfg.val_coef * w * 2.0f * dv;
      m0 += (double)obj; m1 += (double)dv * (double)dv; m2 += (double)H;
    } else {
      const float dl = lp - lpo;
#pragma unroll
      for (int k = 0; k < A; ++k) { gL[k] = ac == k ? cfg.beta * w * 2.0f * dl : 0.0f; gp2d[k] = 0.0f; }
      const float dv = v - vt;
      dvalue[i] = w * 2.0f * dv;
      m0 += (double)dv * (double)dv; m1 += (double)dl * (double)dl;
    }
    clamped_policy_bwd<A>(p, Ssum, c, inb, gL, gp2d, gz);
#pragma unroll
    for (int k = 0; k < A; ++k) dlogits[i * A + k] = gz[k];
  }
  const double dn = (double)n;
  if (!AUX) {
    double sa = 0.0;
    for (int64_t i = a0 + threadIdx.x; i < a0 + n; i += kBlock) sa += (double)adv[i];
    const double obj = block_sum(m0, red) / dn, vl = block_sum(m1, red) / dn, H = block_sum(m2, red) / dn;
    const double am = block_sum(sa, red) / dn;
    if (threadIdx.x == 0) {
      double* o = metrics_ep + (size_t)(seg0 + e) * 5;
      const double clip_loss = -obj, ent_loss = -H;
      o[0] = clip_loss + (double)cfg.val_coef * vl + (double)cfg.ent_coef * ent_loss;
      o[1] = clip_loss; o[2] = vl; o[3] = ent_loss; o[4] = am;
    }
  } else {
    const double al = block_sum(m0, red) / dn, cl = block_sum(m1, red) / dn;
    if (threadIdx.x == 0) {
      double* o = metrics_ep + (size_t)(seg0 + e) * 3;
      o[0] = al; o[1] = cl; o[2] = al + (double)cfg.beta * cl;
    }
  }
}

// metrics_sum[k] += mean over the G episodes of metrics_ep[.][k], in episode order
__global__ void metrics_mean_kernel(const double* __restrict__ metrics_ep, int G, int K, double* __restrict__ metrics_sum) {
  const int k = threadIdx.x;
  if (k >= K) return;
  double s = 0.0;
  for (int e = 0; e < G; ++e) s += metrics_ep[(size_t)e * K + k];
  metrics_sum[k] += s / (double)G;
}

inline bool offsets_ok(const int64_t* off, int E, bool allow_empty) {
  if (!off || E < 0 || off[0] != 0) return false;
  for (int e = 0; e < E; ++e) {
    const int64_t n = off[e + 1] - off[e];
    if (n < 0 || (n == 0 && !allow_empty) || off[e + 1] > ((int64_t)1 << 40)) return false;
  }
  return true;
}

template <typename F>
int for_each_chunk(const int64_t* off, int E, F launch) {
  for (int s0 = 0; s0 < E; s0 += kSegs) {
    const int ns = E - s0 < kSegs ? E - s0 : kSegs;
    SegOffsets S;
    for (int i = 0; i <= ns; ++i) S.off[i] = off[s0 + i];
    launch(S, s0, ns);
    GYMRL_CHECK_LAUNCH();
  }
  return 0;
}

template <bool AUX>
int ppg_loss(const float* logits, const float* value, const int32_t* act, const float* old_logp, const float* adv,
             const float* v_target, const int64_t* offsets, int G, int A, const LossCfg& cfg0, float* dlogits, float* dvalue,
             double* metrics_ep, double* metrics_sum, void* stream) {
  if (!logits || !value || !act || !old_logp || (!AUX && !adv) || !v_target || !dlogits || !dvalue || !metrics_ep) return -22;
  if (G <= 0 || A < 2 || A > 8 || !offsets_ok(offsets, G, false)) return -22;
  LossCfg cfg = cfg0;
  cfg.inv_G = 1.0f / (float)G;
  hipStream_t s = (hipStream_t)stream;
  int rc = for_each_chunk(offsets, G, [&](const SegOffsets& S, int s0, int ns) {
    switch (A) {
#define PPG_CASE(AA) \
  case AA: hipLaunchKernelGGL((ppg_loss_kernel<AA, AUX>), dim3(ns), dim3(kBlock), 0, s, logits, value, act, old_logp, adv, v_target, S, cfg, dlogits, dvalue, metrics_ep, s0); break;
      PPG_CASE(2) PPG_CASE(3) PPG_CASE(4) PPG_CASE(5) PPG_CASE(6) PPG_CASE(7) PPG_CASE(8)
#undef PPG_CASE
    }
  });
  if (rc) return rc;
  if (metrics_sum) {
    hipLaunchKernelGGL(metrics_mean_kernel, dim3(1), dim3(64), 0, s, metrics_ep, G, AUX ? 3 : 5, metrics_sum);
    GYMRL_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" {

int gymrl_episode_gae(const float* rew, const float* val, const float* next_val, const uint8_t* done, const uint8_t* dw,
                      const int64_t* offsets, int E, double gamma, double lam, float* adv_raw, float* adv_norm,
                      float* v_target, double* ep_moments, void* stream) {
  if (!rew || !val || !next_val || !done || !dw || !adv_norm || !v_target) return -22;
  if (E < 0 || !offsets_ok(offsets, E, false)) return -22;
  hipStream_t s = (hipStream_t)stream;
  return for_each_chunk(offsets, E, [&](const SegOffsets& S, int s0, int ns) {
    hipLaunchKernelGGL(episode_gae_kernel, dim3(ns), dim3(kBlock), 0, s, rew, val, next_val, done, dw, S, (float)gamma,
                       (float)(gamma * lam), adv_raw, adv_norm, v_target, ep_moments, s0);
  });
}

int gymrl_ppg_policy_loss_fwd_bwd(const float* logits, const float* value, const int32_t* act, const float* old_logp,
                                  const float* adv, const float* v_target, const int64_t* offsets, int G, int A, float clip,
                                  float dual_clip, float val_coef, float ent_coef, float* dlogits, float* dvalue,
                                  double* metrics_ep, double* metrics_sum, void* stream) {
  const LossCfg cfg{clip, dual_clip, val_coef, ent_coef, 0.0f, 0.0f};
  return ppg_loss<false>(logits, value, act, old_logp, adv, v_target, offsets, G, A, cfg, dlogits, dvalue, metrics_ep,
                         metrics_sum, stream);
}

int gymrl_ppg_aux_loss_fwd_bwd(const float* logits, const float* aux_value, const int32_t* act, const float* old_logp,
                               const float* v_target, const int64_t* offsets, int G, int A, float beta, float* dlogits,
                               float* d_aux, double* metrics_ep, double* metrics_sum, void* stream) {
  const LossCfg cfg{0.0f, 0.0f, 0.0f, 0.0f, beta, 0.0f};
  return ppg_loss<true>(logits, aux_value, act, old_logp, nullptr, v_target, offsets, G, A, cfg, dlogits, d_aux, metrics_ep,
                        metrics_sum, stream);
}

}  // extern "C"
