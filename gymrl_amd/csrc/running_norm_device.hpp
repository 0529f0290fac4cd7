// running_norm_device.hpp — the normalisation point of utils/normalization.py:33, y = (x - mean) / (std + 1e-8), stated once:
// running_norm_kernel (offpolicy.hip) and the one-launch recurrent evaluation (eval_lunar_rnn.hip) call it, so an observation
// normalised inside an episode kernel has the bits gymrl_running_norm_masked(update = 0) gives it.
//
// stats is RunningMeanStd.stats for D features: f64 [n, -, mean[D], S[D], std[D]].  The mean is kept in float32 (the
// reference's float32 update), the subtraction is float32, the division float64.
#pragma once
#include <hip/hip_runtime.h>

namespace gymrl {

__device__ __forceinline__ float running_norm_mean(const double* __restrict__ stats, int k) { return (float)stats[2 + k]; }
__device__ __forceinline__ double running_norm_std(const double* __restrict__ stats, int D, int k) { return stats[2 + 2 * D + k]; }

__device__ __forceinline__ float running_norm_point(float x, float mean, double std) {
  return (float)((double)(x - mean) / (std + 1e-8));
}

// RunningMeanStd.update (utils/normalization.py:13-21) for one value of one feature, stated once: running_norm_kernel and
// reward_scaling_kernel (offpolicy.hip) and the one-launch recurrent collection (collect_lunar_rnn.hip) call it, one value after
// the other in row order.  float32 mean, the float32 product accumulated into the float64 S, population std, the n == 1 quirk.
__device__ __forceinline__ void running_norm_update(float xv, double& n, float& mean, double& S, double& std) {
  n += 1.0;
  if (n == 1.0) { mean = xv; std = (double)xv; }                          // :15-17
  else {
    const float old_mean = mean;
    mean = old_mean + (xv - old_mean) / (float)n;                         // float32 mean (:19)
    S = S + (double)((xv - old_mean) * (xv - mean));                      // f32 product into f64 S (:20)
    std = sqrt(S / n);                                                    // :21
  }
}

// RewardScaling.__call__ (:44-49) for one reward: R = gamma R + r, the statistics take float32(R), -> r / (std + 1e-8)
__device__ __forceinline__ float reward_scaling_step(float r, double gamma, double& R, double& n, float& mean, double& S,
                                                     double& std) {
  const double rv = (double)r;
  R = gamma * R + rv;                                                     // :46
  running_norm_update((float)R, n, mean, S, std);                         // update() casts to float32 (:13)
  return (float)(rv / (std + 1e-8));                                      // :48
}

}  // namespace gymrl
