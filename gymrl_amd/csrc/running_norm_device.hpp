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

}  // namespace gymrl
