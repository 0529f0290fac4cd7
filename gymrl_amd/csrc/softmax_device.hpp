// softmax_device.hpp — the softmax over a row of at most kSoftmaxMaxA action logits and its backward, stated once.
//
// Discrete SAC's actor ends in a softmax (sac_cartpole.py:70-80).  torch's F.softmax and autograd's softmax backward own
// their bits; a kernel cannot promise them.  These two functions are what gymrl_softmax_rows_fwd / _bwd (ops.softmax_rows)
// and the fused discrete-SAC step (dsac_step.hip) both run, so the layer path with Config.kernel_softmax and the fused path
// produce the same bits.  float32 throughout, every sum in ascending action order, -ffp-contract=off like the whole library:
//   forward   e_k = det_expf(z_k - max_j z_j),  p_k = e_k / sum_j e_j
//   backward  dz_k = p_k * (g_k - sum_j g_j p_j)
#pragma once
#include "gymrl_device.hpp"

namespace gymrl {

constexpr int kSoftmaxMaxA = 8;

// z, p: A elements `stride` floats apart (rows of an LDS slab or of a [B][A] array alike)
__device__ __forceinline__ void softmax_row_fwd(const float* z, int A, float* p, int stride = 1) {
  float e[kSoftmaxMaxA];
  float m = z[0];
#pragma unroll
  for (int k = 1; k < kSoftmaxMaxA; ++k) if (k < A) m = fmaxf(m, z[k * stride]);
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < kSoftmaxMaxA; ++k) if (k < A) { e[k] = det_expf(z[k * stride] - m); s += e[k]; }
#pragma unroll
  for (int k = 0; k < kSoftmaxMaxA; ++k) if (k < A) p[k * stride] = e[k] / s;
}

__device__ __forceinline__ void softmax_row_bwd(const float* p, const float* g, int A, float* dz, int stride = 1) {
  float dot = 0.0f;
#pragma unroll
  for (int k = 0; k < kSoftmaxMaxA; ++k) if (k < A) dot += g[k * stride] * p[k * stride];
#pragma unroll
  for (int k = 0; k < kSoftmaxMaxA; ++k) if (k < A) dz[k * stride] = p[k * stride] * (g[k * stride] - dot);
}

}  // namespace gymrl
