// duel_device.hpp — the dueling combination q = v + (a - mean a) and its backward, in the order torch evaluates them on the
// device.  Shared by the row-slab kernels of the dueling networks (ddqn_step.hip, noisy_dqn_step.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace gymrl {
namespace slab {
namespace {

// q = value + (advantage - advantage.mean(dim=-1, keepdim=True)) as torch evaluates it on the device: the mean is the float32
// sum of the row times the float32 reciprocal 1 / A (the reduction's `acc * factor`), then one subtraction and one addition
// per element.  With A = 2 — the only width the entry points take — the sum has one addition and 1 / A is exact.
__device__ __forceinline__ void duel_combine(const float* adv, float v, int A, float* q) {
  float sum = adv[0];
  for (int k = 1; k < A; ++k) sum += adv[k];
  const float m = sum * (1.0f / (float)A);
  for (int k = 0; k < A; ++k) q[k] = v + (adv[k] - m);
}
// Its backward in autograd's order, for the gradient dq of q: the broadcast value takes the row sum, dv = sum_k dq[k]; the
// subtraction hands dq to the advantage and -dq to the broadcast mean, whose gradient is the row sum gm = sum_k (-dq[k]); the
// mean spreads gm * (1 / A) over the row (a division by the host scalar A runs as a multiplication by its reciprocal); the two
// gradients of the advantage are then added: da[k] = dq[k] + gm * (1 / A).
__device__ __forceinline__ void duel_combine_bwd(const float* dq, int A, float* da, float& dv) {
  float sv = dq[0], gm = -dq[0];
  for (int k = 1; k < A; ++k) { sv += dq[k]; gm += -dq[k]; }
  const float spread = gm * (1.0f / (float)A);
  for (int k = 0; k < A; ++k) da[k] = dq[k] + spread;
  dv = sv;
}

}  // namespace
}  // namespace slab
}  // namespace gymrl
