// duel_device.hpp — the dueling combination q = v + (a - mean a) and its backward, in the order torch evaluates them on the
// device, and as Rainbow's layer path does.  Shared by the row-slab kernels of the dueling networks (ddqn_step.hip,
// noisy_dqn_step.hip, rainbow_step.hip) and by the episode kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace gymrl {
namespace slab {
namespace {

// q = value + (advantage - advantage.mean(dim=-1, keepdim=True)) as torch evaluates it on the device: the mean is the float32
// sum of the row times the float32 reciprocal 1 / A (the reduction's `acc * factor`), then one subtraction and one addition
// per element.  With A = 2 — the width of the fused steps and of gymrl_classic_duel_eval — the sum has one addition and 1 / A is
// exact.  With A = 3 (gymrl_mountaincar_net_eval, net 1) the order of the two additions counts, and it is NOT left to right:
// torch's reduction deals a row of three to last_pow2(3) = 2 threads — thread 0 adds a0 + a2, thread 1 holds a1 — and adds the
// two partials, (a0 + a2) + a1.  Measured on the device against the three possible orders, times 1 / 3 and divided by 3, on rows
// [N, 3] for N from 1 to 4096: this one alone matched every row.  Other widths keep the plain left-to-right sum;
// only A = 2 and A = 3 are pinned by a test.
__device__ __forceinline__ void duel_combine(const float* adv, float v, int A, float* q) {
  float sum = adv[0];
  if (A == 3) sum = (adv[0] + adv[2]) + adv[1];
  else for (int k = 1; k < A; ++k) sum += adv[k];
  const float m = sum * (1.0f / (float)A);
  for (int k = 0; k < A; ++k) q[k] = v + (adv[k] - m);
}
// The same combination as Rainbow's layer path evaluates it (lin.hip lin_fwd_kernel's GYMRL_ACT_DUELING epilogue) on one row of
// the stacked head: z[0 .. A-1] = advantage stream, z[A] = value stream -> q[k] = value + (z[k] - sum / A); returns the greedy
// action (first index of the maximum).  The epilogue sums the advantages with a 16-lane butterfly over zero-padded lanes:
// ((z0 + z1) + (z2 + 0)) for A <= 3, and DIVIDES by A — from three actions on not duel_combine's float.  Shared by
// rainbow_step.hip and the episode kernels (eval_kernels_device.hpp).
__device__ __forceinline__ int dueling_row(const float* z, int A, float* q) {
  const float z0 = z[0], z1 = A > 1 ? z[1] : 0.0f, z2 = A > 2 ? z[2] : 0.0f;
  const float sum = (z0 + z1) + (z2 + 0.0f);
  const float v = z[A];
  int bi = 0;
  float best = 0.0f;
  for (int k = 0; k < A; ++k) {
    const float qv = v + (z[k] - sum / (float)A);
    q[k] = qv;
    if (k == 0 || qv > best) { best = qv; bi = k; }
  }
  return bi;
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
