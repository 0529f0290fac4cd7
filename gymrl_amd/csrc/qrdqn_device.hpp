// qrdqn_device.hpp — the arithmetic of the quantile-regression (QR-DQN, Dabney et al. 2018) value head, stated once: one
// wave64 holds the quantiles of one (row, action) pair, quantile i in lane i (1 <= N <= 64 quantiles; lanes >= N are `off` and
// hold the sums' +0).  gymrl_qr_q and gymrl_qr_loss (qrdqn.hip) both run these functions, and tests/qrdqn_ref.py restates them
// line for line.  float32 throughout, no fused operation (-ffp-contract=off like the whole library), no exp / log: every
// operation here is an IEEE +, -, *, / or a comparison, so the restatement is exact in plain numpy.
//
// Sum orders.  Two kinds of sum occur, and neither depends on the batch size or the grid:
//   * a sum over the quantiles of one row (the mean quantile of an action, the row's loss) is row_loss_device.hpp's butterfly
//     over the wave's 64 slots, slots >= N holding +0: the bits of the halving tree v[0:off] + v[off:2 off], off = 32 ... 1;
//   * the sum over the target samples j of lane i's pairwise terms is serial over j = 0 ... N - 1 ascending, starting from +0,
//     one accumulator for the loss and one for the gradient.
//
// Where the factors sit.  With u_ij = T_j - theta_i and the weight wt_ij = (u_ij < 0 ? 1 - tau_i : tau_i) = |tau_i - 1{u_ij < 0}|:
//   tau_i   = (float)(2 i + 1) / (float)(2 N)                       one division; 1 - tau_i is one subtraction
//   mean    q = wave_allsum(theta) / (float)N                       one division per (row, action)
//   H_ij    = |u| <= kappa ? (0.5f * u) * u : kappa * (|u| - 0.5f * kappa)
//   c_ij    = u > kappa ? kappa : (u < -kappa ? -kappa : u)          (a select, not fminf / fmaxf: a NaN u stays NaN)
//   l_i     = sum_j wt_ij * H_ij,   g_i = sum_j wt_ij * c_ij          nothing else inside the sums
//   lane    loss_i = (l_i / kappa) / (float)N,  dtheta_i = -((g_i / kappa) / (float)N)     1 / kappa and 1 / N ONCE PER LANE, as
//           two divisions in this order, after the serial sums
//   row     row_loss = wave_allsum(loss_i),  dquant_i = (w_b * (1.0f / (float)B)) * dtheta_i
// At u == 0 the comparison u < 0 is false and H = c = +0; at |u| == kappa the quadratic branch is taken (it equals the linear).
#pragma once
#include "gymrl_device.hpp"
#include "row_loss_device.hpp"

namespace gymrl {
namespace qr {

constexpr int kMaxQuantiles = GYMRL_WAVE;      // one quantile per lane
constexpr int kMaxActions = 8;
using rowloss::wave_allsum;

// the midpoint tau_i of the i-th of N equal slices of (0, 1)
__device__ __forceinline__ float tau(int i, int N) { return (float)(2 * i + 1) / (float)(2 * N); }

// the mean of a row of N quantiles, on every lane
__device__ __forceinline__ float mean_q(const float* __restrict__ row, int N, int lane) {
  return wave_allsum(lane < N ? row[lane] : 0.0f) / (float)N;
}

// the first maximum over the actions of the mean of rows[a][0:N]; q_out (lane 0 writes) may be nullptr
__device__ __forceinline__ int greedy_action(const float* __restrict__ rows, int A, int N, int lane,
                                             float* __restrict__ q_out) {
  int arg = 0;
  float best = 0.0f;
  for (int a = 0; a < A; ++a) {
    const float q = mean_q(rows + (size_t)a * N, N, lane);
    if (q_out && lane == 0) q_out[a] = q;
    if (a == 0 || q > best) { best = q; arg = a; }
  }
  return arg;
}

// l_i and g_i for i = this lane (theta: its quantile, tau_i: its midpoint).  sT: the row's T_j in LDS; every lane reads the
// same address, a broadcast.
__device__ __forceinline__ void pair_sums(const float* sT, int N, float theta, float tau_i, float kappa, float& l, float& g) {
  const float below = 1.0f - tau_i, half_kappa = 0.5f * kappa;
  l = 0.0f;
  g = 0.0f;
  for (int j = 0; j < N; ++j) {
    const float u = sT[j] - theta;
    const float au = fabsf(u);
    const float wt = u < 0.0f ? below : tau_i;
    const float H = au <= kappa ? (0.5f * u) * u : kappa * (au - half_kappa);
    const float c = u > kappa ? kappa : (u < -kappa ? -kappa : u);
    l += wt * H;
    g += wt * c;
  }
}

}  // namespace qr
}  // namespace gymrl
