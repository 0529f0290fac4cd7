// c51_device.hpp — the arithmetic of the categorical (C51) value head, stated once: one wave64 holds the atoms of one
// (row, action) pair, atom j in lane j (2 <= M <= 64 atoms; lanes >= M are `off` and hold the sums' +0).  gymrl_c51_q and
// gymrl_c51_loss (c51.hip) both run these functions, and tests/c51_ref.py restates them line for line.  float32 throughout,
// no fused operation (-ffp-contract=off like the whole library), exp / log are the reproducible det_* forms.
//
// Sum orders.  Two kinds of sum occur, and neither depends on the batch size or the grid:
//   * a sum over the atoms of one row (the softmax denominator, the expected value, the cross-entropy) is the butterfly over
//     the wave's 64 slots, slots >= M holding +0: v_l <- v_l + v_(l ^ 32), then ^ 16, 8, 4, 2, 1.  Every lane ends with the
//     same bits (each level adds the same two values in either order), which are those of the halving tree
//     v[0:off] + v[off:2 off] for off = 32 ... 1 read at slot 0;
//   * the projection m_i = sum_j p*_j max(0, 1 - |b_j - i|) is a serial sum over j = 0 ... M - 1 ascending, starting from +0.
#pragma once
#include "gymrl_device.hpp"
#include "row_loss_device.hpp"
#include "softmax_device.hpp"

namespace gymrl {
namespace c51 {

constexpr int kMaxAtoms = GYMRL_WAVE;          // one atom per lane
constexpr int kMaxActions = kSoftmaxMaxA;      // 8

using rowloss::wave_allsum;                    // the butterfly of the header above
__device__ __forceinline__ float wave_allmax(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// atom j of the support: z_j = vmin + j * dz, dz = (vmax - vmin) / (M - 1)
__device__ __forceinline__ float atom(float vmin, float dz, int j) { return vmin + (float)j * dz; }

// The softmax over one row's atoms in softmax_device.hpp's form.  x: this lane's logit (anything on an off lane).
// d = x - max_j x_j, e = det_expf(d) (+0 on an off lane), s = sum_j e_j on every lane.
__device__ __forceinline__ void softmax_lane(float x, bool on, float& d, float& e, float& s) {
  const float mx = wave_allmax(on ? x : -__builtin_inff());
  d = x - mx;
  e = on ? det_expf(d) : 0.0f;
  s = wave_allsum(e);
}

// this lane's probability of a row of M logits (+0 on an off lane)
__device__ __forceinline__ float prob_lane(const float* __restrict__ row, int M, int lane) {
  const bool on = lane < M;
  float d, e, s;
  softmax_lane(on ? row[lane] : 0.0f, on, d, e, s);
  return e / s;
}

// q = sum_j p_j z_j of a row of M logits, on every lane; z: this lane's atom
__device__ __forceinline__ float expected_q(const float* __restrict__ row, int M, int lane, float z) {
  const float p = prob_lane(row, M, lane);
  return wave_allsum(lane < M ? p * z : 0.0f);
}

// the first maximum over the actions of the expected value of rows[a][0:M]; q_out (lane 0 writes) may be nullptr
__device__ __forceinline__ int greedy_action(const float* __restrict__ rows, int A, int M, int lane, float z,
                                             float* __restrict__ q_out) {
  int arg = 0;
  float best = 0.0f;
  for (int a = 0; a < A; ++a) {
    const float q = expected_q(rows + (size_t)a * M, M, lane, z);
    if (q_out && lane == 0) q_out[a] = q;
    if (a == 0 || q > best) { best = q; arg = a; }
  }
  return arg;
}

// where atom z of the target net's support lands after the Bellman map, in units of dz from vmin:
// b = (clamp(rew + g z, vmin, vmax) - vmin) / dz, g = gamma_n (1 - flag)
__device__ __forceinline__ float project_pos(float rew, float g, float z, float vmin, float vmax, float dz) {
  const float tz = fminf(fmaxf(rew + g * z, vmin), vmax);
  return (tz - vmin) / dz;
}

// m_i for i = this lane: the gather form of the floor / ceil scatter.  sp / sb: the row's p*_j and b_j in LDS (every lane reads
// the same address: a broadcast).  A b_j that is an integer gives weight 1 to that atom and 0 to its neighbours.
__device__ __forceinline__ float project_mass(const float* sp, const float* sb, int M, int lane) {
  const float fi = (float)lane;
  float m = 0.0f;
  for (int j = 0; j < M; ++j) m += sp[j] * fmaxf(0.0f, 1.0f - fabsf(sb[j] - fi));
  return m;
}

}  // namespace c51
}  // namespace gymrl
