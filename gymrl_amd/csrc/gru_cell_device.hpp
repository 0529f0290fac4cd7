// gru_cell_device.hpp — the pointwise half of torch.nn.GRU's cell, shared by the per-step cell kernels
// (recurrent.hip) and the one-launch sequence kernels (gru_seq.hip) so that both produce the same bits.
//
// Gate order and formulas are PyTorch's:  r = s(gi_r + gh_r), z = s(gi_z + gh_z),
// n = tanh(gi_n + r * gh_n), h' = (1 - z) * n + z * h, with s(x) = 1 / (1 + exp(-x)) on the
// reproducible det_expf.  Every translation unit is built with -ffp-contract=off, so the expressions below
// are evaluated exactly as written wherever they are inlined.
#pragma once
#include "gymrl_device.hpp"

namespace gymrl {

__device__ __forceinline__ float det_sigmoidf(float x) { return 1.0f / (1.0f + det_expf(-x)); }

__device__ __forceinline__ float gru_point_fwd(float ir, float iz, float in, float hr, float hz, float hn, float hp) {
  const float r = det_sigmoidf(ir + hr);
  const float z = det_sigmoidf(iz + hz);
  const float n = det_tanhf_sel(in + r * hn);
  return (1.0f - z) * n + z * hp;
}

// gates recomputed from (gi, gh); go = dL/dh'.  dgi = (dir, diz, din), dgh = (dir, diz, dhn), direct dh = dhp.
__device__ __forceinline__ void gru_point_bwd(float ir, float iz, float in, float hr, float hz, float hn, float hp, float go,
                                              float& dir, float& diz, float& din, float& dhn, float& dhp) {
  const float r = det_sigmoidf(ir + hr);
  const float z = det_sigmoidf(iz + hz);
  const float n = det_tanhf_sel(in + r * hn);
  const float dn = go * (1.0f - z);
  const float dz = go * (hp - n);
  const float dnp = dn * (1.0f - n * n);
  din = dnp;
  dhn = dnp * r;
  dir = (dnp * hn) * (r * (1.0f - r));
  diz = dz * (z * (1.0f - z));
  dhp = go * z;
}

}  // namespace gymrl
