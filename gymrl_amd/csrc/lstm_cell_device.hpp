// lstm_cell_device.hpp — the pointwise half of torch.nn.LSTM's cell, shared by the per-step cell kernels and the
// one-launch sequence kernels (both in lstm_seq.hip) so that both produce the same bits.  tests/lstm_ref.py restates
// this file line by line in numpy float32.
//
// Gate order and formulas are PyTorch's (i, f, g, o), on a = gi + gh:
//   i = s(a_i), f = s(a_f), g = tanh(a_g), o = s(a_o), c' = f * c + i * g, h' = o * tanh(c'),
// with s(x) = 1 / (1 + exp(-x)) on the reproducible det_expf and tanh = det_tanhf_sel, as in gru_cell_device.hpp.
// Every translation unit is built with -ffp-contract=off, so the expressions below are evaluated exactly as written
// wherever they are inlined.
#pragma once
#include "gru_cell_device.hpp"

namespace gymrl {

struct LstmGates {
  float i, f, g, o;
};

__device__ __forceinline__ LstmGates lstm_gates(float ii, float fi, float gi, float oi, float ih, float fh, float gh, float oh) {
  LstmGates k;
  k.i = det_sigmoidf(ii + ih);
  k.f = det_sigmoidf(fi + fh);
  k.g = det_tanhf_sel(gi + gh);
  k.o = det_sigmoidf(oi + oh);
  return k;
}

// (gi_i, gi_f, gi_g, gi_o), (gh_i, gh_f, gh_g, gh_o), c -> h', c'
__device__ __forceinline__ void lstm_point_fwd(float ii, float fi, float gi, float oi, float ih, float fh, float gh, float oh,
                                               float c, float& h_new, float& c_new) {
  const LstmGates k = lstm_gates(ii, fi, gi, oi, ih, fh, gh, oh);
  c_new = (k.f * c) + (k.i * k.g);
  h_new = k.o * det_tanhf_sel(c_new);
}

// Gates recomputed from (gi, gh, c); dh = dL/dh', dcn = dL/dc'.  Since a = gi + gh, (di, df, dg, do_) is both dgi and dgh;
// dcp = dL/dc through the cell state (the path through h_{t-1} is the caller's dgates . W_hh).
__device__ __forceinline__ void lstm_point_bwd(float ii, float fi, float gi, float oi, float ih, float fh, float gh, float oh,
                                               float c, float dh, float dcn, float& di, float& df, float& dg, float& do_,
                                               float& dcp) {
  const LstmGates k = lstm_gates(ii, fi, gi, oi, ih, fh, gh, oh);
  const float cn = (k.f * c) + (k.i * k.g);
  const float tc = det_tanhf_sel(cn);
  do_ = (dh * tc) * (k.o * (1.0f - k.o));
  const float dc = dcn + ((dh * k.o) * (1.0f - (tc * tc)));
  di = (dc * k.g) * (k.i * (1.0f - k.i));
  df = (dc * c) * (k.f * (1.0f - k.f));
  dg = (dc * k.i) * (1.0f - (k.g * k.g));
  dcp = dc * k.f;
}

}  // namespace gymrl
