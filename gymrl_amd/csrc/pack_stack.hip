// pack_stack.hip — P policies x L layers into the one-launch forward's weight layout in ONE launch (gfx950).
//
// gymrl_mlp_pack (mlp.hip) writes one weight's MFMA B-operand image per launch; a population of flat parameter vectors needed
// one such launch and one bias copy per layer and policy.  Here blockIdx.y is the policy and a thread of the row is one float4 of
// the packed row: the 2 L ranges of a row (L images, then L padded biases) are numbered back to back in float4s, a thread finds
// its range by a scan over the table in the kernel arguments and then does exactly what mlp_pack_kernel does for that float4 (or
// copies four bias floats).  Copies and zeros only: the bits are gymrl_mlp_pack's.
//
// The weight reads are strided by in_dim across the 16 low lanes, as in mlp_pack_kernel (not staged through LDS: the image is
// written once and read 4 bytes wide either way; the stores are one coalesced 16-byte store per lane).  No LDS, no atomics, no
// workgroup waits for another.
#include "mlp_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::mlp;

struct PackRange {
  int out_dim, in_dim;   // bias ranges: in_dim == 0
  int nkb;               // K-blocks of the image (K rounded up to 64, / 16)
  unsigned begin;        // first float4 of the range in the row's numbering
  long long src, dst;    // floats into a params row / into a packed row
};
struct PackTable {
  int n_ranges;          // 2 L: the images, then the biases
  unsigned total;        // float4s of a row
  PackRange r[2 * GYMRL_MLP_MAX_STAGES];
};

__global__ __launch_bounds__(256) void mlp_pack_stack_kernel(const float* __restrict__ params, long long params_stride,
                                                             float* __restrict__ packed, long long packed_stride,
                                                             PackTable t) {
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= t.total) return;
  int k = 0;
  for (int i = 1; i < t.n_ranges; ++i) k = idx >= t.r[i].begin ? i : k;       // the ranges ascend in `begin`
  const PackRange g = t.r[k];
  const unsigned local = idx - g.begin;
  const float* src = params + (size_t)blockIdx.y * (size_t)params_stride + g.src;
  float* dst = packed + (size_t)blockIdx.y * (size_t)packed_stride + g.dst;
  f32x4 v;
  if (g.in_dim) {          // P[tile][kblock][lane][c] <- W, mlp_pack_kernel's expression
    const int lane = local & 63, kbi = (int)((local >> 6) % (unsigned)g.nkb), tile = (int)((local >> 6) / (unsigned)g.nkb);
    const int n = 16 * tile + (lane & 15), kk = 16 * kbi + 4 * (lane >> 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = (n < g.out_dim && kk + c < g.in_dim) ? src[(size_t)n * g.in_dim + kk + c] : 0.0f;
  } else {                 // the bias, zeros up to the next multiple of four
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = ((int)(4 * local) + c < g.out_dim) ? src[4 * local + c] : 0.0f;
  }
  reinterpret_cast<f32x4*>(dst)[local] = v;
}

}  // namespace

extern "C" {

size_t gymrl_mlp_pack_stack_args_bytes(void) { return sizeof(gymrl_mlp_pack_stack_args); }

int gymrl_mlp_pack_stack(const gymrl_mlp_pack_stack_args* a, void* stream) {
  if (!a || !a->params || !a->packed) return -22;
  if (a->P < 1 || a->P > 65535 || a->n_layers < 1 || a->n_layers > GYMRL_MLP_MAX_STAGES) return -22;
  if (a->packed_stride < 0 || (a->packed_stride & 3) || a->params_stride < 0) return -22;
  if ((reinterpret_cast<uintptr_t>(a->packed) & 15) || (reinterpret_cast<uintptr_t>(a->params) & 3)) return -22;
  const int L = a->n_layers;
  PackTable t;
  t.n_ranges = 2 * L;
  long long lo[2 * GYMRL_MLP_MAX_STAGES], hi[2 * GYMRL_MLP_MAX_STAGES];
  unsigned at = 0;
  for (int k = 0; k < L; ++k) {
    const gymrl_mlp_pack_layer& l = a->layer[k];
    if (l.out_dim <= 0 || l.in_dim <= 0 || l.out_dim > kMaxW || l.in_dim > kMaxW) return -22;
    if (l.w_off < 0 || l.b_off < 0 || l.w_at < 0 || l.b_at < 0 || (l.w_at & 3) || (l.b_at & 3)) return -22;
    if (l.w_off > a->params_stride - (long long)l.out_dim * l.in_dim || l.b_off > a->params_stride - l.out_dim) return -22;
    const long long image = (long long)gymrl_mlp_packed_floats(l.out_dim, l.in_dim), bias = (l.out_dim + 3) & ~3;
    if (l.w_at > a->packed_stride - image || l.b_at > a->packed_stride - bias) return -22;
    lo[k] = l.w_at, hi[k] = l.w_at + image, lo[L + k] = l.b_at, hi[L + k] = l.b_at + bias;
  }
  for (int i = 0; i < 2 * L; ++i)
    for (int j = i + 1; j < 2 * L; ++j)
      if (lo[i] < hi[j] && lo[j] < hi[i]) return -22;
  for (int k = 0; k < 2 * L; ++k) {
    const gymrl_mlp_pack_layer& l = a->layer[k < L ? k : k - L];
    PackRange& r = t.r[k];
    r.out_dim = l.out_dim, r.in_dim = k < L ? l.in_dim : 0, r.nkb = ((l.in_dim + 63) & ~63) >> 4;
    r.begin = at, r.src = k < L ? l.w_off : l.b_off, r.dst = k < L ? l.w_at : l.b_at;
    at += (unsigned)((hi[k] - lo[k]) >> 2);
  }
  t.total = at;        // <= 8 * (16 * 16 * 64 + 64) float4s
  hipLaunchKernelGGL(mlp_pack_stack_kernel, dim3((at + 255) / 256, (unsigned)a->P), dim3(256), 0, (hipStream_t)stream,
                     a->params, (long long)a->params_stride, a->packed, (long long)a->packed_stride, t);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
