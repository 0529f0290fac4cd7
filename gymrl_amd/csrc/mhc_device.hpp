// mhc_device.hpp — what mhc.hip, mhc_layers.hip, mhc_norm.hip and (through mhc_policy_device.hpp) rollout_lunar.hip share: the
// transcendental helpers, the lane exchanges, the GATE ARITHMETIC of a hyper-connection — forward (sinkhorn_sweeps, row_gates) and
// the backward's row phase (row_gates_bwd), stated once for the per-layer, sub-block and rollout paths — and the parameter
// gradients' partial vectors with their two reductions (add_wave_partials inside a workgroup, partial_reduce_kernel across them).
// All __forceinline__ device code or inline host code in an anonymous namespace: file-local in every unit, nothing exported.
#pragma once
#include "train_device.hpp"

namespace gymrl {
namespace mhc {
namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kWaves = 4;

// exp and 1/x on the hardware units (v_exp_f32, v_rcp_f32: 1 ulp each).  The gate arithmetic and the SiLUs are what these kernels
// issue most — a correctly rounded division is ~12 instructions, libm's expf ~15 — and every result is held to 1e-5 of the
// float64 modules, not to torch's bits.  exp_: x log2(e) in two pieces, so that the product's rounding (up to |x| 2^-24 relative
// in the result) is folded back in.
__device__ __forceinline__ float rcp_(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float exp_(float x) {
  const float t = x * 1.44269504088896341f;
  const float lo = fmaf(x, 1.44269504088896341f, -t) + x * 1.92596299112661746e-8f;
  return __builtin_amdgcn_exp2f(t) * (1.0f + lo * 0.693147180559945309f);
}
__device__ __forceinline__ float sigmoidf_(float x) { return rcp_(1.0f + exp_(-x)); }
__device__ __forceinline__ float silu_(float z) { return z * sigmoidf_(z); }
__device__ __forceinline__ float silu_grad_(float z) { const float s = sigmoidf_(z); return s * (1.0f + z * (1.0f - s)); }

// sum over the 16 lanes of a DPP row, every lane ending with the same bits: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror,
// row_mirror — four v_add_f32_dpp, no LDS traffic (a 64-lane __shfl_xor tree is six ds_bpermute round trips)
__device__ __forceinline__ float row16_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));
  return v;
}
// lane k's v for a uniform k (v_readlane -> an SGPR); lane (src_byte / 4)'s v, a source per lane (ds_bpermute)
__device__ __forceinline__ float lane_value(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
__device__ __forceinline__ float lane_bcast(int src_byte, float v) { return __int_as_float(__builtin_amdgcn_ds_bpermute(src_byte, __float_as_int(v))); }

// ---- the gates of a hyper-connection, forward (ManifoldHyperConnectionFuse.gates, ppo_full_lunarlander.py:125-147) ----------
// Sinkhorn-Knopp scalings of a positive N x N matrix (:141-146): u, v with u A v nearly doubly stochastic after sk_it sweeps.
// A row or column sum starts from its first product, as the n = 2 kernels wrote it: the bits of the N-loops' 0 + x (exact), without
// their extra add on the sweeps' dependent chain.
template <int N>
__device__ __forceinline__ void sinkhorn_sweeps(const float (&A)[N][N], int sk_it, float (&u)[N], float (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) { u[i] = 1.0f; v[i] = 1.0f; }
  for (int it = 0; it < sk_it; ++it) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float s = A[i][0] * v[0];
#pragma unroll
      for (int j = 1; j < N; ++j) s += A[i][j] * v[j];
      u[i] = rcp_(s + 1e-8f);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
      float s = A[0][j] * u[0];
#pragma unroll
      for (int i = 1; i < N; ++i) s += A[i][j] * u[i];
      v[j] = rcp_(s + 1e-8f);
    }
  }
}
// A row's gates from its read-out sums Hs = (norm_w * flat) w [N N + 2 N] and Hs[N N + 2 N] = |flat|^2, nc = N D columns:
// z = r_inv Hs alpha + beta, r_inv = 1 / (|flat| / sqrt(nc) + 1e-6);  pre = sigmoid(z[:N]), post = 2 sigmoid(z[N:2N]),
// mix = u exp(z[2N:]) v.  beta: N N + 2 N floats, global memory or registers.
template <int N>
__device__ __forceinline__ void row_gates(const float (&Hs)[N * N + 2 * N + 1], int nc, const float (&alpha)[3], const float* beta,
                                          int sk_it, float (&pre)[N], float (&post)[N], float (&mix)[N][N]) {
  const float r_inv = 1.0f / (sqrtf(Hs[N * N + 2 * N]) / sqrtf((float)nc) + 1e-6f);
  float A[N][N], u[N], v[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    pre[i] = sigmoidf_(r_inv * Hs[i] * alpha[0] + beta[i]);
    post[i] = 2.0f * sigmoidf_(r_inv * Hs[N + i] * alpha[1] + beta[N + i]);
#pragma unroll
    for (int j = 0; j < N; ++j) A[i][j] = exp_(r_inv * Hs[2 * N + i * N + j] * alpha[2] + beta[2 * N + i * N + j]);
  }
  sinkhorn_sweeps<N>(A, sk_it, u, v);
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) mix[i][j] = u[i] * A[i][j] * v[j];
}

// ---- and backward, a row's phase (u, v are constants: the reference computes them under no_grad).  up = the row's upstream
// (d_pre [N], d_post [N], d_mix [N N]), gates = its saved (pre, post, mix) in that order, st = the sums the forward saved (row_gates'
// Hs), al = alpha.  dz = up times sigmoid' / exp' from the saved outputs, dH = dz r alpha, dn_over =
// d|flat| / |flat| from d r = sum dz H alpha.  The row's terms of d alpha (dz r H) and d beta (dz) are the callers': they guard them differently.
template <int N>
__device__ __forceinline__ void row_gates_bwd(const float (&up)[N * N + 2 * N], const float (&gates)[N * N + 2 * N],
                                              const float (&st)[N * N + 2 * N + 1], const float (&al)[3], float inv_sqrt_nc,
                                              float (&dz)[N * N + 2 * N], float (&dH)[N * N + 2 * N], float& r, float& dn_over) {
  constexpr int G = N * N + 2 * N;
  const float norm = sqrtf(st[G]);
  r = 1.0f / (norm * inv_sqrt_nc + 1e-6f);
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const float y = gates[k];
    dz[k] = k < N ? up[k] * y * (1.0f - y) : (k < 2 * N ? up[k] * y * (1.0f - 0.5f * y) : up[k] * y);
  }
  float d_r = 0.0f;
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const int gi = k < N ? 0 : (k < 2 * N ? 1 : 2);
    dH[k] = dz[k] * r * al[gi];
    d_r += dz[k] * st[k] * al[gi];
  }
  const float d_norm = d_r * (-r * r * inv_sqrt_nc);
  dn_over = norm > 0.0f ? d_norm / norm : 0.0f;
}

// ---- the parameter gradients: one 256-column block's partial of the gates' backward (n = 2, 8 gates) = d norm_w | d w | d alpha | d beta
constexpr int kGatesW = 256, kGatesAlpha = kGatesW + 256 * 8, kGatesBeta = kGatesAlpha + 3, kGatesLen = kGatesBeta + 8;
// out[i] = the WAVES waves' partial vectors red[wave][kGatesLen] (LDS) added in a fixed order, by the whole workgroup
template <int WAVES>
__device__ __forceinline__ void add_wave_partials(const float* red, float* out) {
  for (int i = threadIdx.x; i < kGatesLen; i += 64 * WAVES) {
    float sum = red[i];
#pragma unroll
    for (int w2 = 1; w2 < WAVES; ++w2) sum += red[(size_t)w2 * kGatesLen + i];
    out[i] = sum;
  }
}

// out[i] = sum over b < blocks (ascending within eight fixed slices, the slices ascending) of partial[(y * blocks + b) * len + i];
// the destination of element i of column block y is the segment it falls in: seg_end[s - 1] <= i < seg_end[s] ->
// dst[s][y * seg_stride[s] + i - seg_end[s - 1]]  (seg_stride 0: only column block 0 writes the segment)
struct ReduceArgs {
  const float* partial; int blocks, len, n_seg;
  int seg_end[4]; int seg_stride[4]; float* dst[4];
};
inline ReduceArgs gates_reduce_args(const void* workspace, int blocks, float* d_norm_w, float* d_w, float* d_alpha, float* d_beta) {
  return ReduceArgs{static_cast<const float*>(workspace), blocks, kGatesLen, 4,
                    {kGatesW, kGatesAlpha, kGatesBeta, kGatesLen}, {256, 256 * 8, 0, 0}, {d_norm_w, d_w, d_alpha, d_beta}};
}
template <int = 0>                                         // (a template: a unit that launches none emits none)
__global__ __launch_bounds__(256) void partial_reduce_kernel(const ReduceArgs a) {
  __shared__ float part[8][32];
  const int col = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + col, y = blockIdx.y;
  float s = 0.0f;
  if (i < a.len) {
    const int per = (a.blocks + 7) / 8;
    const int b0 = sl * per, b1 = b0 + per < a.blocks ? b0 + per : a.blocks;
    const float* p = a.partial + (size_t)y * a.blocks * a.len + i;
#pragma unroll 8                                           // eight loads in flight (one at a time: 64 us for 512 partials)
    for (int b = b0; b < b1; ++b) s += p[(size_t)b * a.len];
  }
  part[sl][col] = s;
  __syncthreads();
  if (sl == 0 && i < a.len) {
#pragma unroll
    for (int k = 1; k < 8; ++k) s += part[k][col];
    int lo = 0;
    for (int sg = 0; sg < a.n_seg; ++sg) {
      if (i < a.seg_end[sg]) {
        if (a.seg_stride[sg] || y == 0) a.dst[sg][(size_t)y * a.seg_stride[sg] + (i - lo)] = s;
        break;
      }
      lo = a.seg_end[sg];
    }
  }
}

}  // namespace
}  // namespace mhc
}  // namespace gymrl
