// mhc_norm.hip — RMSNorm and the heads' SiLU -> RMSNorm -> Linear tail, one launch each way; nothing here is specific to hyper-connections.
//   gymrl_rmsnorm / gymrl_rmsnorm_bwd / gymrl_rmsnorm_sum_bwd (optionally over a branch sum / of SiLU(x)), gymrl_norm_proj_fwd / _bwd;
//   parameter gradients are per-workgroup partial sums added in a fixed order (mhc_device.hpp partial_reduce_kernel).
#include "mhc_device.hpp"
#include "../../include/gymrl.h"

namespace {
using namespace gymrl;
using namespace gymrl::mhc;

// y = s * rsqrt(mean(s^2) + eps) * w per row; n_sum > 1: s = the sum of n_sum consecutive [D] blocks of the row;
// silu: s = SiLU(x) (the MLPs' Linear -> SiLU -> RMSNorm: the activation rides in the norm's two launches)
__global__ __launch_bounds__(64 * kWaves) void rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             int B, int D, int n_sum, float eps, int silu, float* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= B) return;
  const float* xr = x + (size_t)row * n_sum * D;
  float sq = 0.0f;
  for (int d = lane; d < D; d += 64) {
    float s = xr[d];
    for (int k = 1; k < n_sum; ++k) s += xr[k * D + d];
    if (silu) s = silu_(s);
    sq += s * s;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
  const float r = rsqrtf(sq / (float)D + eps);
  for (int d = lane; d < D; d += 64) {
    float s = xr[d];
    for (int k = 1; k < n_sum; ++k) s += xr[k * D + d];
    if (silu) s = silu_(s);
    y[(size_t)row * D + d] = s * r * w[d];
  }
}

// the same with the row in registers (D <= 64 Q): one read of x, SiLU evaluated once
template <int Q>
__global__ __launch_bounds__(64 * kWaves) void rmsnorm_reg_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 int B, int D, int n_sum, float eps, int silu, float* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  float wv[Q];                                             // the norm's weight: constants of the launch
#pragma unroll
  for (int q = 0; q < Q; ++q) wv[q] = lane + 64 * q < D ? w[lane + 64 * q] : 0.0f;
  // a wave walks rows (262144 one-row waves cost more in dispatch than in HBM time: 2.8 TB/s)
  for (int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); row < B; row += (int64_t)gridDim.x * kWaves) {
    const float* xr = x + (size_t)row * n_sum * D;
    float sv[Q], sq = 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int d = lane + 64 * q;
      float s = 0.0f;
      if (d < D) {
        s = xr[d];
        for (int k = 1; k < n_sum; ++k) s += xr[k * D + d];
        if (silu) s = silu_(s);
      }
      sv[q] = s;
      sq += s * s;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
    const float r = rsqrtf(sq / (float)D + eps);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int d = lane + 64 * q;
      if (d < D) y[(size_t)row * D + d] = sv[q] * r * wv[q];
    }
  }
}

// backward of y = s r w, s = x or SiLU(x), r = rsqrt(mean(s^2) + eps), one wave per row (D <= 512, lane l holds columns l + 64 q):
//   d s = r (w g) - s r^3 / D sum_d(w g s);  d x = d s [SiLU'(x)];  d w[d] = sum over rows g s r — per-lane column sums over the rows
// the wave visits, added across the workgroup's waves through LDS, one partial vector per workgroup for partial_reduce_kernel.
template <int kNormQ>
__global__ __launch_bounds__(64 * kWaves) void rmsnorm_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                 const float* __restrict__ w, int B, int D, int n_sum, float eps, int silu,
                                                                 float* __restrict__ d_x, float* __restrict__ partial) {
  __shared__ float red[kWaves][64 * kNormQ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float wv[kNormQ], acc[kNormQ];
#pragma unroll
  for (int q = 0; q < kNormQ; ++q) {
    const int d = lane + 64 * q;
    wv[q] = d < D ? w[d] : 0.0f;
    acc[q] = 0.0f;
  }
  const float inv_d = 1.0f / (float)D;
  for (int64_t row = (int64_t)blockIdx.x * kWaves + wave; row < B; row += (int64_t)gridDim.x * kWaves) {
    float xv[kNormQ], gv[kNormQ], sv[kNormQ], sq = 0.0f, dot = 0.0f;
#pragma unroll
    for (int q = 0; q < kNormQ; ++q) {
      const int d = lane + 64 * q;
      float xs = 0.0f;                                     // x = the sum of the row's n_sum blocks (ascending, as the forward adds them)
      if (d < D)
        for (int i = 0; i < n_sum; ++i) xs += x[(row * n_sum + i) * D + d];
      xv[q] = xs;
      gv[q] = d < D ? g[row * D + d] : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < kNormQ; ++q) {
      sv[q] = silu ? silu_(xv[q]) : xv[q];
      sq += sv[q] * sv[q];
      dot += wv[q] * gv[q] * sv[q];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sq += __shfl_xor(sq, off, 64);
      dot += __shfl_xor(dot, off, 64);
    }
    const float r = rsqrtf(sq * inv_d + eps);
    const float k3 = r * r * r * inv_d * dot;
#pragma unroll
    for (int q = 0; q < kNormQ; ++q) {
      const int d = lane + 64 * q;
      if (d < D) {
        float ds = r * wv[q] * gv[q] - sv[q] * k3;
        if (silu) ds *= silu_grad_(xv[q]);
        d_x[row * D + d] = ds;
        acc[q] += gv[q] * sv[q] * r;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kNormQ; ++q) red[wave][lane + 64 * q] = acc[q];
  __syncthreads();
  for (int i = threadIdx.x; i < D; i += 64 * kWaves) {
    float sum = red[0][i];
#pragma unroll
    for (int w2 = 1; w2 < kWaves; ++w2) sum += red[w2][i];
    partial[(size_t)blockIdx.x * D + i] = sum;
  }
}

// ---- training pass: a head's tail, SiLU -> RMSNorm -> Linear(D -> n_out <= 8), in one launch each way ---------------------
// MLP([128, 256, n_out]) (:371-402) ends in y = RMSNorm(SiLU(x)), out = y W2^T + b2 with n_out = 4 (actor) or 1 (critic).  As the
// norm's launches plus the layer kernels that is 1 KB of y per row written, read back twice (the projection, its weight
// gradient) and a [B, D] gradient d y written and re-read: 2.2 KB per row of traffic that carries 16 bytes of information.
// Here a wave walks rows with the row in registers (rmsnorm_reg_kernel's layout: lane l holds columns l + 64 q): forward =
// one read of x, n_out + 1 wave sums; backward = x and the n_out output gradients in, d x out, y recomputed for d W2, and
// the three parameter sums (d norm_w, d W2, d b2) per lane over the rows the wave visits, added across the workgroup through
// LDS: one partial vector per workgroup for partial_reduce_kernel.
template <int Q, int NO>
__global__ __launch_bounds__(64 * kWaves) void norm_proj_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                   const float* __restrict__ W2, const float* __restrict__ b2, int B,
                                                                   int D, int n_out, float eps, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  float wv[Q], W2r[NO][Q], b2r[NO];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int d = lane + 64 * q;
    wv[q] = d < D ? w[d] : 0.0f;
#pragma unroll
    for (int o = 0; o < NO; ++o) W2r[o][q] = (o < n_out && d < D) ? W2[(size_t)o * D + d] : 0.0f;
  }
#pragma unroll
  for (int o = 0; o < NO; ++o) b2r[o] = (o < n_out && b2) ? b2[o] : 0.0f;
  for (int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); row < B; row += (int64_t)gridDim.x * kWaves) {
    float sq = 0.0f, dot[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) dot[o] = 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int d = lane + 64 * q;
      const float sv = d < D ? silu_(x[row * D + d]) : 0.0f;
      sq += sv * sv;
      const float t = sv * wv[q];
#pragma unroll
      for (int o = 0; o < NO; ++o) dot[o] += t * W2r[o][q];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sq += __shfl_xor(sq, off, 64);
#pragma unroll
      for (int o = 0; o < NO; ++o) dot[o] += __shfl_xor(dot[o], off, 64);
    }
    const float r = rsqrtf(sq / (float)D + eps);
#pragma unroll
    for (int o = 0; o < NO; ++o)
      if (lane == o && o < n_out) out[row * n_out + o] = r * dot[o] + b2r[o];
  }
}

// The forward at D = 256 with FOUR rows per wave (the sub-block kernels' layout: lane (grp, sub) holds columns 64 q + 4 sub .. + 3 of
// row 4 it + grp): 16-byte loads, a row's n_out + 1 sums are four DPP adds across sixteen lanes instead of six ds_bpermute
// butterflies across sixty-four, and two row quads are in flight per wave.  One row per wave (above) read x at 2.3 (n_out = 4) /
// 3.0 TB/s (n_out = 1) at 524 288 rows: 231 / 176 us per launch of PPO-full's update.
template <int NO>
__global__ __launch_bounds__(64 * kWaves) void norm_proj_fwd4_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                    const float* __restrict__ W2, const float* __restrict__ b2, int B,
                                                                    int n_out, float eps, float* __restrict__ out) {
  constexpr int D = 256;
  const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4;
  f32x4 wv[4], W2r[NO][4];
  float b2r[NO];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    wv[q] = *reinterpret_cast<const f32x4*>(w + 64 * q + 4 * sub);
#pragma unroll
    for (int o = 0; o < NO; ++o)
      W2r[o][q] = o < n_out ? *reinterpret_cast<const f32x4*>(W2 + (size_t)o * D + 64 * q + 4 * sub) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
#pragma unroll
  for (int o = 0; o < NO; ++o) b2r[o] = (o < n_out && b2) ? b2[o] : 0.0f;
  const int64_t quads = ((int64_t)B + 3) >> 2;
  const int64_t q0 = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), qs = (int64_t)gridDim.x * kWaves;
  auto load = [&](f32x4 (&v)[4], int64_t quad) {
    int64_t row = 4 * quad + grp;
    if (row > B - 1) row = B - 1;
    const float* xr = x + row * D + 4 * sub;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const f32x4*>(xr + 64 * q);
  };
  f32x4 cur[4], nxt[4];
  if (q0 < quads) load(cur, q0);
  for (int64_t quad = q0; quad < quads; quad += qs) {
    if (quad + qs < quads) load(nxt, quad + qs);
    float sq = 0.0f, dot[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) dot[o] = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float sv = silu_(cur[q][e]);
        sq += sv * sv;
        const float t = sv * wv[q][e];
#pragma unroll
        for (int o = 0; o < NO; ++o) dot[o] += t * W2r[o][q][e];
      }
    sq = row16_sum(sq);
#pragma unroll
    for (int o = 0; o < NO; ++o) dot[o] = row16_sum(dot[o]);
    const float r = rsqrtf(sq / (float)D + eps);
    const int64_t row = 4 * quad + grp;
    if (row < B) {
#pragma unroll
      for (int o = 0; o < NO; ++o)
        if (sub == o && o < n_out) out[row * n_out + o] = r * dot[o] + b2r[o];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
  }
}

template <int Q, int NO>
__global__ __launch_bounds__(64 * kWaves) void norm_proj_bwd_kernel(const float* __restrict__ dl, const float* __restrict__ x,
                                                                   const float* __restrict__ w, const float* __restrict__ W2, int B, int D,
                                                                   int n_out, float eps, float* __restrict__ d_x, float* __restrict__ partial) {
  extern __shared__ float np_red[];                        // [kWaves][len], len = D + n_out * (D + 1)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int len = D + n_out * (D + 1);
  float wv[Q], W2r[NO][Q], acc_w[Q], acc_W2[NO][Q], acc_b[NO];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int d = lane + 64 * q;
    wv[q] = d < D ? w[d] : 0.0f;
    acc_w[q] = 0.0f;
#pragma unroll
    for (int o = 0; o < NO; ++o) { W2r[o][q] = (o < n_out && d < D) ? W2[(size_t)o * D + d] : 0.0f; acc_W2[o][q] = 0.0f; }
  }
#pragma unroll
  for (int o = 0; o < NO; ++o) acc_b[o] = 0.0f;
  const float inv_d = 1.0f / (float)D;
  for (int64_t row = (int64_t)blockIdx.x * kWaves + wave; row < B; row += (int64_t)gridDim.x * kWaves) {
    float xv[Q], sv[Q], gv[Q], dlv[NO], sq = 0.0f, dot = 0.0f;
#pragma unroll
    for (int o = 0; o < NO; ++o) dlv[o] = o < n_out ? dl[row * n_out + o] : 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int d = lane + 64 * q;
      xv[q] = d < D ? x[row * D + d] : 0.0f;
      sv[q] = silu_(xv[q]);
      float g = 0.0f;
#pragma unroll
      for (int o = 0; o < NO; ++o) g += dlv[o] * W2r[o][q];
      gv[q] = g;
      sq += sv[q] * sv[q];
      dot += wv[q] * g * sv[q];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sq += __shfl_xor(sq, off, 64);
      dot += __shfl_xor(dot, off, 64);
    }
    const float r = rsqrtf(sq * inv_d + eps);
    const float k3 = r * r * r * inv_d * dot;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int d = lane + 64 * q;
      if (d < D) {
        d_x[row * D + d] = (r * wv[q] * gv[q] - sv[q] * k3) * silu_grad_(xv[q]);
        acc_w[q] += gv[q] * sv[q] * r;
        const float y = sv[q] * r * wv[q];
#pragma unroll
        for (int o = 0; o < NO; ++o) acc_W2[o][q] += dlv[o] * y;
      }
    }
#pragma unroll
    for (int o = 0; o < NO; ++o) acc_b[o] += dlv[o];
  }
  float* mine = np_red + (size_t)wave * len;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int d = lane + 64 * q;
    if (d < D) {
      mine[d] = acc_w[q];
#pragma unroll
      for (int o = 0; o < NO; ++o)
        if (o < n_out) mine[D + o * D + d] = acc_W2[o][q];
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int o = 0; o < NO; ++o)
      if (o < n_out) mine[D + n_out * D + o] = acc_b[o];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < len; i += 64 * kWaves) {
    float sum = np_red[i];
#pragma unroll
    for (int w2 = 1; w2 < kWaves; ++w2) sum += np_red[(size_t)w2 * len + i];
    partial[(size_t)blockIdx.x * len + i] = sum;
  }
}

// The backward at D = 256 with four rows per wave (norm_proj_fwd4_kernel's layout): x in 16-byte loads, d x in 16-byte stores, a
// row's two sums four DPP adds; the per-lane parameter sums (d norm_w, d W2, d b2 over the rows the lane sees) are folded across the
// four row groups by two butterflies per accumulator at the END, then across the workgroup's waves through LDS as before.
template <int NO>
__global__ __launch_bounds__(64 * kWaves) void norm_proj_bwd4_kernel(const float* __restrict__ dl, const float* __restrict__ x,
                                                                    const float* __restrict__ w, const float* __restrict__ W2, int B,
                                                                    int n_out, float eps, float* __restrict__ d_x, float* __restrict__ partial) {
  constexpr int D = 256;
  extern __shared__ float np_red[];                        // [kWaves][len], len = D + n_out * (D + 1)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 15, grp = lane >> 4;
  const int len = D + n_out * (D + 1);
  f32x4 wv[4], W2r[NO][4], acc_w[4], acc_W2[NO][4];
  float acc_b[NO];
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    wv[q] = *reinterpret_cast<const f32x4*>(w + 64 * q + 4 * sub);
    acc_w[q] = zero;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      W2r[o][q] = o < n_out ? *reinterpret_cast<const f32x4*>(W2 + (size_t)o * D + 64 * q + 4 * sub) : zero;
      acc_W2[o][q] = zero;
    }
  }
#pragma unroll
  for (int o = 0; o < NO; ++o) acc_b[o] = 0.0f;
  const float inv_d = 1.0f / (float)D;
  const int64_t quads = ((int64_t)B + 3) >> 2;
  const int64_t q0 = (int64_t)blockIdx.x * kWaves + wave, qs = (int64_t)gridDim.x * kWaves;
  auto load = [&](f32x4 (&v)[4], float (&dv)[NO], int64_t quad) {
    int64_t row = 4 * quad + grp;
    if (row > B - 1) row = B - 1;
    const float* xr = x + row * D + 4 * sub;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const f32x4*>(xr + 64 * q);
#pragma unroll
    for (int o = 0; o < NO; ++o) dv[o] = o < n_out ? dl[row * n_out + o] : 0.0f;
  };
  f32x4 cur[4], nxt[4];
  float dcur[NO], dnxt[NO];
  if (q0 < quads) load(cur, dcur, q0);
  for (int64_t quad = q0; quad < quads; quad += qs) {
    if (quad + qs < quads) load(nxt, dnxt, quad + qs);
    const int64_t row = 4 * quad + grp;
    const bool ok = row < B;                               // (rows past the batch: loaded as a copy of the last row, no contribution)
    f32x4 sv[4], gv[4];
    float sq = 0.0f, dot = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float s1 = silu_(cur[q][e]);
        float g = 0.0f;
#pragma unroll
        for (int o = 0; o < NO; ++o) g += dcur[o] * W2r[o][q][e];
        sv[q][e] = s1; gv[q][e] = g;
        sq += s1 * s1;
        dot += wv[q][e] * g * s1;
      }
    sq = row16_sum(sq);
    dot = row16_sum(dot);
    const float r = rsqrtf(sq * inv_d + eps);
    const float k3 = r * r * r * inv_d * dot;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 dx;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dx[e] = (r * wv[q][e] * gv[q][e] - sv[q][e] * k3) * silu_grad_(cur[q][e]);
        if (ok) {
          acc_w[q][e] += gv[q][e] * sv[q][e] * r;
          const float y = sv[q][e] * r * wv[q][e];
#pragma unroll
          for (int o = 0; o < NO; ++o) acc_W2[o][q][e] += dcur[o] * y;
        }
      }
      if (ok) *reinterpret_cast<f32x4*>(d_x + row * D + 64 * q + 4 * sub) = dx;
    }
    if (ok) {
#pragma unroll
      for (int o = 0; o < NO; ++o) acc_b[o] += dcur[o];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
#pragma unroll
    for (int o = 0; o < NO; ++o) dcur[o] = dnxt[o];
  }
  // the four row groups hold the same columns: (g0 + g1) + (g2 + g3)
  auto fold = [](float v) { v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64); return v; };
  float* mine = np_red + (size_t)wave * len;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int d = 64 * q + 4 * sub + e;
      const float sw = fold(acc_w[q][e]);
      if (grp == 0) mine[d] = sw;
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        const float s2 = fold(acc_W2[o][q][e]);
        if (grp == 0 && o < n_out) mine[D + o * D + d] = s2;
      }
    }
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    const float sb = fold(acc_b[o]);                       // (every lane of a row group counted its row once: lane 0's view)
    if (lane == 0 && o < n_out) mine[D + n_out * D + o] = sb;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < len; i += 64 * kWaves) {
    float sum = np_red[i];
#pragma unroll
    for (int w2 = 1; w2 < kWaves; ++w2) sum += np_red[(size_t)w2 * len + i];
    partial[(size_t)blockIdx.x * len + i] = sum;
  }
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int gymrl_rmsnorm(const float* x, const float* w, int B, int D, int n_sum, float eps, int act, float* y, void* stream) {
  if (!x || !w || !y || B < 0 || D < 1 || n_sum < 1 || (act != GYMRL_ACT_NONE && act != GYMRL_ACT_SILU)) return -22;
  if (B == 0) return 0;
  const dim3 grid((B + kWaves - 1) / kWaves), block(64 * kWaves);
  const dim3 walk(grid.x > 4096 ? 4096 : grid.x);          // the register-resident kernels: every wave slot of the chip, rows in a loop
  const int silu = act == GYMRL_ACT_SILU;
  hipStream_t s = (hipStream_t)stream;
  if (D <= 128) hipLaunchKernelGGL(rmsnorm_reg_kernel<2>, walk, block, 0, s, x, w, B, D, n_sum, eps, silu, y);
  else if (D <= 256) hipLaunchKernelGGL(rmsnorm_reg_kernel<4>, walk, block, 0, s, x, w, B, D, n_sum, eps, silu, y);
  else if (D <= 512) hipLaunchKernelGGL(rmsnorm_reg_kernel<8>, walk, block, 0, s, x, w, B, D, n_sum, eps, silu, y);
  else hipLaunchKernelGGL(rmsnorm_kernel, grid, block, 0, s, x, w, B, D, n_sum, eps, silu, y);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

static int rmsnorm_bwd_blocks(int B) {
  int blocks = (B + kWaves - 1) / kWaves;
  return blocks > 2048 ? 2048 : (blocks < 1 ? 1 : blocks);
}

size_t gymrl_rmsnorm_bwd_workspace_bytes(int D) { return sizeof(float) * 2048 * (size_t)(D < 1 ? 1 : D); }

int gymrl_rmsnorm_sum_bwd(const float* g, const float* x, const float* w, int B, int D, int n_sum, float eps, int act, float* d_x,
                          float* d_w, void* workspace, void* stream) {
  if (!g || !x || !w || !d_x || !d_w || !workspace || B < 1 || D < 1 || D > 512 || n_sum < 1 ||
      (act != GYMRL_ACT_NONE && act != GYMRL_ACT_SILU))
    return -22;
  const int blocks = rmsnorm_bwd_blocks(B), silu = act == GYMRL_ACT_SILU;
  float* part = static_cast<float*>(workspace);
  const dim3 grid(blocks), block(64 * kWaves);
  if (D <= 128) hipLaunchKernelGGL(rmsnorm_bwd_kernel<2>, grid, block, 0, (hipStream_t)stream, g, x, w, B, D, n_sum, eps, silu, d_x, part);
  else if (D <= 256) hipLaunchKernelGGL(rmsnorm_bwd_kernel<4>, grid, block, 0, (hipStream_t)stream, g, x, w, B, D, n_sum, eps, silu, d_x, part);
  else hipLaunchKernelGGL(rmsnorm_bwd_kernel<8>, grid, block, 0, (hipStream_t)stream, g, x, w, B, D, n_sum, eps, silu, d_x, part);
  ReduceArgs r{part, blocks, D, 1, {D, 0, 0, 0}, {0, 0, 0, 0}, {d_w, nullptr, nullptr, nullptr}};
  hipLaunchKernelGGL(partial_reduce_kernel<>, dim3((D + 31) / 32, 1), dim3(256), 0, (hipStream_t)stream, r);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_rmsnorm_bwd(const float* g, const float* x, const float* w, int B, int D, float eps, int act, float* d_x, float* d_w,
                      void* workspace, void* stream) {
  return gymrl_rmsnorm_sum_bwd(g, x, w, B, D, 1, eps, act, d_x, d_w, workspace, stream);
}

#define NORM_PROJ_DISPATCH(KERNEL, ...)                                                                            \
  do {                                                                                                             \
    if (D <= 128) {                                                                                                \
      if (n_out <= 1) hipLaunchKernelGGL((KERNEL<2, 1>), __VA_ARGS__);                                            \
      else if (n_out <= 4) hipLaunchKernelGGL((KERNEL<2, 4>), __VA_ARGS__);                                       \
      else hipLaunchKernelGGL((KERNEL<2, 8>), __VA_ARGS__);                                                        \
    } else {                                                                                                       \
      if (n_out <= 1) hipLaunchKernelGGL((KERNEL<4, 1>), __VA_ARGS__);                                            \
      else if (n_out <= 4) hipLaunchKernelGGL((KERNEL<4, 4>), __VA_ARGS__);                                       \
      else hipLaunchKernelGGL((KERNEL<4, 8>), __VA_ARGS__);                                                        \
    }                                                                                                              \
  } while (0)

int gymrl_norm_proj_fwd(const float* x, const float* norm_w, const float* W2, const float* b2, int B, int D, int n_out, float eps,
                        float* out, void* stream) {
  if (!x || !norm_w || !W2 || !out || B < 0 || D < 1 || D > 256 || n_out < 1 || n_out > 8) return -22;
  if (B == 0) return 0;
  const dim3 block(64 * kWaves);
  const unsigned want = (unsigned)((B + kWaves - 1) / kWaves);
  const dim3 grid(want > 4096 ? 4096 : want);
  // The kernel — and with it the summation order, i.e. the result's last bits — is chosen by SHAPE alone: D = 256 takes the
  // four-row kernel and therefore REQUIRES 16-byte aligned operands (-22 otherwise: the caller copies to an aligned buffer);
  // a choice by pointer alignment would make the bits depend on where an allocation or a view happens to start.
  if (D == 256 && !(al16(x) && al16(norm_w) && al16(W2))) return -22;
  if (D == 256) {                                                   // four rows per wave (16-byte loads, 16-lane sums)
    const unsigned wq = (unsigned)(((B + 3) / 4 + kWaves - 1) / kWaves);
    const dim3 g4(wq > 2048 ? 2048 : wq);
    if (n_out <= 1) hipLaunchKernelGGL(norm_proj_fwd4_kernel<1>, g4, block, 0, (hipStream_t)stream, x, norm_w, W2, b2, B, n_out, eps, out);
    else if (n_out <= 4) hipLaunchKernelGGL(norm_proj_fwd4_kernel<4>, g4, block, 0, (hipStream_t)stream, x, norm_w, W2, b2, B, n_out, eps, out);
    else hipLaunchKernelGGL(norm_proj_fwd4_kernel<8>, g4, block, 0, (hipStream_t)stream, x, norm_w, W2, b2, B, n_out, eps, out);
    GYMRL_CHECK_LAUNCH();
    return 0;
  }
  NORM_PROJ_DISPATCH(norm_proj_fwd_kernel, grid, block, 0, (hipStream_t)stream, x, norm_w, W2, b2, B, D, n_out, eps, out);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

size_t gymrl_norm_proj_bwd_workspace_bytes(int D, int n_out) {
  return sizeof(float) * 2048 * ((size_t)(D < 1 ? 1 : D) * (size_t)((n_out < 1 ? 1 : n_out) + 1) + (size_t)(n_out < 1 ? 1 : n_out));
}

int gymrl_norm_proj_bwd(const float* d_out, const float* x, const float* norm_w, const float* W2, int B, int D, int n_out, float eps,
                        float* d_x, float* d_norm_w, float* d_W2, float* d_b2, void* workspace, void* stream) {
  if (!d_out || !x || !norm_w || !W2 || !d_x || !d_norm_w || !d_W2 || !d_b2 || !workspace || B < 1 || D < 1 || D > 256 || n_out < 1 ||
      n_out > 8)
    return -22;
  const int blocks = rmsnorm_bwd_blocks(B), len = D + n_out * (D + 1);
  float* part = static_cast<float*>(workspace);
  const dim3 grid(blocks), block(64 * kWaves);
  const size_t lds = sizeof(float) * (size_t)kWaves * len;
  // four rows per wave for ONE output (the critic's head: 244 -> 189 us at 524 288 rows).  With four outputs the per-lane weight and
  // accumulator vectors take 292 registers — one wave per SIMD: 410 us against the one-row kernel's 268 — so n_out > 1 stays there.
  // Chosen by shape alone (gymrl_norm_proj_fwd's rule): D = 256 with one output requires aligned operands.  The backward
  // recomputes the row's 1 / rms in ITS kernel's summation order — for n_out > 1 at D = 256 not the forward's (four-row) order:
  // the two values of r can differ in the last bit, a relative 1e-7 on the gradient, the same for every run.
  if (D == 256 && n_out == 1 && !(al16(x) && al16(norm_w) && al16(W2) && al16(d_x))) return -22;
  if (D == 256 && n_out == 1)
    hipLaunchKernelGGL(norm_proj_bwd4_kernel<1>, grid, block, lds, (hipStream_t)stream, d_out, x, norm_w, W2, B, n_out, eps, d_x, part);
  else
  NORM_PROJ_DISPATCH(norm_proj_bwd_kernel, grid, block, lds, (hipStream_t)stream, d_out, x, norm_w, W2, B, D, n_out, eps, d_x, part);
  ReduceArgs r{part, blocks, len, 3, {D, D + n_out * D, len, 0}, {0, 0, 0, 0}, {d_norm_w, d_W2, d_b2, nullptr}};
  hipLaunchKernelGGL(partial_reduce_kernel<>, dim3((len + 31) / 32, 1), dim3(256), 0, (hipStream_t)stream, r);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
