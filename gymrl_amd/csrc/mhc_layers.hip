// mhc_layers.hip — a hyper-connection layer by layer: what PPO-full runs for every shape but the default one (mhc.hip has that
// one's one-launch kernels and the backbone's description) and in the non-fused training nodes (_MhcGates / _MhcRead / _MhcCombine).
// Rollout, per layer: gymrl_mhc_gates (gates + read = sum_i pre_i h_i), gymrl_lin_fwd (csrc/lin.hip), gymrl_mhc_combine
//   (h'[b, i, :] = post_i out + sum_j mix_ij h[b, j, :]), gymrl_rmsnorm (csrc/mhc_norm.hip).  Training pass: gymrl_mhc_gates (+ stats) /
//   gymrl_mhc_gates_bwd, gymrl_mhc_combine(_bwd) with SiLU on load, gymrl_mhc_read_fwd/_bwd, gymrl_sinkhorn; parameter gradients are
//   per-workgroup partial sums added in a fixed order.  The gate arithmetic itself (forward, the backward's row phase): mhc_device.hpp.
#include "mhc_device.hpp"
#include "../../include/gymrl.h"

namespace {
using namespace gymrl;
using namespace gymrl::mhc;

struct GatesArgs {
  const float* h; const float* norm_w; const float* w; const float* alpha; const float* beta;
  float* pre; float* post; float* mix; float* read; float* stats;
  int B, D, sk_it;
};

template <int N>
__global__ __launch_bounds__(64 * kWaves) void mhc_gates_kernel(const GatesArgs a) {
  constexpr int G = N * N + 2 * N;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= a.B) return;
  const int nc = N * a.D;
  const float* __restrict__ hr = a.h + (size_t)row * nc;
  float Hs[G], sq = 0.0f;
#pragma unroll
  for (int j = 0; j < G; ++j) Hs[j] = 0.0f;
  for (int c = 4 * lane; c < nc; c += 256) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(hr + c);
    const f32x4 nw = *reinterpret_cast<const f32x4*>(a.norm_w + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = nw[e] * x[e];
      sq += x[e] * x[e];
      const float* wr = a.w + (size_t)(c + e) * G;
#pragma unroll
      for (int j = 0; j < G; ++j) Hs[j] += t * wr[j];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sq += __shfl_xor(sq, off, 64);
#pragma unroll
    for (int j = 0; j < G; ++j) Hs[j] += __shfl_xor(Hs[j], off, 64);
  }
  // every lane now holds the row's sums
  float sums[G + 1], pre[N], post[N], mix[N][N];            // (Hs and sq stay apart above: as one array the kernel's registers change)
#pragma unroll
  for (int j = 0; j < G; ++j) sums[j] = Hs[j];
  sums[G] = sq;
  const float al[3] = {a.alpha[0], a.alpha[1], a.alpha[2]};
  row_gates<N>(sums, nc, al, a.beta, a.sk_it, pre, post, mix);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      a.pre[(size_t)row * N + i] = pre[i];
      a.post[(size_t)row * N + i] = post[i];
#pragma unroll
      for (int j = 0; j < N; ++j) a.mix[((size_t)row * N + i) * N + j] = mix[i][j];
    }
  }
  for (int d = lane; d < a.D; d += 64) {                   // read = bmm(pre, h): the weighted sum of the branches
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) s += pre[i] * hr[i * a.D + d];
    a.read[(size_t)row * a.D + d] = s;
  }
}

// The n = 2 gates at nc = 256 * CH columns.  The one-wave-per-row kernel above spends ~1100 of its ~1500 instructions per row on
// the Sinkhorn sweeps, every lane repeating them (0.3 ms at 131072 rows against 50 us of HBM time; 23 us per rollout call at 4096
// rows).  Here a wave takes RB = 16 / CH rows: 16 lanes per row (a 256-byte segment per load, all of the batch's loads issued up
// front and kept in registers for the read-out), the read-out sums through DPP, then ONE lane per row does the sigmoids, the exp
// and the sweeps, and the branch sum is formed from the registers.  stats [B, 9] (optional) = the eight read-out sums and
// |flat|^2 of the row, for gymrl_mhc_gates_bwd.
template <int CH>
__global__ __launch_bounds__(64) void mhc_gates2_kernel(const GatesArgs a) {
  constexpr int N = 2, G = 8, IT = 4 / CH, RB = 4 * IT, Q = 4 * CH;
  const int lane = threadIdx.x, sub = lane & 15, grp = lane >> 4;
  const int nc = 256 * CH;
  const int64_t base = (int64_t)blockIdx.x * RB;
  f32x4 x[IT][Q];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    int64_t row = base + grp * IT + it;
    if (row > a.B - 1) row = a.B - 1;
    const float* hr = a.h + row * nc + 4 * sub;
#pragma unroll
    for (int q = 0; q < Q; ++q) x[it][q] = *reinterpret_cast<const f32x4*>(hr + 64 * q);
  }
  float Hs[IT][G + 1];
#pragma unroll
  for (int it = 0; it < IT; ++it)
#pragma unroll
    for (int k = 0; k <= G; ++k) Hs[it][k] = 0.0f;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int c = 64 * q + 4 * sub;
    const f32x4 nw = *reinterpret_cast<const f32x4*>(a.norm_w + c);
    float wq[4][G];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(a.w + (size_t)(c + e) * G);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(a.w + (size_t)(c + e) * G + 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) { wq[e][k] = lo[k]; wq[e][4 + k] = hi[k]; }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xv = x[it][q][e], t = nw[e] * xv;
        Hs[it][G] += xv * xv;
#pragma unroll
        for (int k = 0; k < G; ++k) Hs[it][k] += t * wq[e][k];
      }
  }
  float mine[G + 1];                                       // lane `sub` of a group keeps the sums of the group's row `sub`
#pragma unroll
  for (int k = 0; k <= G; ++k) mine[k] = 0.0f;
#pragma unroll
  for (int it = 0; it < IT; ++it)
#pragma unroll
    for (int k = 0; k <= G; ++k) {
      const float s = row16_sum(Hs[it][k]);
      mine[k] = sub == it ? s : mine[k];
    }
  const int64_t my_row = base + grp * IT + sub;
  float pre[N] = {0.0f, 0.0f};
  if (sub < IT && my_row < a.B) {
    const float al[3] = {a.alpha[0], a.alpha[1], a.alpha[2]};
    float post[N], mix[N][N];
    row_gates<N>(mine, nc, al, a.beta, a.sk_it, pre, post, mix);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      a.pre[my_row * N + i] = pre[i];
      a.post[my_row * N + i] = post[i];
#pragma unroll
      for (int j = 0; j < N; ++j) a.mix[(my_row * N + i) * N + j] = mix[i][j];
    }
    if (a.stats) {
#pragma unroll
      for (int k = 0; k <= G; ++k) a.stats[my_row * (G + 1) + k] = mine[k];
    }
  }
  // read = pre_0 h_0 + pre_1 h_1 from the registers: row (grp, it)'s gates live in lane 16 grp + it
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int src = ((lane & 48) + it) << 2;
    const float p0 = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(pre[0])));
    const float p1 = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(pre[1])));
    const int64_t row = base + grp * IT + it;
    if (row < a.B) {
#pragma unroll
      for (int q = 0; q < Q / 2; ++q) {
        f32x4 s;
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = p0 * x[it][q][e] + p1 * x[it][q + Q / 2][e];
        *reinterpret_cast<f32x4*>(a.read + row * (nc / 2) + 64 * q + 4 * sub) = s;
      }
    }
  }
}

template <int N>
__global__ __launch_bounds__(256) void mhc_combine_kernel(const float* __restrict__ post, const float* __restrict__ mix,
                                                          const float* __restrict__ out, const float* __restrict__ h, int B,
                                                          int D, int silu, float* __restrict__ h_out) {
  const int64_t total = (int64_t)B * D;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t b = t / D;
    const int d = (int)(t % D);
    float hv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) hv[j] = h[(b * N + j) * D + d];
    float o = out[b * D + d];
    if (silu) o = silu_(o);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float s = 0.0f;
#pragma unroll
      for (int j = 0; j < N; ++j) s += mix[(b * N + i) * N + j] * hv[j];
      h_out[(b * N + i) * D + d] = post[b * N + i] * o + s;
    }
  }
}

// ---- training pass: the two branch-mixing products of a hyper-connection with their backward, one launch each way ----
// read[b, :] = sum_i pre[b, i] h[b, i, :]                        (MHCBlock._sub :161)
template <int N>
__global__ __launch_bounds__(256) void mhc_read_fwd_kernel(const float* __restrict__ pre, const float* __restrict__ h, int B, int D,
                                                           float* __restrict__ read) {
  const int64_t total = (int64_t)B * (D >> 2);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t b = t / (D >> 2);
    const int d = (int)(t % (D >> 2)) * 4;
    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float p = pre[b * N + i];
      const f32x4 x = *reinterpret_cast<const f32x4*>(h + (b * N + i) * D + d);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += p * x[e];
    }
    *reinterpret_cast<f32x4*>(read + b * D + d) = s;
  }
}

// one wave per row: d_pre[b, i] = sum_d g[b, d] h[b, i, d];  d_h[b, i, d] (+)= pre[b, i] g[b, d]  (d_h == nullptr: d_pre only)
template <int N>
__global__ __launch_bounds__(64 * kWaves) void mhc_read_bwd_kernel(const float* __restrict__ g, const float* __restrict__ pre,
                                                                 const float* __restrict__ h, int B, int D,
                                                                 float* __restrict__ d_pre, float* __restrict__ d_h, int accumulate) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= B) return;
  float p[N], acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) { p[i] = pre[row * N + i]; acc[i] = 0.0f; }
  for (int d = lane; d < D; d += 64) {
    const float gv = g[row * D + d];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int64_t o = (row * N + i) * D + d;
      acc[i] += gv * h[o];
      if (d_h) d_h[o] = accumulate ? d_h[o] + p[i] * gv : p[i] * gv;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[i] += __shfl_xor(acc[i], off, 64);
    if (lane == 0) d_pre[row * N + i] = acc[i];
  }
}

// backward of h'[b, i, :] = post[b, i] out[b, :] + sum_j mix[b, i, j] h[b, j, :], one wave per row:
//   d_post[i] = sum_d g[i, d] out[d];  d_out[d] = sum_i post[i] g[i, d];  d_mix[i, j] = sum_d g[i, d] h[j, d];  d_h[j, d] = sum_i mix[i, j] g[i, d]
template <int N>
__global__ __launch_bounds__(64 * kWaves) void mhc_combine_bwd_kernel(const float* __restrict__ g, const float* __restrict__ post,
                                                                    const float* __restrict__ mix, const float* __restrict__ out,
                                                                    const float* __restrict__ h, int B, int D, int silu,
                                                                    float* __restrict__ d_post, float* __restrict__ d_mix,
                                                                    float* __restrict__ d_out, float* __restrict__ d_h) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= B) return;
  float po[N], mx[N][N], a_post[N], a_mix[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    po[i] = post[row * N + i]; a_post[i] = 0.0f;
#pragma unroll
    for (int j = 0; j < N; ++j) { mx[i][j] = mix[(row * N + i) * N + j]; a_mix[i][j] = 0.0f; }
  }
  for (int d = lane; d < D; d += 64) {
    float gv[N], hv[N];
    const float z = out[row * D + d];
    const float o = silu ? silu_(z) : z;
#pragma unroll
    for (int i = 0; i < N; ++i) { gv[i] = g[(row * N + i) * D + d]; hv[i] = h[(row * N + i) * D + d]; }
    float so = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      so += po[i] * gv[i];
      a_post[i] += gv[i] * o;
#pragma unroll
      for (int j = 0; j < N; ++j) a_mix[i][j] += gv[i] * hv[j];
    }
    d_out[row * D + d] = silu ? so * silu_grad_(z) : so;        // silu: `out` holds z and d_out is dL/dz
    if (d_h) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        float sh = 0.0f;
#pragma unroll
        for (int i = 0; i < N; ++i) sh += mx[i][j] * gv[i];
        d_h[(row * N + j) * D + d] = sh;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a_post[i] += __shfl_xor(a_post[i], off, 64);
    if (lane == 0) d_post[row * N + i] = a_post[i];
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) a_mix[i][j] += __shfl_xor(a_mix[i][j], off, 64);
      if (lane == 0) d_mix[(row * N + i) * N + j] = a_mix[i][j];
    }
  }
}

// ---- training pass: backward of the gates (n = 2 branches) -----------------------------------------------------------
// z = r H alpha + beta with H = (norm_w * flat) w, r = 1 / (|flat| / sqrt(nc) + 1e-6);  pre = sigmoid(z[:n]), post = 2 sigmoid(z[n:2n]),
// mix = u exp(z[2n:]) v with u, v constants (the reference computes them under no_grad).  The forward saved H and |flat|^2 per row
// (stats), so nothing here needs a reduction over a row's columns:
//   phase A, one LANE per row, 64 rows per wave step: dz (sigmoid' / exp' from the saved outputs), dH = dz r alpha,
//            d|flat| / |flat| from d r = sum dz H alpha, and the row's terms of d alpha, d beta;
//   phase B, one lane per 4 columns (a wave covers 256; blockIdx.y picks the 256-column block when nc = 512), streaming the
//            wave's rows two at a time with row r's nine scalars read from lane r (v_readlane -> SGPRs):
//            d flat = norm_w (dH w^T) + d|flat| flat / |flat|   [+ pre_j d_read + sum_i mix_ij g_i: the sub-block's other two
//            consumers of h, folded in so that autograd has nothing to add], and the columns' terms of d norm_w, d w in registers.
// The first version recomputed H with 54 ds_bpermute per row at 2 waves per SIMD and ran 0.44 ms at 131072 rows (0.6 TB/s).
// Parameter gradients: added across the workgroup's waves through LDS in a fixed order, one partial vector per workgroup,
// summed ascending by partial_reduce_kernel: no atomics.
struct GatesBwdArgs {
  const float* h; const float* norm_w; const float* w; const float* alpha;
  const float* pre; const float* post; const float* mix; const float* stats;
  const float* d_pre; const float* d_post; const float* d_mix;
  const float* d_read;                                     // nullable [B, D]: d_h[b, j] += pre[b, j] d_read[b]
  const float* g_out;                                      // nullable [B, 2, D]: d_h[b, j] += sum_i mix[b, i, j] g_out[b, i]
  float* d_h; float* partial;
  int B, D;
};

__global__ __launch_bounds__(64 * kWaves) void mhc_gates_bwd_kernel(const GatesBwdArgs a) {
  constexpr int N = 2, G = N * N + 2 * N, U = 2;
  extern __shared__ float red[];                           // [kWaves][kGatesLen]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nc = N * a.D;
  const int c0 = 256 * blockIdx.y + 4 * lane;              // this lane's four columns of flat
  const int j = c0 / a.D, d0 = c0 % a.D;                   // = branch j, columns d0 .. d0 + 3
  const f32x4 nw = *reinterpret_cast<const f32x4*>(a.norm_w + c0);
  float wr[4][G];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(a.w + (size_t)(c0 + e) * G);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(a.w + (size_t)(c0 + e) * G + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) { wr[e][k] = lo[k]; wr[e][4 + k] = hi[k]; }
  }
  const float al[3] = {a.alpha[0], a.alpha[1], a.alpha[2]};
  float acc_nw[4], acc_w[4][G], acc_al[3] = {0.0f, 0.0f, 0.0f}, acc_be[G];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    acc_nw[e] = 0.0f;
#pragma unroll
    for (int k = 0; k < G; ++k) acc_w[e][k] = 0.0f;
  }
#pragma unroll
  for (int k = 0; k < G; ++k) acc_be[k] = 0.0f;
  const float inv_sqrt_nc = 1.0f / sqrtf((float)nc);
  for (int64_t base = ((int64_t)blockIdx.x * kWaves + wave) * 64; base < a.B; base += (int64_t)gridDim.x * kWaves * 64) {
    // ---- phase A: lane = row
    const int64_t row = base + lane;
    float dH[G], dn_over = 0.0f, p0 = 0.0f, p1 = 0.0f, m00 = 0.0f, m01 = 0.0f, m10 = 0.0f, m11 = 0.0f;
#pragma unroll
    for (int k = 0; k < G; ++k) dH[k] = 0.0f;
    if (row < a.B) {
      float st[G + 1], dz[G], r;
#pragma unroll
      for (int k = 0; k <= G; ++k) st[k] = a.stats[row * (G + 1) + k];
      p0 = a.pre[row * N]; p1 = a.pre[row * N + 1];
      m00 = a.mix[row * 4]; m01 = a.mix[row * 4 + 1]; m10 = a.mix[row * 4 + 2]; m11 = a.mix[row * 4 + 3];
      const float gates[G] = {p0, p1, a.post[row * N], a.post[row * N + 1], m00, m01, m10, m11};
      const float up[G] = {a.d_pre[row * N], a.d_pre[row * N + 1], a.d_post[row * N], a.d_post[row * N + 1],
                           a.d_mix[row * 4], a.d_mix[row * 4 + 1], a.d_mix[row * 4 + 2], a.d_mix[row * 4 + 3]};
      row_gates_bwd<N>(up, gates, st, al, inv_sqrt_nc, dz, dH, r, dn_over);
#pragma unroll
      for (int k = 0; k < G; ++k) {
        acc_al[k < N ? 0 : (k < 2 * N ? 1 : 2)] += dz[k] * r * st[k];
        acc_be[k] += dz[k];
      }
    }
    // ---- phase B: lane = 4 columns, the wave's rows in pairs
    const int nrows = (int)((a.B - base) < 64 ? (a.B - base) : 64);
    for (int r0 = 0; r0 < nrows; r0 += U) {
      f32x4 x[U], gr[U], g0[U], g1[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int rr = r0 + u < nrows ? r0 + u : nrows - 1;
        const int64_t rw = base + rr;
        x[u] = *reinterpret_cast<const f32x4*>(a.h + rw * nc + c0);
        if (a.d_read) gr[u] = *reinterpret_cast<const f32x4*>(a.d_read + rw * a.D + d0);
        if (a.g_out) {
          g0[u] = *reinterpret_cast<const f32x4*>(a.g_out + (rw * N) * a.D + d0);
          g1[u] = *reinterpret_cast<const f32x4*>(a.g_out + (rw * N + 1) * a.D + d0);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int rr = r0 + u;
        if (rr < nrows) {
          float sH[G];
#pragma unroll
          for (int k = 0; k < G; ++k) sH[k] = lane_value(dH[k], rr);
          const float s_dn = lane_value(dn_over, rr);
          f32x4 dx;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float t2 = 0.0f;
#pragma unroll
            for (int k = 0; k < G; ++k) t2 += sH[k] * wr[e][k];
            dx[e] = nw[e] * t2 + s_dn * x[u][e];
            acc_nw[e] += x[u][e] * t2;
            const float t = nw[e] * x[u][e];
#pragma unroll
            for (int k = 0; k < G; ++k) acc_w[e][k] += t * sH[k];
          }
          if (a.d_read) {
            const float pj = j ? lane_value(p1, rr) : lane_value(p0, rr);
#pragma unroll
            for (int e = 0; e < 4; ++e) dx[e] += pj * gr[u][e];
          }
          if (a.g_out) {
            const float m0j = j ? lane_value(m01, rr) : lane_value(m00, rr);
            const float m1j = j ? lane_value(m11, rr) : lane_value(m10, rr);
#pragma unroll
            for (int e = 0; e < 4; ++e) dx[e] += m0j * g0[u][e] + m1j * g1[u][e];
          }
          *reinterpret_cast<f32x4*>(a.d_h + (base + rr) * nc + c0) = dx;
        }
      }
    }
  }
  // d alpha / d beta: the lanes' row sums added across the wave (fixed tree), then everything across the workgroup's waves
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int g = 0; g < 3; ++g) acc_al[g] += __shfl_xor(acc_al[g], off, 64);
#pragma unroll
    for (int k = 0; k < G; ++k) acc_be[k] += __shfl_xor(acc_be[k], off, 64);
  }
  float* mine = red + (size_t)wave * kGatesLen;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = 4 * lane + e;
    mine[c] = acc_nw[e];
#pragma unroll
    for (int k = 0; k < G; ++k) mine[kGatesW + c * G + k] = acc_w[e][k];
  }
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < 3; ++g) mine[kGatesAlpha + g] = acc_al[g];
#pragma unroll
    for (int k = 0; k < G; ++k) mine[kGatesBeta + k] = acc_be[k];
  }
  __syncthreads();
  add_wave_partials<kWaves>(red, a.partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kGatesLen);
}

// Sinkhorn-Knopp scalings of B positive n x n matrices (ManifoldHyperConnectionFuse.gates :141-146, under no_grad in the
// reference: u, v are constants of the backward pass): one lane per matrix instead of ~6 launches per sweep.
template <int N>
__global__ __launch_bounds__(256) void sinkhorn_kernel(const float* __restrict__ A, int B, int sk_it, float* __restrict__ u_out,
                                                       float* __restrict__ v_out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float a[N][N], u[N], v[N];
#pragma unroll
  for (int i = 0; i < N * N; ++i) a[i / N][i % N] = A[(size_t)b * N * N + i];
  sinkhorn_sweeps<N>(a, sk_it, u, v);
#pragma unroll
  for (int i = 0; i < N; ++i) { u_out[(size_t)b * N + i] = u[i]; v_out[(size_t)b * N + i] = v[i]; }
}

}  // namespace

extern "C" {

int gymrl_mhc_gates(const float* h, const float* norm_w, const float* w, const float* alpha, const float* beta, int B, int n,
                    int D, int sk_it, float* pre_out, float* post_out, float* mix_out, float* read_out, float* stats_out,
                    void* stream) {
  if (!h || !norm_w || !w || !alpha || !beta || !pre_out || !post_out || !mix_out || !read_out || B < 0 || D < 4 || D % 4 ||
      sk_it < 0 || (n != 2 && n != 4))
    return -22;
  const bool batched = n == 2 && (n * D == 256 || n * D == 512);
  if (stats_out && !batched) return -22;
  if (B == 0) return 0;
  GatesArgs a{h, norm_w, w, alpha, beta, pre_out, post_out, mix_out, read_out, stats_out, B, D, sk_it};
  if (batched) {
    const int rb = n * D == 256 ? 16 : 8;                  // rows per wave
    const dim3 grid((B + rb - 1) / rb), block(64);
    if (n * D == 256) hipLaunchKernelGGL(mhc_gates2_kernel<1>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(mhc_gates2_kernel<2>, grid, block, 0, (hipStream_t)stream, a);
  } else {
    const dim3 grid((B + kWaves - 1) / kWaves), block(64 * kWaves);
    if (n == 2) hipLaunchKernelGGL(mhc_gates_kernel<2>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(mhc_gates_kernel<4>, grid, block, 0, (hipStream_t)stream, a);
  }
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_mhc_combine(const float* post, const float* mix, const float* out, const float* h, int B, int n, int D, int act,
                      float* h_out, void* stream) {
  if (!post || !mix || !out || !h || !h_out || B < 0 || D < 1 || (n != 2 && n != 4) || (act != GYMRL_ACT_NONE && act != GYMRL_ACT_SILU))
    return -22;
  if (B == 0) return 0;
  int64_t nb = ((int64_t)B * D + 255) / 256;
  if (nb > 4096) nb = 4096;
  const int silu = act == GYMRL_ACT_SILU;
  if (n == 2) hipLaunchKernelGGL(mhc_combine_kernel<2>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, post, mix, out, h, B, D, silu, h_out);
  else hipLaunchKernelGGL(mhc_combine_kernel<4>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, post, mix, out, h, B, D, silu, h_out);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_mhc_read_fwd(const float* pre, const float* h, int B, int n, int D, float* read_out, void* stream) {
  if (!pre || !h || !read_out || B < 0 || D < 4 || D % 4 || (n != 2 && n != 4)) return -22;
  if (B == 0) return 0;
  int64_t nb = ((int64_t)B * (D / 4) + 255) / 256;
  if (nb > 16384) nb = 16384;
  if (n == 2) hipLaunchKernelGGL(mhc_read_fwd_kernel<2>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, pre, h, B, D, read_out);
  else hipLaunchKernelGGL(mhc_read_fwd_kernel<4>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, pre, h, B, D, read_out);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_mhc_read_bwd(const float* g, const float* pre, const float* h, int B, int n, int D, float* d_pre, float* d_h,
                       int accumulate, void* stream) {
  if (!g || !pre || !h || !d_pre || B < 0 || D < 1 || (n != 2 && n != 4)) return -22;
  if (B == 0) return 0;
  const dim3 grid((B + kWaves - 1) / kWaves), block(64 * kWaves);
  if (n == 2) hipLaunchKernelGGL(mhc_read_bwd_kernel<2>, grid, block, 0, (hipStream_t)stream, g, pre, h, B, D, d_pre, d_h, accumulate);
  else hipLaunchKernelGGL(mhc_read_bwd_kernel<4>, grid, block, 0, (hipStream_t)stream, g, pre, h, B, D, d_pre, d_h, accumulate);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_mhc_combine_bwd(const float* g, const float* post, const float* mix, const float* out, const float* h, int B, int n, int D,
                          int act, float* d_post, float* d_mix, float* d_out, float* d_h, void* stream) {
  if (!g || !post || !mix || !out || !h || !d_post || !d_mix || !d_out || B < 0 || D < 1 || (n != 2 && n != 4) ||
      (act != GYMRL_ACT_NONE && act != GYMRL_ACT_SILU))
    return -22;
  if (B == 0) return 0;
  const dim3 grid((B + kWaves - 1) / kWaves), block(64 * kWaves);
  const int silu = act == GYMRL_ACT_SILU;
  if (n == 2) hipLaunchKernelGGL(mhc_combine_bwd_kernel<2>, grid, block, 0, (hipStream_t)stream, g, post, mix, out, h, B, D, silu, d_post, d_mix, d_out, d_h);
  else hipLaunchKernelGGL(mhc_combine_bwd_kernel<4>, grid, block, 0, (hipStream_t)stream, g, post, mix, out, h, B, D, silu, d_post, d_mix, d_out, d_h);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

static int gates_bwd_blocks(int B) {
  int blocks = (B + 64 * kWaves - 1) / (64 * kWaves);     // 512 = every wave slot of the chip at the kernel's 2 waves per SIMD
  return blocks > 512 ? 512 : (blocks < 1 ? 1 : blocks);
}

size_t gymrl_mhc_gates_bwd_workspace_bytes(int n, int D) {
  const int ch = n * D / 256;
  return sizeof(float) * 1024 * (size_t)(ch < 1 ? 1 : ch) * kGatesLen;
}

int gymrl_mhc_gates_bwd(const float* h, const float* norm_w, const float* w, const float* alpha, const float* pre, const float* post,
                        const float* mix, const float* stats, const float* d_pre, const float* d_post, const float* d_mix,
                        const float* d_read, const float* g_out, int B, int n, int D, float* d_h, float* d_norm_w, float* d_w,
                        float* d_alpha, float* d_beta, void* workspace, void* stream) {
  if (!h || !norm_w || !w || !alpha || !pre || !post || !mix || !stats || !d_pre || !d_post || !d_mix || !d_h || !d_norm_w || !d_w ||
      !d_alpha || !d_beta || !workspace || B < 1 || n != 2 || (n * D != 256 && n * D != 512))
    return -22;
  const int ch = n * D / 256, blocks = gates_bwd_blocks(B);
  GatesBwdArgs a{h, norm_w, w, alpha, pre, post, mix, stats, d_pre, d_post, d_mix, d_read, g_out, d_h, static_cast<float*>(workspace),
                 B, D};
  hipLaunchKernelGGL(mhc_gates_bwd_kernel, dim3(blocks, ch), dim3(64 * kWaves), sizeof(float) * kWaves * kGatesLen,
                     (hipStream_t)stream, a);
  const ReduceArgs r = gates_reduce_args(workspace, blocks, d_norm_w, d_w, d_alpha, d_beta);
  hipLaunchKernelGGL(partial_reduce_kernel<>, dim3((kGatesLen + 31) / 32, ch), dim3(256), 0, (hipStream_t)stream, r);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_sinkhorn(const float* A, int B, int n, int sk_it, float* u_out, float* v_out, void* stream) {
  if (!A || !u_out || !v_out || B < 0 || sk_it < 0 || (n != 2 && n != 4)) return -22;
  if (B == 0) return 0;
  const dim3 grid((B + 255) / 256), block(256);
  if (n == 2) hipLaunchKernelGGL(sinkhorn_kernel<2>, grid, block, 0, (hipStream_t)stream, A, B, sk_it, u_out, v_out);
  else hipLaunchKernelGGL(sinkhorn_kernel<4>, grid, block, 0, (hipStream_t)stream, A, B, sk_it, u_out, v_out);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
