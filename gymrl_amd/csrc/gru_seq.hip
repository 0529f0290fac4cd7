// gru_seq.hip — the GRU recurrence over whole episodes in one launch per direction (ppg_rnn_lunarlander.py:125-140,
// ppo_rnn_lunarlander.py: MLPRNN's nn.GRU(256, 64) fed one unbatched [T, 256] episode at a time).
//
//   gymrl_gru_seq_fwd   h_t = cell(gi_t, h_{t-1} W_hh^T + b_hh, h_{t-1}) for t < len[b], every step in one launch
//   gymrl_gru_seq_bwd   the reverse recurrence: gh_t recomputed from the stored h_{t-1}, the cell backward, and
//                       dh_{t-1} = dh_direct + dgh_t . W_hh, every step in one launch
//
// The input projection gi = x W_ih^T + b_ih and the weight gradients (dW_hh = sum_t dgh_t^T h_{t-1}, db_hh, dW_ih, dx)
// are one library GEMM each over the flattened [T*B] rows; what is left is the dependent chain of small GEMMs that a
// per-step composition runs as 2T launches per direction.
//
// Layout.  A workgroup owns a tile of 16 rows (episodes) and runs all of its steps alone: rows never interact, so no
// workgroup waits for another and each step ends with one workgroup barrier.  It has H / 16 waves; wave w owns hidden
// units [16w, 16w + 16) and computes the r, z and n gate tiles of exactly those units (3 x H/4 v_mfma_f32_16x16x4_f32,
// exact f32 products), so the pointwise cell (gru_cell_device.hpp, the arithmetic of gymrl_gru_cell_fwd / _bwd) runs
// from the accumulators.  Lane (r = lane & 15, q = lane >> 4) holds rows 4q..4q+3 of unit 16w + r.
//   * W_hh stays in registers for the whole launch: each wave loads the B operands of its own three gate tiles once
//     (3 * H/16 f32x4 per lane, 48 VGPRs at H = 64; the backward also keeps the transposed slice for dgh . W_hh, another
//     48), so every element of W_hh is read from memory once per workgroup and never again.
//   * h_{t-1} (forward) and dgh_t (backward) are the only operands a wave needs from the other waves: they pass through a
//     double-buffered 16-row LDS tile (16 x (H+4) and 16 x (3H+4) floats), which is what makes one barrier per step enough.
//   * gi_{t+1} (and, backward, h_{t-2}, d_hseq_{t-1}) are loaded while step t computes.
// Rows with t >= len[b] are frozen: h_seq is written as zero, h stays h_{len-1} (so h_last = h_{len-1}), and backward
// they write zero gradients and pass dh through unchanged.  A tile stops at its longest row; the tails are zero-filled.
//
// Lengths are host arrays (validated before any HIP call) and reach the kernel by value, 768 rows per launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gymrl.h"
#include "gru_cell_device.hpp"

using namespace gymrl;

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kRows = 16;                  // rows of a tile = rows of an MFMA tile
constexpr int kLaunchRows = 768;           // lengths passed by value per launch (3 KB of kernel arguments)

struct SeqLens {
  int32_t len[kLaunchRows];
};

__device__ __forceinline__ v4f mfma16(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

template <int H>
__global__ __launch_bounds__(4 * H) void gru_seq_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ W,
                                                             const float* __restrict__ bh, const float* __restrict__ h0, int T,
                                                             int B, int row0, int nrows, SeqLens L, float* __restrict__ h_seq,
                                                             float* __restrict__ h_last) {
  constexpr int NC = H / 16;
  constexpr int LD = H + 4;
  __shared__ float hs[2][kRows][LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int u = 16 * w + r;
  const int tr0 = blockIdx.x * kRows;

  int lenr[4];
  bool rowok[4];
  int64_t brow[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int i = tr0 + 4 * q + g;
    rowok[g] = i < nrows;
    lenr[g] = rowok[g] ? L.len[i] : 0;
    brow[g] = (int64_t)row0 + i;
  }
  int tmax = 0;
  for (int i = 0; i < kRows; ++i)
    if (tr0 + i < nrows) tmax = max(tmax, L.len[tr0 + i]);

  v4f wb[3][NC];
#pragma unroll
  for (int gt = 0; gt < 3; ++gt)
#pragma unroll
    for (int c = 0; c < NC; ++c) wb[gt][c] = *reinterpret_cast<const v4f*>(W + (size_t)(gt * H + u) * H + 16 * c + 4 * q);
  const float br = bh[u], bz = bh[H + u], bn = bh[2 * H + u];

  float hreg[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    hreg[g] = (rowok[g] && h0) ? h0[brow[g] * H + u] : 0.0f;
    hs[0][4 * q + g][u] = hreg[g];
  }
  __syncthreads();

  float gc[4][3], gn[4][3];
  auto load_gi = [&](int t, float (&d)[4][3]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (rowok[g] && t < lenr[g]) {
        const float* p = gi + ((size_t)t * B + brow[g]) * (3 * H) + u;
        d[g][0] = p[0]; d[g][1] = p[H]; d[g][2] = p[2 * H];
      } else {
        d[g][0] = d[g][1] = d[g][2] = 0.0f;
      }
    }
  };
  if (tmax > 0) load_gi(0, gc);

  for (int t = 0; t < tmax; ++t) {
    const int cur = t & 1;
    if (t + 1 < tmax) load_gi(t + 1, gn);
    v4f ar = {br, br, br, br}, az = {bz, bz, bz, bz}, an = {bn, bn, bn, bn};
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const v4f x = *reinterpret_cast<const v4f*>(&hs[cur][r][16 * c + 4 * q]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ar = mfma16(x[e], wb[0][c][e], ar);
        az = mfma16(x[e], wb[1][c][e], az);
        an = mfma16(x[e], wb[2][c][e], an);
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (rowok[g]) {
        float* o = h_seq + ((size_t)t * B + brow[g]) * H + u;
        if (t < lenr[g]) {
          hreg[g] = gru_point_fwd(gc[g][0], gc[g][1], gc[g][2], ar[g], az[g], an[g], hreg[g]);
          *o = hreg[g];
        } else {
          *o = 0.0f;
        }
      }
      hs[cur ^ 1][4 * q + g][u] = hreg[g];
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 4; ++g) { gc[g][0] = gn[g][0]; gc[g][1] = gn[g][1]; gc[g][2] = gn[g][2]; }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    if (!rowok[g]) continue;
    h_last[brow[g] * H + u] = hreg[g];
    for (int t = tmax; t < T; ++t) h_seq[((size_t)t * B + brow[g]) * H + u] = 0.0f;
  }
}

template <int H>
__global__ __launch_bounds__(4 * H) void gru_seq_bwd_kernel(const float* __restrict__ gi, const float* __restrict__ W,
                                                             const float* __restrict__ bh, const float* __restrict__ h0,
                                                             const float* __restrict__ h_seq, const float* __restrict__ d_hseq,
                                                             const float* __restrict__ d_hlast, int T, int B, int row0,
                                                             int nrows, SeqLens L, float* __restrict__ dgi,
                                                             float* __restrict__ dgh, float* __restrict__ dh0) {
  constexpr int NC = H / 16;
  constexpr int N3 = 3 * H / 16;
  constexpr int LDG = 3 * H + 4;
  __shared__ float gs[2][kRows][LDG];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int u = 16 * w + r;
  const int tr0 = blockIdx.x * kRows;

  int lenr[4];
  bool rowok[4];
  int64_t brow[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int i = tr0 + 4 * q + g;
    rowok[g] = i < nrows;
    lenr[g] = rowok[g] ? L.len[i] : 0;
    brow[g] = (int64_t)row0 + i;
  }
  // the A-operand row of this lane (row r of the tile)
  const bool aok = tr0 + r < nrows;
  const int alen = aok ? L.len[tr0 + r] : 0;
  const int64_t arow = (int64_t)row0 + tr0 + r;
  int tmax = 0;
  for (int i = 0; i < kRows; ++i)
    if (tr0 + i < nrows) tmax = max(tmax, L.len[tr0 + i]);

  v4f wf[3][NC];
#pragma unroll
  for (int gt = 0; gt < 3; ++gt)
#pragma unroll
    for (int c = 0; c < NC; ++c) wf[gt][c] = *reinterpret_cast<const v4f*>(W + (size_t)(gt * H + u) * H + 16 * c + 4 * q);
  v4f wt[N3];
#pragma unroll
  for (int c = 0; c < N3; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) wt[c][e] = W[(size_t)(16 * c + 4 * q + e) * H + u];
  const float br = bh[u], bz = bh[H + u], bn = bh[2 * H + u];

  float dhc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) dhc[g] = (rowok[g] && d_hlast) ? d_hlast[brow[g] * H + u] : 0.0f;

  struct Step {
    float gi[4][3];
    float hp[4];
    float dhs[4];
    v4f xa[NC];
  };
  auto load = [&](int t, Step& s) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (rowok[g] && t < lenr[g]) {
        const float* p = gi + ((size_t)t * B + brow[g]) * (3 * H) + u;
        s.gi[g][0] = p[0]; s.gi[g][1] = p[H]; s.gi[g][2] = p[2 * H];
        s.dhs[g] = d_hseq ? d_hseq[((size_t)t * B + brow[g]) * H + u] : 0.0f;
        s.hp[g] = t == 0 ? (h0 ? h0[brow[g] * H + u] : 0.0f) : h_seq[((size_t)(t - 1) * B + brow[g]) * H + u];
      } else {
        s.gi[g][0] = s.gi[g][1] = s.gi[g][2] = 0.0f;
        s.dhs[g] = s.hp[g] = 0.0f;
      }
    }
    const bool ok = aok && t < alen;
    const float* hrow = t == 0 ? (h0 ? h0 + arow * H : nullptr) : h_seq + ((size_t)(t - 1) * B + arow) * H;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const v4f zero = {0.0f, 0.0f, 0.0f, 0.0f};
      s.xa[c] = (ok && hrow) ? *reinterpret_cast<const v4f*>(hrow + 16 * c + 4 * q) : zero;
    }
  };

  Step sc, sn;
  if (tmax > 0) load(tmax - 1, sc);
  for (int t = tmax - 1; t >= 0; --t) {
    const int cur = t & 1;
    if (t > 0) load(t - 1, sn);
    v4f ar = {br, br, br, br}, az = {bz, bz, bz, bz}, an = {bn, bn, bn, bn};
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ar = mfma16(sc.xa[c][e], wf[0][c][e], ar);
        az = mfma16(sc.xa[c][e], wf[1][c][e], az);
        an = mfma16(sc.xa[c][e], wf[2][c][e], an);
      }
    float ddir[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float dir = 0.0f, diz = 0.0f, din = 0.0f, dhn = 0.0f;
      if (rowok[g] && t < lenr[g]) {
        const float go = dhc[g] + sc.dhs[g];
        gru_point_bwd(sc.gi[g][0], sc.gi[g][1], sc.gi[g][2], ar[g], az[g], an[g], sc.hp[g], go, dir, diz, din, dhn, ddir[g]);
      } else {
        ddir[g] = dhc[g];
      }
      if (rowok[g]) {
        float* pi = dgi + ((size_t)t * B + brow[g]) * (3 * H) + u;
        float* ph = dgh + ((size_t)t * B + brow[g]) * (3 * H) + u;
        pi[0] = dir; pi[H] = diz; pi[2 * H] = din;
        ph[0] = dir; ph[H] = diz; ph[2 * H] = dhn;
      }
      gs[cur][4 * q + g][u] = dir;
      gs[cur][4 * q + g][H + u] = diz;
      gs[cur][4 * q + g][2 * H + u] = dhn;
    }
    __syncthreads();
    // dh_{t-1} = dh_direct + dgh_t . W_hh  (three accumulators, one per gate block of the reduction)
    v4f a0 = {ddir[0], ddir[1], ddir[2], ddir[3]}, a1 = {0.0f, 0.0f, 0.0f, 0.0f}, a2 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < N3; ++c) {
      const v4f x = *reinterpret_cast<const v4f*>(&gs[cur][r][16 * c + 4 * q]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (c < NC) a0 = mfma16(x[e], wt[c][e], a0);
        else if (c < 2 * NC) a1 = mfma16(x[e], wt[c][e], a1);
        else a2 = mfma16(x[e], wt[c][e], a2);
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) dhc[g] = (a0[g] + a1[g]) + a2[g];
    sc = sn;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    if (!rowok[g]) continue;
    if (dh0) dh0[brow[g] * H + u] = dhc[g];
    for (int t = tmax; t < T; ++t) {
      float* pi = dgi + ((size_t)t * B + brow[g]) * (3 * H) + u;
      float* ph = dgh + ((size_t)t * B + brow[g]) * (3 * H) + u;
      pi[0] = pi[H] = pi[2 * H] = 0.0f;
      ph[0] = ph[H] = ph[2 * H] = 0.0f;
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// T = 0 or B = 0 leaves the [T,B,*] arrays without an element, and an allocator hands out NULL for those
inline bool seq_elems(int T, int B) { return T > 0 && B > 0; }

inline bool lens_ok(const int32_t* len, int B, int T) {
  for (int b = 0; b < B; ++b)
    if (len[b] < 0 || len[b] > T) return false;
  return true;
}

}  // namespace

extern "C" {

int gymrl_gru_seq_fwd(const float* gi, const float* W_hh, const float* b_hh, const float* h0, const int32_t* len, int T, int B,
                      int H, float* h_seq, float* h_last, void* stream) {
  if (!W_hh || !b_hh || !len || T < 0 || B < 0) return -22;
  if (seq_elems(T, B) && (!gi || !h_seq)) return -22;                 // an empty [T,B,*] array may be NULL
  if (B > 0 && !h_last) return -22;
  if (H != 16 && H != 32 && H != 48 && H != 64) return -22;
  if (!aligned16(W_hh) || !aligned16(h_seq) || (h0 && !aligned16(h0))) return -22;
  if (!lens_ok(len, B, T)) return -22;
  for (int row0 = 0; row0 < B; row0 += kLaunchRows) {
    const int nrows = B - row0 < kLaunchRows ? B - row0 : kLaunchRows;
    SeqLens L;
    for (int i = 0; i < nrows; ++i) L.len[i] = len[row0 + i];
    const dim3 grid((nrows + kRows - 1) / kRows), block(4 * H);
    hipStream_t s = (hipStream_t)stream;
    switch (H) {
      case 16: hipLaunchKernelGGL(gru_seq_fwd_kernel<16>, grid, block, 0, s, gi, W_hh, b_hh, h0, T, B, row0, nrows, L, h_seq, h_last); break;
      case 32: hipLaunchKernelGGL(gru_seq_fwd_kernel<32>, grid, block, 0, s, gi, W_hh, b_hh, h0, T, B, row0, nrows, L, h_seq, h_last); break;
      case 48: hipLaunchKernelGGL(gru_seq_fwd_kernel<48>, grid, block, 0, s, gi, W_hh, b_hh, h0, T, B, row0, nrows, L, h_seq, h_last); break;
      default: hipLaunchKernelGGL(gru_seq_fwd_kernel<64>, grid, block, 0, s, gi, W_hh, b_hh, h0, T, B, row0, nrows, L, h_seq, h_last); break;
    }
    GYMRL_CHECK_LAUNCH();
  }
  return 0;
}

int gymrl_gru_seq_bwd(const float* gi, const float* W_hh, const float* b_hh, const float* h0, const float* h_seq,
                      const float* d_hseq, const float* d_hlast, const int32_t* len, int T, int B, int H, float* dgi,
                      float* dgh, float* dh0, void* stream) {
  if (!W_hh || !b_hh || !len || T < 0 || B < 0) return -22;
  if (seq_elems(T, B) && (!gi || !h_seq || !dgi || !dgh)) return -22;  // an empty [T,B,*] array may be NULL
  if (H != 16 && H != 32 && H != 48 && H != 64) return -22;
  if (!aligned16(W_hh) || !aligned16(h_seq) || (h0 && !aligned16(h0))) return -22;
  if (!lens_ok(len, B, T)) return -22;
  for (int row0 = 0; row0 < B; row0 += kLaunchRows) {
    const int nrows = B - row0 < kLaunchRows ? B - row0 : kLaunchRows;
    SeqLens L;
    for (int i = 0; i < nrows; ++i) L.len[i] = len[row0 + i];
    const dim3 grid((nrows + kRows - 1) / kRows), block(4 * H);
    hipStream_t s = (hipStream_t)stream;
#define GRU_SEQ_BWD(HH)                                                                                                  \
  hipLaunchKernelGGL(gru_seq_bwd_kernel<HH>, grid, block, 0, s, gi, W_hh, b_hh, h0, h_seq, d_hseq, d_hlast, T, B, row0, \
                     nrows, L, dgi, dgh, dh0)
    switch (H) {
      case 16: GRU_SEQ_BWD(16); break;
      case 32: GRU_SEQ_BWD(32); break;
      case 48: GRU_SEQ_BWD(48); break;
      default: GRU_SEQ_BWD(64); break;
    }
#undef GRU_SEQ_BWD
    GYMRL_CHECK_LAUNCH();
  }
  return 0;
}

}  // extern "C"
