// lstm_seq.hip — torch.nn.LSTM's cell and its recurrence for the recurrent PPO trainer (ppo_lstm_lunarlander.py:449-491,
// URNN with layer=nn.LSTM: hidden state cat(h, c), chunk_size 2).
//
//   gymrl_lstm_cell_fwd / _bwd  the pointwise half of the cell, one pass over [B, H]: the acting step (L = 1) and every
//                               hidden size the one-launch kernels do not cover (the reference's 512)
//   gymrl_lstm_seq_fwd          (h_t, c_t) = cell(gi_t, h_{t-1} W_hh^T + b_hh, c_{t-1}) for t < len[b], every step in one launch
//   gymrl_lstm_seq_bwd          the reverse recurrence: gh_t recomputed from the stored h_{t-1}, the cell backward from the
//                               stored c_{t-1}, and dh_{t-1} = dgates_t . W_hh, every step in one launch
//
// The arithmetic of the cell is lstm_cell_device.hpp for all four.  The input projection gi = x W_ih^T + b_ih and the
// weight gradients (dW_hh = sum_t dgates_t^T h_{t-1}, db_hh, dW_ih, dx) are one library GEMM each over the flattened
// [T*B] rows; since a = gi + gh, one dgates [T,B,4H] is both dgi and dgh.
//
// Layout of the sequence kernels (gru_seq.hip's).  A workgroup owns a tile of 16 rows and runs all of its steps alone:
// rows never interact, so no workgroup waits for another and each step ends with one workgroup barrier.  It has H / 16
// waves; wave w owns hidden units [16w, 16w + 16) and computes the i, f, g and o gate tiles of exactly those units
// (4 x H/4 v_mfma_f32_16x16x4_f32, exact f32 products), so the pointwise cell runs from the accumulators.  Lane
// (r = lane & 15, q = lane >> 4) holds rows 4q..4q+3 of unit 16w + r.
//   * c never crosses waves: c_t (forward) and dc_t (backward) stay in the owning lane's registers.
//   * W_hh stays in registers for the whole launch: each wave loads the B operands of its own four gate tiles once
//     (4 * H/16 f32x4 per lane, 64 VGPRs at H = 64).  The backward's transposed slice for dgates . W_hh (K = 4H) is kept
//     in LDS, [H][4H + 4] floats written once in the prologue and read-only afterwards: in registers it would be another
//     64 VGPRs on top of the forward slice, the two prefetched steps and the accumulators.
//   * h_{t-1} (forward) and dgates_t (backward) are the only operands a wave needs from the other waves: they pass through
//     a double-buffered 16-row LDS tile (16 x (H+4) and 16 x (4H+4) floats), which is what makes one barrier per step enough.
//   * gi_{t+1} (and, backward, h_{t-2}, c_{t-2}, d_hseq_{t-1}) are loaded while step t computes.
// Rows with t >= len[b] are frozen: h_seq and c_seq are written as zero, (h, c) stay (h, c)_{len-1} (so h_last = h_{len-1},
// c_last = c_{len-1}), and backward they write zero gradients and pass dh and dc through unchanged.  A tile stops at its
// longest row; the tails are zero-filled.
//
// Lengths are host arrays (validated before any HIP call) and reach the kernel by value, 768 rows per launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gymrl.h"
#include "lstm_cell_device.hpp"

using namespace gymrl;

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;                // the per-step cell kernels
constexpr int kRows = 16;                  // rows of a tile = rows of an MFMA tile
constexpr int kLaunchRows = 768;           // lengths passed by value per launch (3 KB of kernel arguments)

struct SeqLens {
  int32_t len[kLaunchRows];
};

__device__ __forceinline__ v4f mfma16(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__global__ __launch_bounds__(kBlock) void lstm_cell_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ gh,
                                                               const float* __restrict__ c, int B, int H,
                                                               float* __restrict__ h_out, float* __restrict__ c_out) {
  const int H4 = H >> 2;
  const int64_t total = (int64_t)B * H4;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int64_t b = e / H4;
    const int k = (int)(e - b * H4) << 2;
    const int64_t g0 = b * 4 * H + k;
    const float4 ii = *reinterpret_cast<const float4*>(gi + g0), fi = *reinterpret_cast<const float4*>(gi + g0 + H),
                 gg = *reinterpret_cast<const float4*>(gi + g0 + 2 * H), oi = *reinterpret_cast<const float4*>(gi + g0 + 3 * H);
    const float4 ih = *reinterpret_cast<const float4*>(gh + g0), fh = *reinterpret_cast<const float4*>(gh + g0 + H),
                 hg = *reinterpret_cast<const float4*>(gh + g0 + 2 * H), oh = *reinterpret_cast<const float4*>(gh + g0 + 3 * H);
    const float4 cp = *reinterpret_cast<const float4*>(c + b * H + k);
    float4 ho, co;
#define LSTM_FWD(x) lstm_point_fwd(ii.x, fi.x, gg.x, oi.x, ih.x, fh.x, hg.x, oh.x, cp.x, ho.x, co.x);
    LSTM_FWD(x) LSTM_FWD(y) LSTM_FWD(z) LSTM_FWD(w)
#undef LSTM_FWD
    *reinterpret_cast<float4*>(h_out + b * H + k) = ho;
    *reinterpret_cast<float4*>(c_out + b * H + k) = co;
  }
}

// gates are recomputed from (gi, gh, c): nothing but the cell's inputs has to be kept for backward
__global__ __launch_bounds__(kBlock) void lstm_cell_bwd_kernel(const float* __restrict__ gi, const float* __restrict__ gh,
                                                               const float* __restrict__ c, const float* __restrict__ dh_out,
                                                               const float* __restrict__ dc_out, int B, int H,
                                                               float* __restrict__ dgates, float* __restrict__ dc) {
  const int H4 = H >> 2;
  const int64_t total = (int64_t)B * H4;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int64_t b = e / H4;
    const int k = (int)(e - b * H4) << 2;
    const int64_t g0 = b * 4 * H + k;
    const float4 ii = *reinterpret_cast<const float4*>(gi + g0), fi = *reinterpret_cast<const float4*>(gi + g0 + H),
                 gg = *reinterpret_cast<const float4*>(gi + g0 + 2 * H), oi = *reinterpret_cast<const float4*>(gi + g0 + 3 * H);
    const float4 ih = *reinterpret_cast<const float4*>(gh + g0), fh = *reinterpret_cast<const float4*>(gh + g0 + H),
                 hg = *reinterpret_cast<const float4*>(gh + g0 + 2 * H), oh = *reinterpret_cast<const float4*>(gh + g0 + 3 * H);
    const float4 cp = *reinterpret_cast<const float4*>(c + b * H + k);
    const float4 dh = *reinterpret_cast<const float4*>(dh_out + b * H + k);
    const float4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    const float4 dcn = dc_out ? *reinterpret_cast<const float4*>(dc_out + b * H + k) : zero;
    float4 di, df, dg, dd, dcp;
#define LSTM_BWD(x) lstm_point_bwd(ii.x, fi.x, gg.x, oi.x, ih.x, fh.x, hg.x, oh.x, cp.x, dh.x, dcn.x, di.x, df.x, dg.x, dd.x, dcp.x);
    LSTM_BWD(x) LSTM_BWD(y) LSTM_BWD(z) LSTM_BWD(w)
#undef LSTM_BWD
    *reinterpret_cast<float4*>(dgates + g0) = di;
    *reinterpret_cast<float4*>(dgates + g0 + H) = df;
    *reinterpret_cast<float4*>(dgates + g0 + 2 * H) = dg;
    *reinterpret_cast<float4*>(dgates + g0 + 3 * H) = dd;
    *reinterpret_cast<float4*>(dc + b * H + k) = dcp;
  }
}

template <int H>
__global__ __launch_bounds__(4 * H) void lstm_seq_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ W,
                                                              const float* __restrict__ bh, const float* __restrict__ h0,
                                                              const float* __restrict__ c0, int T, int B, int row0, int nrows,
                                                              SeqLens L, float* __restrict__ h_seq, float* __restrict__ c_seq,
                                                              float* __restrict__ h_last, float* __restrict__ c_last) {
  constexpr int NC = H / 16;
  constexpr int LD = H + 4;
  __shared__ __attribute__((aligned(16))) float hs[2][kRows][LD];
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

  v4f wb[4][NC];
#pragma unroll
  for (int gt = 0; gt < 4; ++gt)
#pragma unroll
    for (int c = 0; c < NC; ++c) wb[gt][c] = *reinterpret_cast<const v4f*>(W + (size_t)(gt * H + u) * H + 16 * c + 4 * q);
  float bias[4];
#pragma unroll
  for (int gt = 0; gt < 4; ++gt) bias[gt] = bh[gt * H + u];

  float hreg[4], creg[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    hreg[g] = (rowok[g] && h0) ? h0[brow[g] * H + u] : 0.0f;
    creg[g] = (rowok[g] && c0) ? c0[brow[g] * H + u] : 0.0f;
    hs[0][4 * q + g][u] = hreg[g];
  }
  __syncthreads();

  float gc[4][4], gn[4][4];
  auto load_gi = [&](int t, float (&d)[4][4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (rowok[g] && t < lenr[g]) {
        const float* p = gi + ((size_t)t * B + brow[g]) * (4 * H) + u;
        d[g][0] = p[0]; d[g][1] = p[H]; d[g][2] = p[2 * H]; d[g][3] = p[3 * H];
      } else {
        d[g][0] = d[g][1] = d[g][2] = d[g][3] = 0.0f;
      }
    }
  };
  if (tmax > 0) load_gi(0, gc);

  for (int t = 0; t < tmax; ++t) {
    const int cur = t & 1;
    if (t + 1 < tmax) load_gi(t + 1, gn);
    v4f acc[4];
#pragma unroll
    for (int gt = 0; gt < 4; ++gt) acc[gt] = v4f{bias[gt], bias[gt], bias[gt], bias[gt]};
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const v4f x = *reinterpret_cast<const v4f*>(&hs[cur][r][16 * c + 4 * q]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int gt = 0; gt < 4; ++gt) acc[gt] = mfma16(x[e], wb[gt][c][e], acc[gt]);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (rowok[g]) {
        const size_t o = ((size_t)t * B + brow[g]) * H + u;
        if (t < lenr[g]) {
          float hn, cn;
          lstm_point_fwd(gc[g][0], gc[g][1], gc[g][2], gc[g][3], acc[0][g], acc[1][g], acc[2][g], acc[3][g], creg[g], hn, cn);
          hreg[g] = hn;
          creg[g] = cn;
          h_seq[o] = hn;
          c_seq[o] = cn;
        } else {
          h_seq[o] = 0.0f;
          c_seq[o] = 0.0f;
        }
      }
      hs[cur ^ 1][4 * q + g][u] = hreg[g];
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int gt = 0; gt < 4; ++gt) gc[g][gt] = gn[g][gt];
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    if (!rowok[g]) continue;
    if (h_last) h_last[brow[g] * H + u] = hreg[g];
    if (c_last) c_last[brow[g] * H + u] = creg[g];
    for (int t = tmax; t < T; ++t) {
      h_seq[((size_t)t * B + brow[g]) * H + u] = 0.0f;
      c_seq[((size_t)t * B + brow[g]) * H + u] = 0.0f;
    }
  }
}

template <int H>
__global__ __launch_bounds__(4 * H) void lstm_seq_bwd_kernel(const float* __restrict__ gi, const float* __restrict__ W,
                                                              const float* __restrict__ bh, const float* __restrict__ h0,
                                                              const float* __restrict__ c0, const float* __restrict__ h_seq,
                                                              const float* __restrict__ c_seq, const float* __restrict__ d_hseq,
                                                              const float* __restrict__ d_hlast, const float* __restrict__ d_clast,
                                                              int T, int B, int row0, int nrows, SeqLens L,
                                                              float* __restrict__ dgates, float* __restrict__ dh0,
                                                              float* __restrict__ dc0) {
  constexpr int NC = H / 16;
  constexpr int N4 = 4 * H / 16;
  constexpr int LDG = 4 * H + 4;
  __shared__ __attribute__((aligned(16))) float gs[2][kRows][LDG];      // dgates_t of the tile, double-buffered
  __shared__ __attribute__((aligned(16))) float wt[H][LDG];             // wt[u][k] = W_hh[k][u], read-only after the prologue
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

  v4f wf[4][NC];
#pragma unroll
  for (int gt = 0; gt < 4; ++gt)
#pragma unroll
    for (int c = 0; c < NC; ++c) wf[gt][c] = *reinterpret_cast<const v4f*>(W + (size_t)(gt * H + u) * H + 16 * c + 4 * q);
  // W_hh transposed into LDS once: thread x of the 4H walks row k = x of W_hh (coalesced reads are not worth a second
  // pass here: 4H * H floats per workgroup, once per launch)
  for (int k = threadIdx.x; k < 4 * H; k += 4 * H)
    for (int j = 0; j < H; ++j) wt[j][k] = W[(size_t)k * H + j];
  float bias[4];
#pragma unroll
  for (int gt = 0; gt < 4; ++gt) bias[gt] = bh[gt * H + u];

  float dhc[4], dcc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    dhc[g] = (rowok[g] && d_hlast) ? d_hlast[brow[g] * H + u] : 0.0f;
    dcc[g] = (rowok[g] && d_clast) ? d_clast[brow[g] * H + u] : 0.0f;
  }
  __syncthreads();

  struct Step {
    float gi[4][4];
    float cp[4];
    float dhs[4];
    v4f xa[NC];
  };
  auto load = [&](int t, Step& s) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (rowok[g] && t < lenr[g]) {
        const float* p = gi + ((size_t)t * B + brow[g]) * (4 * H) + u;
        s.gi[g][0] = p[0]; s.gi[g][1] = p[H]; s.gi[g][2] = p[2 * H]; s.gi[g][3] = p[3 * H];
        s.dhs[g] = d_hseq ? d_hseq[((size_t)t * B + brow[g]) * H + u] : 0.0f;
        s.cp[g] = t == 0 ? (c0 ? c0[brow[g] * H + u] : 0.0f) : c_seq[((size_t)(t - 1) * B + brow[g]) * H + u];
      } else {
        s.gi[g][0] = s.gi[g][1] = s.gi[g][2] = s.gi[g][3] = 0.0f;
        s.dhs[g] = s.cp[g] = 0.0f;
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
    v4f acc[4];
#pragma unroll
    for (int gt = 0; gt < 4; ++gt) acc[gt] = v4f{bias[gt], bias[gt], bias[gt], bias[gt]};
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int gt = 0; gt < 4; ++gt) acc[gt] = mfma16(sc.xa[c][e], wf[gt][c][e], acc[gt]);
    float keep[4];                       // dh that a frozen row passes through unchanged (an active row's dh is all dgates . W_hh)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float di = 0.0f, df = 0.0f, dg = 0.0f, dd = 0.0f;
      if (rowok[g] && t < lenr[g]) {
        float dcp;
        lstm_point_bwd(sc.gi[g][0], sc.gi[g][1], sc.gi[g][2], sc.gi[g][3], acc[0][g], acc[1][g], acc[2][g], acc[3][g], sc.cp[g],
                       dhc[g] + sc.dhs[g], dcc[g], di, df, dg, dd, dcp);
        dcc[g] = dcp;
        keep[g] = 0.0f;
      } else {
        keep[g] = dhc[g];
      }
      if (rowok[g]) {
        float* p = dgates + ((size_t)t * B + brow[g]) * (4 * H) + u;
        p[0] = di; p[H] = df; p[2 * H] = dg; p[3 * H] = dd;
      }
      gs[cur][4 * q + g][u] = di;
      gs[cur][4 * q + g][H + u] = df;
      gs[cur][4 * q + g][2 * H + u] = dg;
      gs[cur][4 * q + g][3 * H + u] = dd;
    }
    __syncthreads();
    // dh_{t-1} = dgates_t . W_hh  (four accumulators, one per gate block of the reduction)
    v4f a[4];
    a[0] = v4f{keep[0], keep[1], keep[2], keep[3]};
#pragma unroll
    for (int gt = 1; gt < 4; ++gt) a[gt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < N4; ++c) {
      const v4f x = *reinterpret_cast<const v4f*>(&gs[cur][r][16 * c + 4 * q]);
      const v4f y = *reinterpret_cast<const v4f*>(&wt[u][16 * c + 4 * q]);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[c / NC] = mfma16(x[e], y[e], a[c / NC]);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) dhc[g] = (a[0][g] + a[1][g]) + (a[2][g] + a[3][g]);
    sc = sn;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    if (!rowok[g]) continue;
    if (dh0) dh0[brow[g] * H + u] = dhc[g];
    if (dc0) dc0[brow[g] * H + u] = dcc[g];
    for (int t = tmax; t < T; ++t) {
      float* p = dgates + ((size_t)t * B + brow[g]) * (4 * H) + u;
      p[0] = p[H] = p[2 * H] = p[3 * H] = 0.0f;
    }
  }
}

inline int grid_for(int64_t work) {
  int64_t nb = (work + kBlock - 1) / kBlock;
  return (int)(nb < 1 ? 1 : (nb > 8192 ? 8192 : nb));
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

int gymrl_lstm_cell_fwd(const float* gi, const float* gh, const float* c, int B, int H, float* h_out, float* c_out,
                        void* stream) {
  if (!gi || !gh || !c || !h_out || !c_out || B < 0 || H <= 0 || (H & 3) || !aligned16(gi) || !aligned16(gh) ||
      !aligned16(c) || !aligned16(h_out) || !aligned16(c_out))
    return -22;
  if (B == 0) return 0;
  hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(grid_for((int64_t)B * (H >> 2))), dim3(kBlock), 0, (hipStream_t)stream, gi,
                     gh, c, B, H, h_out, c_out);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_lstm_cell_bwd(const float* gi, const float* gh, const float* c, const float* dh_out, const float* dc_out, int B,
                        int H, float* dgates, float* dc, void* stream) {
  if (!gi || !gh || !c || !dh_out || !dgates || !dc || B < 0 || H <= 0 || (H & 3) || !aligned16(gi) || !aligned16(gh) ||
      !aligned16(c) || !aligned16(dh_out) || (dc_out && !aligned16(dc_out)) || !aligned16(dgates) || !aligned16(dc))
    return -22;
  if (B == 0) return 0;
  hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(grid_for((int64_t)B * (H >> 2))), dim3(kBlock), 0, (hipStream_t)stream, gi,
                     gh, c, dh_out, dc_out, B, H, dgates, dc);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_lstm_seq_fwd(const float* gi, const float* W_hh, const float* b_hh, const float* h0, const float* c0,
                       const int32_t* len, int T, int B, int H, float* h_seq, float* c_seq, float* h_last, float* c_last,
                       void* stream) {
  if (!W_hh || !b_hh || !len || T < 0 || B < 0) return -22;
  if (seq_elems(T, B) && (!gi || !h_seq || !c_seq)) return -22;       // an empty [T,B,*] array may be NULL
  if (H != 16 && H != 32 && H != 48 && H != 64) return -22;
  if (!aligned16(W_hh) || !aligned16(h_seq) || (h0 && !aligned16(h0))) return -22;
  if (!lens_ok(len, B, T)) return -22;
  for (int row0 = 0; row0 < B; row0 += kLaunchRows) {
    const int nrows = B - row0 < kLaunchRows ? B - row0 : kLaunchRows;
    SeqLens L;
    for (int i = 0; i < nrows; ++i) L.len[i] = len[row0 + i];
    const dim3 grid((nrows + kRows - 1) / kRows), block(4 * H);
    hipStream_t s = (hipStream_t)stream;
#define LSTM_SEQ_FWD(HH)                                                                                                 \
  hipLaunchKernelGGL(lstm_seq_fwd_kernel<HH>, grid, block, 0, s, gi, W_hh, b_hh, h0, c0, T, B, row0, nrows, L, h_seq, c_seq, \
                     h_last, c_last)
    switch (H) {
      case 16: LSTM_SEQ_FWD(16); break;
      case 32: LSTM_SEQ_FWD(32); break;
      case 48: LSTM_SEQ_FWD(48); break;
      default: LSTM_SEQ_FWD(64); break;
    }
#undef LSTM_SEQ_FWD
    GYMRL_CHECK_LAUNCH();
  }
  return 0;
}

int gymrl_lstm_seq_bwd(const float* gi, const float* W_hh, const float* b_hh, const float* h0, const float* c0,
                       const float* h_seq, const float* c_seq, const float* d_hseq, const float* d_hlast,
                       const float* d_clast, const int32_t* len, int T, int B, int H, float* dgates, float* dh0, float* dc0,
                       void* stream) {
  if (!W_hh || !b_hh || !len || T < 0 || B < 0) return -22;
  if (seq_elems(T, B) && (!gi || !h_seq || !c_seq || !dgates)) return -22;   // an empty [T,B,*] array may be NULL
  if (H != 16 && H != 32 && H != 48 && H != 64) return -22;
  if (!aligned16(W_hh) || !aligned16(h_seq) || (h0 && !aligned16(h0))) return -22;
  if (!lens_ok(len, B, T)) return -22;
  hipStream_t s = (hipStream_t)stream;
  for (int row0 = 0; row0 < B; row0 += kLaunchRows) {
    const int nrows = B - row0 < kLaunchRows ? B - row0 : kLaunchRows;
    SeqLens L;
    for (int i = 0; i < nrows; ++i) L.len[i] = len[row0 + i];
    const dim3 grid((nrows + kRows - 1) / kRows), block(4 * H);
#define LSTM_SEQ_BWD(HH)                                                                                                \
  hipLaunchKernelGGL(lstm_seq_bwd_kernel<HH>, grid, block, 0, s, gi, W_hh, b_hh, h0, c0, h_seq, c_seq, \
                     d_hseq, d_hlast, d_clast, T, B, row0, nrows, L, dgates, dh0, dc0)
    switch (H) {
      case 16: LSTM_SEQ_BWD(16); break;
      case 32: LSTM_SEQ_BWD(32); break;
      case 48: LSTM_SEQ_BWD(48); break;
      default: LSTM_SEQ_BWD(64); break;
    }
#undef LSTM_SEQ_BWD
    GYMRL_CHECK_LAUNCH();
  }
  return 0;
}

}  // extern "C"
