// mlprnn_device.hpp — the PSCN -> MLPRNN (GRU) -> heads forward of the PPG / PPO-RNN networks for a tile of 16 rows in LDS,
// stated once: the acting step (mlprnn_act.hip, 8 waves, one step per launch) and the one-launch LunarLander evaluation
// (eval_lunar_rnn.hip, one step per iteration of its episode loop, the hidden state staying in the tile) call it.
//
// Layout.  The activations live in LDS, the weights (~165 k floats) stream from global memory / L2 every step.  Every dense
// layer with K % 16 == 0 is a set of 16 x 16 output tiles of v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation; the
// operand mapping of gru_seq.hip: lane (r = lane & 15, q = lane >> 4) feeds X[r][16c + 4q + e] and W[n0 + r][16c + 4q + e]
// and holds rows 4q..4q+3 of column n0 + r).  Tiles are dealt round-robin to the WAVES waves of the workgroup; each phase ends
// with one workgroup barrier.  The K = D input layer and the N <= 8 output layers are plain FMA loops.  Which wave or thread
// computes an output element changes with WAVES, its arithmetic does not: every element is one thread's sum in a fixed order.
//   P1  PSCN layer 0 (K = D)                          -> feat[0:128] | x1
//   P2  PSCN layer 1 (x1, 8 tiles) + gh = h W_hh^T + b_hh (12 tiles: h is known from the start)
//   P3  PSCN layer 2 (4 tiles)  P4  PSCN layer 3 (2 tiles)  -> feat[128:256]
//   P5  rnn_linear and W_ih as one 256 -> 384 product (24 tiles)
//   P6  the GRU cell (gru_cell_device.hpp: the bits of gymrl_gru_cell_fwd for the same gi, gh)
//   P7  actor / critic hidden layers (6 tiles)   P8  logits, value
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gymrl.h"
#include "gru_cell_device.hpp"

namespace gymrl {
namespace mlprnn {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kRows = 16;                  // rows per workgroup = rows of an MFMA tile
constexpr int kF = 256;                    // PSCN / MLPRNN width
constexpr int kH = 64;                     // GRU hidden size
constexpr int kG = 3 * kH;                 // gate rows
constexpr int kMaxD = 16;

// LDS row strides (floats): K + 4 keeps the 16-byte row reads of a tile on distinct banks
constexpr int LD_F = kF + 4, LD_H = kH + 4, LD_G = kG + 4, LD_A = 128 + 4, LD_B = 64 + 4, LD_X = kMaxD;
// scratch reused across phases: PSCN layer 1 / 2 outputs (P2-P4) | gi (P5-P6) | head hidden (P7-P8)
constexpr int kScrA = 0, kScrB = kRows * LD_A;
constexpr int kScr = kScrB + kRows * LD_B;
static_assert(kRows * LD_G <= kScr && kRows * 100 <= kScr && kRows * LD_X <= kScrB, "scratch too small");

// The forward's tiles.  hs is the hidden state the step starts from; outs[.][192:256) holds the new one.
struct Tiles {
  float* feat;   // [kRows][LD_F]  PSCN output (the MLPRNN input)
  float* outs;   // [kRows][LD_F]  MLPRNN output (the heads' input)
  float* hs;     // [kRows][LD_H]  hidden state
  float* gh;     // [kRows][LD_G]
  float* scr;    // [kScr]
};
constexpr int kTileFloats = 2 * kRows * LD_F + kRows * LD_H + kRows * LD_G + kScr;
__device__ __forceinline__ Tiles carve(float* base) {       // `base` 16-byte aligned: every tile then is
  Tiles t;
  t.feat = base;
  t.outs = t.feat + kRows * LD_F;
  t.hs = t.outs + kRows * LD_F;
  t.gh = t.hs + kRows * LD_H;
  t.scr = t.gh + kRows * LD_G;
  return t;
}

__device__ __forceinline__ v4f mfma16(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ float prelu(float v, float a) { return v > 0.0f ? v : a * v; }

// acc[g] = b[n0 + r] + sum_k X[4q + g][k] W[n0 + r][k] for one 16 x 16 output tile (K % 16 == 0, W row-major [N][K])
template <int K>
__device__ __forceinline__ v4f tile_mm(const float* __restrict__ X, int ldx, const float* __restrict__ W,
                                       const float* __restrict__ b, int n0, int r, int q) {
  const float bias = b[n0 + r];
  v4f acc = {bias, bias, bias, bias};
  const float* wrow = W + (size_t)(n0 + r) * K + 4 * q;
  const float* xrow = X + r * ldx + 4 * q;
#pragma unroll 4
  for (int c = 0; c < K / 16; ++c) {
    const v4f wv = *reinterpret_cast<const v4f*>(wrow + 16 * c);
    const v4f xv = *reinterpret_cast<const v4f*>(xrow + 16 * c);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = mfma16(xv[e], wv[e], acc);
  }
  return acc;
}

// Y[4q + g][col] = act(acc[g]); slope == nullptr: no activation
__device__ __forceinline__ void tile_store(float* __restrict__ Y, int ldy, int col, v4f acc, int q, const float* slope) {
  const float a = slope ? *slope : 0.0f;
#pragma unroll
  for (int g = 0; g < 4; ++g) Y[(4 * q + g) * ldy + col] = slope ? prelu(acc[g], a) : acc[g];
}

// P1-P8 for the 16 rows of xs [kRows][LD_X] (features past D are not read) and t.hs, both complete behind a barrier when
// every thread of the workgroup of 64 * WAVES threads calls this.  -> zl[row] = A logits, then the value; the new hidden
// state in t.outs[row][192:256) and handed to keep_h(row, unit, h) by the one thread that read t.hs[row][unit] for it: the
// caller stores it (the acting step's h_out) or writes it back into t.hs (an episode loop).  Closed by a barrier.  xs may be
// t.scr: it is last read in P1, the scratch first written in P2.
template <int WAVES, int A, class KeepH>
__device__ __forceinline__ void forward_tile(const gymrl_mlprnn_params& P, const int D, const float* xs, const Tiles& t,
                                             float (*zl)[A + 1], KeepH&& keep_h) {
  constexpr int kThreads = 64 * WAVES;
  static_assert(kThreads % kF == 0 && kRows % (kThreads / kF) == 0, "P1 deals whole rows of 256 columns");
  static_assert(kThreads >= kRows * (A + 1), "P8: one thread per output");
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  float* const feat = t.feat;
  float* const outs = t.outs;
  float* const hs = t.hs;
  float* const gh = t.gh;
  float* const scr = t.scr;

  // P1: PSCN layer 0, D -> 256, PReLU; columns [0, 128) are the first PSCN part, [128, 256) the next layer's input
  {
    constexpr int kRowsEach = kRows / (kThreads / kF);
    const int n = tid % kF, rb = (tid / kF) * kRowsEach;
    const float a0 = *P.pscn_a[0], bn = P.pscn_b[0][n];
    float wn[kMaxD];
#pragma unroll
    for (int k = 0; k < kMaxD; ++k) wn[k] = k < D ? P.pscn_w[0][(size_t)n * D + k] : 0.0f;
    for (int rr = rb; rr < rb + kRowsEach; ++rr) {
      float s = bn;
#pragma unroll
      for (int k = 0; k < kMaxD; ++k)
        if (k < D) s += xs[rr * LD_X + k] * wn[k];
      feat[rr * LD_F + n] = prelu(s, a0);
    }
  }
  __syncthreads();

  // P2: PSCN layer 1 (128 -> 128) into scratch A, and gh = h W_hh^T + b_hh
  float* sa = scr + kScrA;
  float* sb = scr + kScrB;
  for (int j = w; j < 8 + kG / 16; j += WAVES) {
    if (j < 8) {
      const v4f acc = tile_mm<128>(feat + 128, LD_F, P.pscn_w[1], P.pscn_b[1], 16 * j, r, q);
      tile_store(sa, LD_A, 16 * j + r, acc, q, P.pscn_a[1]);
    } else {
      const int n0 = 16 * (j - 8);
      const v4f acc = tile_mm<kH>(hs, LD_H, P.w_hh, P.b_hh, n0, r, q);
      tile_store(gh, LD_G, n0 + r, acc, q, nullptr);
    }
  }
  __syncthreads();

  // P3: PSCN layer 2 (64 -> 64) from the second half of layer 1; the first half is PSCN part 1
  for (int j = w; j < 4; j += WAVES) {
    const v4f acc = tile_mm<64>(sa + 64, LD_A, P.pscn_w[2], P.pscn_b[2], 16 * j, r, q);
    tile_store(sb, LD_B, 16 * j + r, acc, q, P.pscn_a[2]);
  }
  for (int i = tid; i < kRows * 64; i += kThreads) feat[(i / 64) * LD_F + 128 + i % 64] = sa[(i / 64) * LD_A + i % 64];
  __syncthreads();

  // P4: PSCN layer 3 (32 -> 32) straight into feat[224, 256); layer 2's first half is PSCN part 2
  for (int j = w; j < 2; j += WAVES) {
    const v4f acc = tile_mm<32>(sb + 32, LD_B, P.pscn_w[3], P.pscn_b[3], 16 * j, r, q);
    tile_store(feat, LD_F, 224 + 16 * j + r, acc, q, P.pscn_a[3]);
  }
  for (int i = tid; i < kRows * 32; i += kThreads) feat[(i / 32) * LD_F + 192 + i % 32] = sb[(i / 32) * LD_B + i % 32];
  __syncthreads();

  // P5: rnn_linear (no activation) -> outs[0, 192); gi = feat W_ih^T + b_ih -> scratch
  float* gi = scr;
  for (int j = w; j < 2 * (kG / 16); j += WAVES) {
    if (j < kG / 16) {
      const v4f acc = tile_mm<kF>(feat, LD_F, P.lin_w, P.lin_b, 16 * j, r, q);
      tile_store(outs, LD_F, 16 * j + r, acc, q, nullptr);
    } else {
      const int n0 = 16 * (j - kG / 16);
      const v4f acc = tile_mm<kF>(feat, LD_F, P.w_ih, P.b_ih, n0, r, q);
      tile_store(gi, LD_G, n0 + r, acc, q, nullptr);
    }
  }
  __syncthreads();

  // P6: the GRU cell -> outs[192, 256)
  for (int i = tid; i < kRows * kH; i += kThreads) {
    const int rr = i / kH, u = i % kH;
    const float* a = gi + rr * LD_G;
    const float* b = gh + rr * LD_G;
    const float hn = gru_point_fwd(a[u], a[kH + u], a[2 * kH + u], b[u], b[kH + u], b[2 * kH + u], hs[rr * LD_H + u]);
    outs[rr * LD_F + 3 * kH + u] = hn;
    keep_h(rr, u, hn);
  }
  __syncthreads();

  // P7: actor hidden 256 -> 64 (scratch [0, 64)), critic hidden 256 -> 32 (scratch [64, 96)), PReLU each
  float* hh = scr;
  constexpr int LD_HH = 100;
  for (int j = w; j < 6; j += WAVES) {
    if (j < 4) {
      const v4f acc = tile_mm<kF>(outs, LD_F, P.actor_w1, P.actor_b1, 16 * j, r, q);
      tile_store(hh, LD_HH, 16 * j + r, acc, q, P.actor_a);
    } else {
      const int n0 = 16 * (j - 4);
      const v4f acc = tile_mm<kF>(outs, LD_F, P.critic_w1, P.critic_b1, n0, r, q);
      tile_store(hh, LD_HH, 64 + n0 + r, acc, q, P.critic_a);
    }
  }
  __syncthreads();

  // P8: logits 64 -> A, value 32 -> 1
  if (tid < kRows * (A + 1)) {
    const int rr = tid / (A + 1), k = tid % (A + 1);
    const float* hrow = hh + rr * LD_HH;
    float s;
    if (k < A) {
      s = P.actor_b2[k];
      for (int i = 0; i < 64; ++i) s += hrow[i] * P.actor_w2[k * 64 + i];
    } else {
      s = P.critic_b2[0];
      for (int i = 0; i < 32; ++i) s += hrow[64 + i] * P.critic_w2[i];
    }
    zl[rr][k] = s;
  }
  __syncthreads();
}

// What every entry point refuses in a parameter table before its first HIP call: a NULL member, and a weight the tiles read
// with 16-byte loads that is not 16-byte aligned.
inline bool params_ok(const gymrl_mlprnn_params* params) {
  if (!params) return false;
  const gymrl_mlprnn_params& P = *params;
  for (int i = 0; i < 4; ++i)
    if (!P.pscn_w[i] || !P.pscn_b[i] || !P.pscn_a[i]) return false;
  const void* req[] = {P.lin_w, P.lin_b, P.w_ih, P.b_ih, P.w_hh, P.b_hh, P.actor_w1, P.actor_b1, P.actor_a, P.actor_w2,
                       P.actor_b2, P.critic_w1, P.critic_b1, P.critic_a, P.critic_w2, P.critic_b2};
  for (const void* p : req)
    if (!p) return false;
  const void* v4[] = {P.pscn_w[1], P.pscn_w[2], P.pscn_w[3], P.lin_w, P.w_ih, P.w_hh, P.actor_w1, P.critic_w1};
  for (const void* p : v4)
    if (((uintptr_t)p & 15u) != 0) return false;
  return true;
}

}  // namespace
}  // namespace mlprnn
}  // namespace gymrl
