// mlprnn_act.hip — the acting step of the PPG / PPO-RNN LunarLander trainers as ONE launch per vector step
// (ppg_rnn_lunarlander.py:311-320 choose_action / :322-328 evaluate_action over ActorCriticPPG.forward :165-176;
// ppo_rnn_lunarlander.py the same without the aux head, which acting never reads).
//
//   gymrl_mlprnn_act   PSCN(D, 256) (:92-122) -> MLPRNN(256, 256) = cat(rnn_linear(x), GRU step(x, h)) (:125-140)
//                      -> actor_fc / critic_fc (:156-157) -> softmax -> Categorical draw, log-prob, value
//
// Layout.  A workgroup owns a tile of 16 envs and carries it through the whole chain alone (rows never interact): the
// activations live in LDS, the weights (~165 k floats) stream from global memory / L2 every step.  Every dense layer with
// K % 16 == 0 is a set of 16 x 16 output tiles of v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation; the
// operand mapping of gru_seq.hip: lane (r = lane & 15, q = lane >> 4) feeds X[r][16c + 4q + e] and W[n0 + r][16c + 4q + e]
// and holds rows 4q..4q+3 of column n0 + r).  Tiles are dealt round-robin to the 8 waves; each phase ends with one
// workgroup barrier.  The K = D input layer and the N <= 8 output layers are plain FMA loops.
//   P1  PSCN layer 0 (K = D)                          -> feat[0:128] | x1
//   P2  PSCN layer 1 (x1, 8 tiles) + gh = h W_hh^T + b_hh (12 tiles: h is known from the start)
//   P3  PSCN layer 2 (4 tiles)  P4  PSCN layer 3 (2 tiles)  -> feat[128:256]
//   P5  rnn_linear and W_ih as one 256 -> 384 product (24 tiles)
//   P6  the GRU cell (gru_cell_device.hpp: the bits of gymrl_gru_cell_fwd for the same gi, gh)
//   P7  actor / critic hidden layers (6 tiles)   P8  logits, value   P9  Categorical (clamped_policy_device.hpp) + draw
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gymrl.h"
#include "clamped_policy_device.hpp"
#include "gru_cell_device.hpp"

using namespace gymrl;

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kRows = 16;                  // envs per workgroup = rows of an MFMA tile
constexpr int kWaves = 8;
constexpr int kThreads = 64 * kWaves;
constexpr int kF = 256;                    // PSCN / MLPRNN width
constexpr int kH = 64;                     // GRU hidden size
constexpr int kG = 3 * kH;                 // gate rows
constexpr int kMaxD = 16;
constexpr int kMaxN = 1 << 24;

// LDS row strides (floats): K + 4 keeps the 16-byte row reads of a tile on distinct banks
constexpr int LD_F = kF + 4, LD_H = kH + 4, LD_G = kG + 4, LD_A = 128 + 4, LD_B = 64 + 4, LD_X = kMaxD;
// scratch reused across phases: x (P1) | PSCN layer 1 / 2 outputs (P2-P4) | gi (P5-P6) | head hidden (P7-P8)
constexpr int kScrA = 0, kScrB = kRows * LD_A;
constexpr int kScr = kScrB + kRows * LD_B;
static_assert(kRows * LD_G <= kScr && kRows * 100 <= kScr && kRows * LD_X <= kScrB, "scratch too small");

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

template <int A>
__global__ __launch_bounds__(kThreads) void mlprnn_act_kernel(const float* __restrict__ x, const float* __restrict__ h_in,
                                                              gymrl_mlprnn_params P, int N, int D,
                                                              const uint8_t* __restrict__ live,
                                                              const float* __restrict__ noise_exp, uint64_t seed,
                                                              uint64_t counter, int64_t env_id0, int deterministic,
                                                              float* __restrict__ h_out, int32_t* __restrict__ act_out,
                                                              float* __restrict__ logp_out, float* __restrict__ value_out,
                                                              float* __restrict__ probs_out) {
  __shared__ __attribute__((aligned(16))) float feat[kRows * LD_F];   // PSCN output (the MLPRNN input)
  __shared__ __attribute__((aligned(16))) float outs[kRows * LD_F];   // MLPRNN output (the heads' input)
  __shared__ __attribute__((aligned(16))) float hs[kRows * LD_H];
  __shared__ __attribute__((aligned(16))) float gh[kRows * LD_G];
  __shared__ __attribute__((aligned(16))) float scr[kScr];
  __shared__ float zl[kRows][A + 1];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;

  // P0: inputs (rows past N and features past D are zero)
  float* xs = scr;
  for (int i = tid; i < kRows * kMaxD; i += kThreads) {
    const int rr = i / kMaxD, k = i % kMaxD;
    const int64_t row = row0 + rr;
    xs[rr * LD_X + k] = (row < N && k < D) ? x[row * D + k] : 0.0f;
  }
  for (int i = tid; i < kRows * kH; i += kThreads) {
    const int rr = i / kH, u = i % kH;
    const int64_t row = row0 + rr;
    hs[rr * LD_H + u] = row < N ? h_in[row * kH + u] : 0.0f;
  }
  __syncthreads();

  // P1: PSCN layer 0, D -> 256, PReLU; columns [0, 128) are the first PSCN part, [128, 256) the next layer's input
  {
    const int n = tid % kF, rb = (tid / kF) * (kRows / 2);
    const float a0 = *P.pscn_a[0], bn = P.pscn_b[0][n];
    float wn[kMaxD];
#pragma unroll
    for (int k = 0; k < kMaxD; ++k) wn[k] = k < D ? P.pscn_w[0][(size_t)n * D + k] : 0.0f;
    for (int rr = rb; rr < rb + kRows / 2; ++rr) {
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
  for (int j = w; j < 8 + kG / 16; j += kWaves) {
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
  for (int j = w; j < 4; j += kWaves) {
    const v4f acc = tile_mm<64>(sa + 64, LD_A, P.pscn_w[2], P.pscn_b[2], 16 * j, r, q);
    tile_store(sb, LD_B, 16 * j + r, acc, q, P.pscn_a[2]);
  }
  for (int i = tid; i < kRows * 64; i += kThreads) feat[(i / 64) * LD_F + 128 + i % 64] = sa[(i / 64) * LD_A + i % 64];
  __syncthreads();

  // P4: PSCN layer 3 (32 -> 32) straight into feat[224, 256); layer 2's first half is PSCN part 2
  for (int j = w; j < 2; j += kWaves) {
    const v4f acc = tile_mm<32>(sb + 32, LD_B, P.pscn_w[3], P.pscn_b[3], 16 * j, r, q);
    tile_store(feat, LD_F, 224 + 16 * j + r, acc, q, P.pscn_a[3]);
  }
  for (int i = tid; i < kRows * 32; i += kThreads) feat[(i / 32) * LD_F + 192 + i % 32] = sb[(i / 32) * LD_B + i % 32];
  __syncthreads();

  // P5: rnn_linear (no activation) -> outs[0, 192); gi = feat W_ih^T + b_ih -> scratch
  float* gi = scr;
  for (int j = w; j < 2 * (kG / 16); j += kWaves) {
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

  // P6: the GRU cell -> outs[192, 256) and h_out
  for (int i = tid; i < kRows * kH; i += kThreads) {
    const int rr = i / kH, u = i % kH;
    const float* a = gi + rr * LD_G;
    const float* b = gh + rr * LD_G;
    const float hn = gru_point_fwd(a[u], a[kH + u], a[2 * kH + u], b[u], b[kH + u], b[2 * kH + u], hs[rr * LD_H + u]);
    outs[rr * LD_F + 3 * kH + u] = hn;
    const int64_t row = row0 + rr;
    if (row < N && (!live || live[row])) h_out[row * kH + u] = hn;
  }
  __syncthreads();

  // P7: actor hidden 256 -> 64 (scratch [0, 64)), critic hidden 256 -> 32 (scratch [64, 96)), PReLU each
  float* hh = scr;
  constexpr int LD_HH = 100;
  for (int j = w; j < 6; j += kWaves) {
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

  // P9: Categorical(softmax(logits)) — draw, log-prob, value
  if (tid < kRows) {
    const int64_t row = row0 + tid;
    if (row >= N || (live && !live[row])) return;
    float z[A], p[A], S, p2[A], L[A], c[A];
    bool inb[A];
#pragma unroll
    for (int k = 0; k < A; ++k) z[k] = zl[tid][k];
    clamped_policy<A>(z, p, S, p2, L, c, inb);
    int a = 0;
    if (deterministic) {                               // probs.argmax(): the first maximum
      float best = p[0];
#pragma unroll
      for (int k = 1; k < A; ++k) if (p[k] > best) { best = p[k]; a = k; }
    } else {                                           // torch.multinomial(probs / sum, 1): argmax p2 / q, q ~ Exp(1)
      float qv[A];
      if (noise_exp) {
#pragma unroll
        for (int k = 0; k < A; ++k) qv[k] = noise_exp[row * A + k];
      } else {                                         // the keys of gymrl_categorical_sample (policy_device.hpp)
        const uint64_t env = (uint64_t)(env_id0 + row);
#pragma unroll
        for (int blk = 0; blk < (A + 3) / 4; ++blk) {
          const u32x4 rn = philox4x32(seed, (uint32_t)env, (uint32_t)(env >> 32), (uint32_t)counter,
                                      RNG_POLICY | ((uint32_t)((counter >> 32) & 0x3FFFFFu) << 2) | (uint32_t)blk);
          const uint32_t wv[4] = {rn.x, rn.y, rn.z, rn.w};
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (blk * 4 + k < A) qv[blk * 4 + k] = -det_logf(u01f_open0(wv[k]));
        }
      }
      float best = p2[0] / qv[0];
#pragma unroll
      for (int k = 1; k < A; ++k) {
        const float cand = p2[k] / qv[k];
        if (cand > best) { best = cand; a = k; }
      }
    }
    float lp = L[0];
#pragma unroll
    for (int k = 1; k < A; ++k) if (a == k) lp = L[k];
    act_out[row] = a;
    logp_out[row] = lp;
    value_out[row] = zl[tid][A];
    if (probs_out) {
#pragma unroll
      for (int k = 0; k < A; ++k) probs_out[row * A + k] = p[k];
    }
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" {

size_t gymrl_mlprnn_params_bytes(void) { return sizeof(gymrl_mlprnn_params); }

int gymrl_mlprnn_act(const float* x, const float* h_in, const gymrl_mlprnn_params* params, int N, int D, int A,
                     const uint8_t* live, const float* noise_exp, uint64_t seed, uint64_t counter, int64_t env_id0,
                     int deterministic, float* h_out, int32_t* act, float* logp, float* value, float* probs,
                     void* stream_) {
  if (!x || !h_in || !params || !h_out || !act || !logp || !value) return -22;
  if (N < 0 || N > kMaxN || D < 1 || D > kMaxD || A < 2 || A > 8) return -22;
  const gymrl_mlprnn_params& P = *params;
  for (int i = 0; i < 4; ++i)
    if (!P.pscn_w[i] || !P.pscn_b[i] || !P.pscn_a[i]) return -22;
  const void* req[] = {P.lin_w, P.lin_b, P.w_ih, P.b_ih, P.w_hh, P.b_hh, P.actor_w1, P.actor_b1, P.actor_a, P.actor_w2,
                       P.actor_b2, P.critic_w1, P.critic_b1, P.critic_a, P.critic_w2, P.critic_b2};
  for (const void* p : req)
    if (!p) return -22;
  // the tiles read these with 16-byte loads
  const void* v4[] = {P.pscn_w[1], P.pscn_w[2], P.pscn_w[3], P.lin_w, P.w_ih, P.w_hh, P.actor_w1, P.critic_w1};
  for (const void* p : v4)
    if (!al16(p)) return -22;
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream_;
  const dim3 grid((N + kRows - 1) / kRows), block(kThreads);
#define MLPRNN_CASE(AA)                                                                                                   \
  case AA:                                                                                                                \
    hipLaunchKernelGGL(mlprnn_act_kernel<AA>, grid, block, 0, s, x, h_in, P, N, D, live, noise_exp, seed, counter,      \
                       env_id0, deterministic, h_out, act, logp, value, probs);                                           \
    break;
  switch (A) {
    MLPRNN_CASE(2) MLPRNN_CASE(3) MLPRNN_CASE(4) MLPRNN_CASE(5) MLPRNN_CASE(6) MLPRNN_CASE(7) MLPRNN_CASE(8)
    default: return -22;
  }
#undef MLPRNN_CASE
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
