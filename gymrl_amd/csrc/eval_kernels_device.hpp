// eval_kernels_device.hpp — the two episode kernels of the classic-control policy evaluation, stated once per network shape:
//
//   classic_eval_kernel   a three-layer MLP D -> H -> H -> A under an argmax head (CartPole-v1, MountainCar-v0, Acrobot-v1) or a tanh head
//                         (Pendulum-v1)
//   duel_eval_kernel      a dueling network: a ReLU trunk of one or two layers, a value head and an advantage head in ONE
//                         two-item stage, the combine, the first maximum (CartPole-v1, MountainCar-v0, Acrobot-v1)
//
// Both are templates over the env kind (EpisodeEnv<KIND>, env_classic_device.hpp: the widths and the action type) and the
// ARGUMENT BLOCK of the entry point that launches them: eval_classic.hip (gymrl_classic_eval_args), eval_duel.hip
// (gymrl_classic_duel_eval_args) and eval_net.hip (gymrl_mountaincar_net_eval_args, gymrl_acrobot_net_eval_args: one set of
// fields) name the same tensors differently, and mlp3_of / duel_of below read them out.  The episode loop is
// eval_episode_device.hpp's run_episodes; what is stated here is one step's policy forward and its action.
//
// Register pressure: the tensors' pointers pass through an empty asm inside the forward, so that the stages' per-lane operand
// addresses are formed again in every iteration — hoisted out of the loop they were 47 spilled registers, reloaded from scratch
// memory step by step.
#pragma once
#include <type_traits>
#include "duel_device.hpp"
#include "eval_episode_device.hpp"

namespace gymrl {
namespace slab {
namespace {

constexpr int kHeadArgmax = 0, kHeadTanh = 1;
constexpr int kCombineMean = 1, kCombineRow = 2;       // duel_combine (torch's mean) | dueling_row (Rainbow's epilogue)

// policy 0's tensors as the kernels name them: a block with head_w (the net entry points': fc3 or the advantage head), or the
// CartPole / Pendulum blocks' own names
struct Mlp3 { const float *w0, *w1, *w2, *b0, *b1, *b2; };
__device__ __forceinline__ Mlp3 mlp3_of(const gymrl_classic_eval_args& a) { return Mlp3{a.w[0], a.w[1], a.w[2], a.b[0], a.b[1], a.b[2]}; }
template <class Args>
__device__ __forceinline__ Mlp3 mlp3_of(const Args& a) { return Mlp3{a.w[0], a.w[1], a.head_w, a.b[0], a.b[1], a.head_b}; }
struct DuelNet { const float *w0, *b0, *w1, *b1, *wv, *bv, *wa, *ba; };
__device__ __forceinline__ DuelNet duel_of(const gymrl_classic_duel_eval_args& a) { return DuelNet{a.w[0], a.b[0], a.w[1], a.b[1], a.value_w, a.value_b, a.adv_w, a.adv_b}; }
template <class Args>
__device__ __forceinline__ DuelNet duel_of(const Args& a) { return DuelNet{a.w[0], a.b[0], a.w[1], a.b[1], a.value_w, a.value_b, a.head_w, a.head_b}; }

// KIND: an env whose Action is an index (the first maximum of fc3's row) or a float (Pendulum-v1: tanh * a.bound);
// HC: the hidden width the instance is built for (0: a.H)
template <int HC, int KIND, class Args>
__global__ __launch_bounds__(kThreads) void classic_eval_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ int running;                 // the loop's exit word: written by wave 0, read by everybody behind the barrier
  const Lds L;
  using Env = EpisodeEnv<KIND>;
  constexpr bool argmax = std::is_same<typename Env::Action, int>::value;
  constexpr int D = Env::kObs, A = Env::kActions;
  const int H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int X0 = L.big, X1 = X0 + 16 * ld;
  const int groups = (a.E + 15) / 16;
  const int p = (int)blockIdx.x / groups, e0 = ((int)blockIdx.x - p * groups) * 16, nrows = min(16, a.E - e0);
  const size_t shift = (size_t)p * (size_t)a.policy_stride;
  const Mlp3 net = mlp3_of(a);
  const float *w0 = net.w0 + shift, *w1 = net.w1 + shift, *w2 = net.w2 + shift;
  const float *b0 = net.b0 + shift, *b1 = net.b1 + shift, *b2 = net.b2 + shift;
  const float* img = (a.images && (H & 15) == 0) ? a.images : nullptr;
  const int R = GYMRL_ACT_RELU, kD = kMaxD, kA = kMaxA;
  run_episodes<KIND>(
      a, lds + L.S, kD, running, p, e0, nrows,
      [=]() {
        const float *v0 = w0, *v1 = w1, *v2 = w2, *c0 = b0, *c1 = b1, *c2 = b2, *im = img;
        // (the pointers pass through an empty asm: see the register-pressure note at the head of this file)
        asm volatile("" : "+s"(v0), "+s"(v1), "+s"(v2), "+s"(c0), "+s"(c1), "+s"(c2), "+s"(im));
        fwd_one(lds, {fwd_item(L.S, kD, -1, 0, D, D, H, v0, c0, X0, ld, nullptr, 0, R)}, 0, nrows);
        fwd_one(lds, {fwd_item(X0, ld, -1, 0, H, H, H, v1, c1, X1, ld, nullptr, 0, R, 0.0f, 0.0f, im)}, 0, nrows);
        fwd_one(lds, {fwd_item(X1, ld, -1, 0, H, H, A, v2, c2, L.Mean, kA, nullptr, 0, argmax ? GYMRL_ACT_NONE : GYMRL_ACT_TANH)}, 0, nrows);
      },
      [=](int t) {
        if constexpr (argmax) {
          // the greedy branch of epsilon_greedy_pick (u0 = 1 is never below epsilon = 0): the first maximum, no draw
          const float never[2] = {1.0f, 0.0f};
          return epsilon_greedy_pick(lds + L.Mean + t * kMaxA, A, never, 0ull, 0ull, 0ull, 0.0f);
        } else {
          return lds[L.Mean + t * kMaxA] * a.bound;
        }
      });
}

// NH: hidden layers of the trunk (1 | 2); HC: the hidden width the instance is built for (0: a.H); COMBINE: kCombineMean |
// kCombineRow.  With two actions the two combines are the same floats (sum / 2 == sum * 0.5f) and kCombineMean serves both.
template <int HC, int NH, int KIND, int COMBINE, class Args>
__global__ __launch_bounds__(kThreads) void duel_eval_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ int running;                 // the loop's exit word: written by wave 0, read by everybody behind the barrier
  const Lds L;
  constexpr int D = EpisodeEnv<KIND>::kObs, A = EpisodeEnv<KIND>::kActions;
  const int H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int X0 = L.big, X1 = X0 + 16 * ld, Xh = NH == 2 ? X1 : X0;       // Xh: the slab the heads read
  const int groups = (a.E + 15) / 16;
  const int p = (int)blockIdx.x / groups, e0 = ((int)blockIdx.x - p * groups) * 16, nrows = min(16, a.E - e0);
  const size_t shift = (size_t)p * (size_t)a.policy_stride;
  const DuelNet net = duel_of(a);
  const float *w0 = net.w0 + shift, *b0 = net.b0 + shift;
  const float *w1 = NH == 2 ? net.w1 + shift : nullptr, *b1 = NH == 2 ? net.b1 + shift : nullptr;
  const float *wv = net.wv + shift, *bv = net.bv + shift, *wa = net.wa + shift, *ba = net.ba + shift;
  const float* img = (NH == 2 && a.images && (H & 15) == 0) ? a.images : nullptr;
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD;
  run_episodes<KIND>(
      a, lds + L.S, kD, running, p, e0, nrows,
      [=]() {
        const float *v0 = w0, *c0 = b0, *v1 = w1, *c1 = b1, *vv = wv, *cv = bv, *va = wa, *ca = ba, *im = img;
        // (the pointers pass through an empty asm: see the register-pressure note at the head of this file)
        asm volatile("" : "+s"(v0), "+s"(c0), "+s"(v1), "+s"(c1), "+s"(vv), "+s"(cv), "+s"(va), "+s"(ca), "+s"(im));
        fwd_one(lds, {fwd_item(L.S, kD, -1, 0, D, D, H, v0, c0, X0, ld, nullptr, 0, R)}, 0, nrows);
        if constexpr (NH == 2) fwd_one(lds, {fwd_item(X0, ld, -1, 0, H, H, H, v1, c1, X1, ld, nullptr, 0, R, 0.0f, 0.0f, im)}, 0, nrows);
        const FwdItem st[2] = {fwd_item(Xh, ld, -1, 0, H, H, 1, vv, cv, L.Cq1, 4, nullptr, 0, NA),
                               fwd_item(Xh, ld, -1, 0, H, H, A, va, ca, L.Cq0, 4, nullptr, 0, NA)};
        fwd_stage<2>(lds, st, 0, nrows);
        __syncthreads();
      },
      [=](int t) {
        float q[kMaxA];
        if constexpr (COMBINE == kCombineRow) {
          // the row of Rainbow's stacked head: the advantages, then the value
          float z[kMaxA + 1] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
          for (int k = 0; k < A; ++k) z[k] = lds[L.Cq0 + t * 4 + k];
          z[A] = lds[L.Cq1 + t * 4];
          return dueling_row(z, A, q);
        } else {
          duel_combine(lds + L.Cq0 + t * 4, lds[L.Cq1 + t * 4], A, q);
          int act = 0;
          float best = q[0];
          for (int k = 1; k < A; ++k) if (q[k] > best) { best = q[k]; act = k; }
          return act;
        }
      });
}

}  // namespace
}  // namespace slab
}  // namespace gymrl
