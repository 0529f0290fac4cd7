// value_step_device.hpp — what the row-slab steps of the discrete value learners share on top of slab_step_device.hpp:
// dqn_step.hip (DQN), ddqn_step.hip (DDQN + PER, plain and dueling), noisy_dqn_step.hip (NoisyNet dueling DQN) and, for the
// act kernels' observation load, dsac_step.hip (discrete SAC).  Each piece is stated ONCE and what the algorithms differ in
// is a parameter of it: which ring row a batch lane reads and whether it is checked against the ring (`checked`), the row's
// weight (RowWeight), which Q row picks the greedy action (td_row's sel), what lies under the dueling heads (duel_heads_segment).
// Everything is __forceinline__ device code or inline host code inside an anonymous namespace, as in slab_step_device.hpp.
#pragma once
#include "duel_device.hpp"
#include "policy_device.hpp"
#include "slab_step_device.hpp"

namespace gymrl {
namespace slab {
namespace {

// `images` of a three-layer Q network's update, f32[3][H*H]: two forward images (policy, target), then the policy net's
// input-gradient image.  Args: gymrl_dqn_update_args or gymrl_ddqn_update_args (the same layout).
struct QNet3Images {
  const float *pf, *tf, *pb;
  __host__ __device__ QNet3Images(const float* base, int H) {
    const ImageSlots at(base, H);
    pf = at(0); tf = at(1); pb = at(2);
  }
  static constexpr int kCount = 3;
  template <class Args>
  static PackTable sources(const Args& a) {
    return PackTable{{a.policy.w[1], a.target.w[1], a.policy.w[1], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, 2};
  }
};

// hand-off between the row phase and the tile phase of a three-layer Q network's update (caller-owned workspace)
struct QNet3Ws {
  float* s;                            // [B][D]: the gathered states
  float *H1, *Z1, *H2, *Z2, *dq;       // the policy net's activations on s and dL/dz per layer ([B][H]; dq [B][A]); the dueling
                                       // instance has one hidden layer: H2 holds dv [B], dq holds da [B][A], Z2 is unused
  double* terms;                       // [B][3]: the row's td^2 (* w) in column 0 (sac_dw_body's row pitch)
  __host__ __device__ static size_t carve(QNet3Ws* w, void* base, int B, int D, int A, int H) {
    carve_taker take{base};
    float* s = take((size_t)B * D);
    float* h[4];
    for (int i = 0; i < 4; ++i) h[i] = take((size_t)B * H);
    float* dq = take((size_t)B * A);
    double* terms = reinterpret_cast<double*>(take((size_t)B * 6));
    if (w) { w->s = s; w->H1 = h[0]; w->Z1 = h[1]; w->H2 = h[2]; w->Z2 = h[3]; w->dq = dq; w->terms = terms; }
    return take.off;
  }
};

// The ring row of a batch lane CHECKED against the ring, or -1 for a ZERO ROW: a lane beyond the batch (draw() is not called for
// it) or a row outside [0, cap).  Such a row is never read: it enters the batch as zeros with weight 0 (td_out = -y of a zero
// row, no gradient), instead of a read outside the ring.  draw(): idx[b] for DDQN's sampled rows, replay_draw_row for NoisyNet.
// DQN does not check — its rows come from the keyed draw over the ring's size or from a caller who owns the ring — and says
// `in_batch ? replay_draw_row : -1` itself.
template <class Draw>
__device__ __forceinline__ int64_t checked_ring_row(bool in_batch, Draw draw, int64_t cap) {
  if (!in_batch) return -1;
  const int64_t row = draw();
  return (row >= 0 && row < cap) ? row : -1;
}

// slot 3 of the row's L.Misc: not written (DQN), 1 (NoisyNet: no weights, but a zero row weighs
// 0), or is_weight[b] (DDQN + PER)
enum class RowWeight { kNone, kUnit, kGiven };

// The gather of lane t < 16: ring row `row` (-1: zeros) -> L.S (state), L.S2 (next state), L.Misc {reward,
// done as float32, the action word's bits, the weight} and, for a lane in the batch, the state to s_out[b] for the tile phase.
// checked: the row comes from checked_ring_row, so a lane in the batch may still hold -1.  This is the ONE flag of the check.
// An unchecked row (DQN) is a zero row exactly where the lane is beyond the batch, and saying so keeps the loads and the s_out
// store under ONE predicate: with `row >= 0` for both, dqn_r1_kernel came out 50-70 instructions longer and its step 1 % slower
// at N = 64 (DESIGN 4m').
template <class Args>
__device__ __forceinline__ void gather_ring_row(const Args& a, float* lds, const Lds& L, int t, int b, bool in_batch, int64_t row, bool checked,
                                                float* s_out, RowWeight weight = RowWeight::kNone, const float* is_weight = nullptr) {
  const int D = a.D;
  const bool ok = checked ? row >= 0 : in_batch;
  for (int k = 0; k < kMaxD; ++k) {
    const float sv = (ok && k < D) ? a.r_state[row * D + k] : 0.0f;
    lds[L.S + t * kMaxD + k] = sv;
    lds[L.S2 + t * kMaxD + k] = (ok && k < D) ? a.r_next[row * D + k] : 0.0f;
    if (in_batch && k < D) s_out[(size_t)b * D + k] = sv;
  }
  lds[L.Misc + t * 4 + 0] = ok ? a.r_reward[row] : 0.0f;
  lds[L.Misc + t * 4 + 1] = ok ? (float)a.r_flag[row] : 0.0f;            // dones become float32
  lds[L.Misc + t * 4 + 2] = ok ? __int_as_float((int)a.r_action[row]) : 0.0f;
  if (weight != RowWeight::kNone) lds[L.Misc + t * 4 + 3] = !ok ? 0.0f : weight == RowWeight::kUnit ? 1.0f : is_weight[b];
}

// offpolicy.hip dqn_td_kernel on one row: q = Q(s), qt = target Q(s'), sel = the row whose FIRST maximum is a* (qt itself for
// DQN: qn_online == nullptr; the online Q(s') for the double-Q learners); misc = the row's {reward, done, action word};
// wb = the row's weight (DQN: the literal 1.0f, w == nullptr).  -> td, dq = dL/dq (2 td w / B at the taken action); returns td^2 w.
// BY_LOOP: q and qt are register arrays (the dueling kernels' combine outputs), which a run-time index would send to scratch:
// nq and qa are selected by a loop over k.  Otherwise they are LDS rows and are indexed.  (One form for both changes the
// compiled kernels: the loop reads whole rows from LDS, the index spills the arrays.)
template <bool BY_LOOP>
__device__ __forceinline__ float td_row(const float* q, const float* qt, const float* sel, int A, const float* misc, float gamma, float wb, float invB,
                                        float& td, float (&dq)[4]) {
  int astar = 0;
  float best = sel[0];
  for (int k = 1; k < A; ++k) if (sel[k] > best) { best = sel[k]; astar = k; }
  const int act = __float_as_int(misc[2]);
  float nq, qa;
  if (BY_LOOP) {
    nq = qt[0]; qa = q[0];
    for (int k = 1; k < A; ++k) { if (k == astar) nq = qt[k]; if (k == act) qa = q[k]; }
  } else {
    nq = qt[astar]; qa = q[act];
  }
  const float y = misc[0] + gamma * nq * (1.0f - misc[1]);
  td = qa - y;
  for (int k = 0; k < 4; ++k) dq[k] = k == act ? (2.0f * td) * wb * invB : 0.0f;
  return (td * td) * wb;
}

// ---- the dueling heads over three chains, the loss, and the way back to the layer under the heads ----
// X[c]: the [16][ld] slab the heads of chain c read — c = 0 policy(s), 1 policy(s') (it picks a*), 2 target(s') —, and hp[c] its
// value (1 column) and advantage (A columns) layers.  Six items of ONE stage; the three combines; td_row with the row's weight
// from L.Misc[3]; duel_combine_bwd; dv -> dv_out [B], da -> da_out [B][A], td -> td_out (nullptr: none), td^2 w -> terms; then
// each head's input gradient on its own (two backward launches on the layer path) into Xv / Xa — slabs that are dead by then —,
// autograd's sum of the two, and the ReLU derivative of the layer below from its saved output X[0]: dL/dz of that layer goes to
// Zg [B][H] and, where another stage follows (Zs >= 0: NoisyNet's fc2 -> fc1), to the LDS slab Zs.  No barrier behind it.
struct DuelHeads { const float *wv, *bv, *wa, *ba; };
__device__ __forceinline__ void duel_heads_segment(float* lds, const Lds& L, int A, int H, int ld, int row0, int nrows, float gamma, int B,
                                                   const int (&X)[3], const DuelHeads (&hp)[3], int Xv, int Xa, float* dv_out, float* da_out,
                                                   float* td_out, double* terms, int Zs, float* Zg) {
  const int t = threadIdx.x;
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE;
  {                                       // value (1 column) and advantage (A columns) of every chain: six items of one stage
    const FwdItem st[6] = {fwd_item(X[0], ld, -1, 0, H, H, 1, hp[0].wv, hp[0].bv, L.Cq1, 4, nullptr, 0, NA),
                           fwd_item(X[0], ld, -1, 0, H, H, A, hp[0].wa, hp[0].ba, L.Cq0, 4, nullptr, 0, NA),
                           fwd_item(X[1], ld, -1, 0, H, H, 1, hp[1].wv, hp[1].bv, L.Dq1, 4, nullptr, 0, NA),
                           fwd_item(X[1], ld, -1, 0, H, H, A, hp[1].wa, hp[1].ba, L.Q1, 4, nullptr, 0, NA),
                           fwd_item(X[2], ld, -1, 0, H, H, 1, hp[2].wv, hp[2].bv, L.Mean, 4, nullptr, 0, NA),
                           fwd_item(X[2], ld, -1, 0, H, H, A, hp[2].wa, hp[2].ba, L.Q0, 4, nullptr, 0, NA)};
    fwd_stage<6>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 16) {                           // the three combines, then dqn_td_kernel with qn_online (and w) set, then the combine's backward
    float q[4], qo[4], qt[4];
    duel_combine(lds + L.Cq0 + t * 4, lds[L.Cq1 + t * 4], A, q);
    duel_combine(lds + L.Q1 + t * 4, lds[L.Dq1 + t * 4], A, qo);
    duel_combine(lds + L.Q0 + t * 4, lds[L.Mean + t * 4], A, qt);
    float td, dq[4], da[4], dv;
    const float term = td_row<true>(q, qt, qo, A, lds + L.Misc + t * 4, gamma, lds[L.Misc + t * 4 + 3], 1.0f / (float)B, td, dq);
    duel_combine_bwd(dq, A, da, dv);
    for (int k = 0; k < 4; ++k) {
      lds[L.Dq0 + t * 4 + k] = k < A ? da[k] : 0.0f;
      lds[L.Dq1 + t * 4 + k] = k == 0 ? dv : 0.0f;
      if (t < nrows && k < A) da_out[(size_t)(row0 + t) * A + k] = da[k];
    }
    if (t < nrows) {
      dv_out[row0 + t] = dv;
      if (td_out) td_out[row0 + t] = td;
      terms[(size_t)(row0 + t) * 3] = (double)term;
    }
  }
  __syncthreads();
  {
    const BwdItem st[2] = {BwdItem{L.Dq1, 4, 1, hp[0].wv, H, -1, nullptr, -1, 0, NA, Xv, ld, nullptr, 0, nullptr},
                           BwdItem{L.Dq0, 4, A, hp[0].wa, H, -1, nullptr, -1, 0, NA, Xa, ld, nullptr, 0, nullptr}};
    bwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  for (int e = t; e < 16 * H; e += kThreads) {
    const int row = e / H, k = e - row * H;
    const float g = (lds[Xv + row * ld + k] + lds[Xa + row * ld + k]) * act_bwd(lds[X[0] + row * ld + k], R, 0.0f, 0.0f);
    if (Zs >= 0) lds[Zs + row * ld + k] = g;
    if (row < nrows) Zg[(size_t)(row0 + row) * H + k] = g;
  }
}

// The tile phase of a three-layer Q network's update: the policy net's tile list — no target twins (the hard copy is the
// caller's), the reference's clamp of every gradient element in front of Adam's moments — and its launch.  The dueling net's
// middle segments are its two heads on fc1's output: the value head from dv (ws.H2, [B][1]), the advantage head from da (ws.dq);
// it has no H x H layer and so no images.  (At most 256 rows: no slice partials, and the loss sum closes in this launch's last
// block — dqn_td_kernel's one block.)
template <class Args>
inline void launch_qnet3_dw(const Args& a, const QNet3Ws& ws, bool dueling, hipStream_t stream) {
  const int B = a.B, D = a.D, A = a.A, H = a.H;
  DwArgs p{};
  DwBuilder pb{p, B};
  pb.seg(ws.Z1, H, H, ws.s, D, nullptr, 0, D, D, a.policy.w[0], a.policy.b[0]);
  if (dueling) pb.seg(ws.H2, 1, 1, ws.H1, H, nullptr, 0, H, H, a.policy.w[1], a.policy.b[1]);
  else {
    const QNet3Images im(a.images, H);
    pb.seg(ws.Z2, H, H, ws.H1, H, nullptr, 0, H, H, a.policy.w[1], a.policy.b[1], nullptr, nullptr, im.pf, im.pb);
  }
  pb.seg(ws.dq, A, A, dueling ? ws.H1 : ws.H2, H, nullptr, 0, H, H, a.policy.w[2], a.policy.b[2]);
  pb.close(a, nullptr, a.policy_p, a.policy_m, a.policy_v, a.adam_policy, a.adam_policy_dev, 0.0f, 0.0f, ws.terms, nullptr, 0, 1, a.loss_sum);
  p.clamp_abs = a.clamp_abs;
  launch_dw(p, stream);
}

// ---- acting ----
// lanes t < 16: the slab's observations into L.S (rows beyond N are zero), and the barrier in front of the first stage
template <class Args>
__device__ __forceinline__ void act_load_obs(const Args& a, float* lds, const Lds& L, int t, int row0, int nrows) {
  if (t < 16) {
    const int i = row0 + t, D = a.D;
    for (int k = 0; k < kMaxD; ++k) lds[L.S + t * kMaxD + k] = (t < nrows && k < D) ? a.obs[(size_t)i * D + k] : 0.0f;
  }
  __syncthreads();
}
// the epsilon-greedy choice of env lane t < nrows on its Q row (gymrl_epsilon_greedy's keys; counter and epsilon from the
// device record where there is one)
__device__ __forceinline__ int epsilon_greedy_lane(const gymrl_dqn_act_args& a, const float* q, int t, int row0) {
  const uint64_t counter = a.counter_dev ? a.counter_dev[0] : a.counter;
  const float eps = a.epsilon_dev ? a.epsilon_dev[0] : a.epsilon;
  return epsilon_greedy_pick(q, a.A, a.u ? a.u + (size_t)(row0 + t) * 2 : nullptr, a.seed, (uint64_t)(a.env_id0 + row0 + t), counter, eps);
}

}  // namespace
}  // namespace slab
}  // namespace gymrl
