// ddqn_step.hip — double DQN + PER's update (ddqn_per_cartpole.py:197-244) on the row-slab stages of slab_step_device.hpp, in
// dqn_step.hip's scheme:
//
//   ddqn_r1_kernel  B/16 workgroups: gather by the SAMPLED rows, policy(s) | policy(s') | target(s'), the double-Q target,
//                   the importance-weighted loss gradient, the TD errors for the sum tree, the policy net's dX chain     (rows)
//   sac_dw_kernel   the policy net's tiles + the +-1 gradient clamp + Adam, the loss sum                                (tiles)
//
// DQN's row phase with a third forward chain (the online network on s' picks the action the target network evaluates, :225-228),
// a weight per row (:232) and td_out leaving for gymrl_per_update_td.  Acting is gymrl_dqn_act_step itself: the network has
// QNetwork's shape.  The stratified draw stays gymrl_per_sample's launch (the weights' batch-wide maximum is a reduction across
// workgroups): idx and is_weight arrive as arrays.  ONE workgroup carries a slab through the whole row phase, so nothing here
// waits for another workgroup: no flag, no counter; launch order on one stream is the only ordering.
//
// LDS per workgroup: the small per-row slabs (kSmallFloats floats = 4.0 KB) + six [16][slab_ld(H)] activation slabs — P1, N1,
// T1 (first layers of policy(s), policy(s'), target(s')) and P2, N2, T2 (second layers); all six are live across the second
// stage.  T1 is dead once that stage is out and carries dL/dz2 through the input-gradient chain, as in dqn_r1_kernel.  At
// H = 256 (slab_ld = 260): 6 * 16 * 260 * 4 = 99,840 B + 4,096 B = 103,936 B of the compute unit's 160 KB: one workgroup per
// compute unit, which a grid of at most 16 workgroups (B <= 256) never asks more of.  At H = 32 (slab_ld = 36): 17.9 KB.
//
// The dueling network (ddqn_per_duel_cartpole.py:58-78: fc1, then value_stream [1][H] and advantage_stream [A][H]) has a second
// instance of the row kernel and an act kernel of its own, ddqn_duel_r1_kernel / ddqn_duel_act_kernel: one hidden layer, the two
// heads as two items of one stage per chain, the combine q = v + (a - mean a) and its backward per row, ONE dX stage.  LDS: three
// slabs (P1, N1, T1; N1 and T1 are dead after the heads and take the two heads' input gradients): 54,016 B at H = 256.  No
// H x H layer, so no weight images.  duel_combine below states the arithmetic order.
#include "value_step_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::slab;

constexpr int kDdqnMaxBatch = 256;     // (ops.DDQN_FUSED_MAX_BATCH) one grid of at most 16 slabs in the row phase: the loss sum is one block's
constexpr int kDdqnSlabs = 6;
// (gymrl_ddqn_update_args.images — gymrl_dqn_update_args.images' layout — and the workspace: QNet3Images / QNet3Ws)

template <int HC>
__global__ __launch_bounds__(kThreads) void ddqn_r1_kernel(const gymrl_ddqn_update_args a, const QNet3Ws ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int P1 = L.big, N1 = P1 + 16 * ld, T1 = N1 + 16 * ld, P2 = T1 + 16 * ld, N2 = P2 + 16 * ld, T2 = N2 + 16 * ld;
  const int Z0 = T1;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD;
  const QNet3Images im(a.images, H);
  const gymrl_td3_actor_params &p = a.policy, &tg = a.target;
  // ---- ring gather by the sampled rows: one thread per row, rows beyond the batch are zero (weight 0).  (The text of
  // gather_ring_row and, below, of td_row<false>, kept in place: called from here they left this kernel's registers different
  // and the Acrobot N = 64 step 1.9 % outside the parent's range — DESIGN 4m') ----
  if (t < 16) {
    const int b = row0 + t;
    const int64_t row = checked_ring_row(t < nrows, [&] { return (int64_t)a.idx[b]; }, a.cap);
    const bool ok = row >= 0;
    for (int k = 0; k < kMaxD; ++k) {
      const float sv = (ok && k < D) ? a.r_state[row * D + k] : 0.0f;
      lds[L.S + t * kMaxD + k] = sv;
      lds[L.S2 + t * kMaxD + k] = (ok && k < D) ? a.r_next[row * D + k] : 0.0f;
      if (t < nrows && k < D) ws.s[(size_t)b * D + k] = sv;
    }
    lds[L.Misc + t * 4 + 0] = ok ? a.r_reward[row] : 0.0f;
    lds[L.Misc + t * 4 + 1] = ok ? (float)a.r_flag[row] : 0.0f;            // dones become float32
    lds[L.Misc + t * 4 + 2] = ok ? __int_as_float((int)a.r_action[row]) : 0.0f;
    lds[L.Misc + t * 4 + 3] = ok ? a.is_weight[b] : 0.0f;
  }
  __syncthreads();
  // ---- policy_net(s) (:222), policy_net(s') (:225) and target_net(s') (:227): three independent chains, layer by layer ----
  {
    const FwdItem st[3] = {fwd_item(L.S, kD, -1, 0, D, D, H, p.w[0], p.b[0], P1, ld, ws.H1, H, R),
                           fwd_item(L.S2, kD, -1, 0, D, D, H, p.w[0], p.b[0], N1, ld, nullptr, 0, R),
                           fwd_item(L.S2, kD, -1, 0, D, D, H, tg.w[0], tg.b[0], T1, ld, nullptr, 0, R)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[3] = {fwd_item(P1, ld, -1, 0, H, H, H, p.w[1], p.b[1], P2, ld, ws.H2, H, R, 0.0f, 0.0f, im.pf),
                           fwd_item(N1, ld, -1, 0, H, H, H, p.w[1], p.b[1], N2, ld, nullptr, 0, R, 0.0f, 0.0f, im.pf),
                           fwd_item(T1, ld, -1, 0, H, H, H, tg.w[1], tg.b[1], T2, ld, nullptr, 0, R, 0.0f, 0.0f, im.tf)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[3] = {fwd_item(P2, ld, -1, 0, H, H, A, p.w[2], p.b[2], L.Cq0, 4, nullptr, 0, NA),
                           fwd_item(N2, ld, -1, 0, H, H, A, p.w[2], p.b[2], L.Q1, 4, nullptr, 0, NA),
                           fwd_item(T2, ld, -1, 0, H, H, A, tg.w[2], tg.b[2], L.Q0, 4, nullptr, 0, NA)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 16) {                           // offpolicy.hip dqn_td_kernel (:225-232) with qn_online and w set, gamma_n = gamma
    const float* sel = lds + L.Q1 + t * 4;
    int astar = 0;
    float best = sel[0];
    for (int k = 1; k < A; ++k) if (sel[k] > best) { best = sel[k]; astar = k; }
    const float nq = lds[L.Q0 + t * 4 + astar];
    const float y = lds[L.Misc + t * 4 + 0] + a.gamma * nq * (1.0f - lds[L.Misc + t * 4 + 1]);
    const int act = __float_as_int(lds[L.Misc + t * 4 + 2]);
    const float td = lds[L.Cq0 + t * 4 + act] - y;
    const float wb = lds[L.Misc + t * 4 + 3], invB = 1.0f / (float)a.B;
    for (int k = 0; k < 4; ++k) {
      const float d = k == act ? (2.0f * td) * wb * invB : 0.0f;
      lds[L.Dq0 + t * 4 + k] = d;
      if (t < nrows && k < A) ws.dq[(size_t)(row0 + t) * A + k] = d;
    }
    if (t < nrows) {
      a.td_out[row0 + t] = td;
      ws.terms[(size_t)(row0 + t) * 3] = (double)((td * td) * wb);
    }
  }
  __syncthreads();
  // ---- the policy net's input-gradient chain (what backward() computes before the weight gradients) ----
  bwd_one(lds, {BwdItem{L.Dq0, 4, A, p.w[2], H, -1, nullptr, P2, ld, R, Z0, ld, ws.Z2, H, nullptr}}, row0, nrows);
  bwd_stage(lds, {BwdItem{Z0, ld, H, p.w[1], H, -1, nullptr, P1, ld, R, -1, 0, ws.Z1, H, im.pb}}, row0, nrows);      // (the last stage: no barrier behind it)
}

// ---- the dueling instance: policy.w / .b = {fc1, value_stream, advantage_stream}; ws.H2 holds dv [B], ws.dq holds da [B][A] ----
template <int HC>
__global__ __launch_bounds__(kThreads) void ddqn_duel_r1_kernel(const gymrl_ddqn_update_args a, const QNet3Ws ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int P1 = L.big, N1 = P1 + 16 * ld, T1 = N1 + 16 * ld;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const int R = GYMRL_ACT_RELU, kD = kMaxD;
  const gymrl_td3_actor_params &p = a.policy, &tg = a.target;
  // ---- ring gather by the SAMPLED rows: a row beyond the batch or outside [0, cap) is a zero row of weight 0 ----
  if (t < 16) {
    const int b = row0 + t;
    const int64_t row = checked_ring_row(t < nrows, [&] { return (int64_t)a.idx[b]; }, a.cap);
    gather_ring_row(a, lds, L, t, b, t < nrows, row, /*checked=*/true, ws.s, RowWeight::kGiven, a.is_weight);
  }
  __syncthreads();
  {
    const FwdItem st[3] = {fwd_item(L.S, kD, -1, 0, D, D, H, p.w[0], p.b[0], P1, ld, ws.H1, H, R),
                           fwd_item(L.S2, kD, -1, 0, D, D, H, p.w[0], p.b[0], N1, ld, nullptr, 0, R),
                           fwd_item(L.S2, kD, -1, 0, D, D, H, tg.w[0], tg.b[0], T1, ld, nullptr, 0, R)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  // the heads, the loss and ONE dX stage back to fc1: N1 and T1 take the heads' input gradients once policy(s') and target(s')
  // are through their heads; dL/dz1 leaves for ws.Z1 with no further stage (Zs = -1)
  const DuelHeads pol{p.w[1], p.b[1], p.w[2], p.b[2]}, tgt{tg.w[1], tg.b[1], tg.w[2], tg.b[2]};
  duel_heads_segment(lds, L, A, H, ld, row0, nrows, a.gamma, a.B, {P1, N1, T1}, {pol, pol, tgt}, /*Xv=*/N1, /*Xa=*/T1, ws.H2, ws.dq, a.td_out,
                     ws.terms, /*Zs=*/-1, ws.Z1);
}

// ---- acting with the dueling network: gymrl_dqn_act_step's kernel with the two heads and the combine in front of the choice ----
template <int HC>
__global__ __launch_bounds__(kThreads) void ddqn_duel_act_kernel(const gymrl_dqn_act_args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int X0 = L.big;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.N - row0);
  const int t = threadIdx.x;
  act_load_obs(a, lds, L, t, row0, nrows);
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD;
  fwd_one(lds, {fwd_item(L.S, kD, -1, 0, D, D, H, a.policy.w[0], a.policy.b[0], X0, ld, nullptr, 0, R)}, row0, nrows);
  {
    const FwdItem st[2] = {fwd_item(X0, ld, -1, 0, H, H, 1, a.policy.w[1], a.policy.b[1], L.Cq1, 4, nullptr, 0, NA),
                           fwd_item(X0, ld, -1, 0, H, H, A, a.policy.w[2], a.policy.b[2], L.Cq0, 4, nullptr, 0, NA)};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 64) {
    int act = 0;
    if (t < nrows) {
      float* q = lds + L.Mean + t * kMaxA;
      duel_combine(lds + L.Cq0 + t * 4, lds[L.Cq1 + t * 4], A, q);
      act = epsilon_greedy_lane(a, q, t, row0);
    }
    cartpole_act_tail(a, lds, L, t, row0, nrows, act);
  }
}

}  // namespace

extern "C" {

size_t gymrl_ddqn_update_workspace_bytes(int B, int D, int A, int H) { return workspace_bytes<QNet3Ws>(B, D, A, H); }
size_t gymrl_ddqn_args_bytes(int which) { return which == 1 ? sizeof(gymrl_ddqn_update_args) : 0; }

static int ddqn_set_lds_attr() {
  static bool done = false;
  return set_max_lds_once(done, {(const void*)ddqn_r1_kernel<0>, (const void*)ddqn_r1_kernel<256>, (const void*)ddqn_duel_r1_kernel<0>,
                                 (const void*)ddqn_duel_r1_kernel<256>, (const void*)ddqn_duel_act_kernel<0>,
                                 (const void*)ddqn_duel_act_kernel<256>}, (int)lds_bytes(256, kDdqnSlabs));
}

static bool ddqn_update_args_ok(const gymrl_ddqn_update_args& a) {
  if (!slab_shape_ok(a.B, kDdqnMaxBatch, a.D, a.A, a.H)) return false;
  if (!ring_ok(a) || !all_set({a.idx, a.is_weight, a.td_out, a.workspace, a.loss_sum, a.policy_p, a.policy_m, a.policy_v}) ||
      !(a.clamp_abs >= 0.0f) || a.cap < 1 || (a.dueling != 0 && a.dueling != 1))
    return false;
  if (a.dueling && a.A != 2) return false;            // duel_combine's order is pinned for two actions
  return net_ok(a.policy) && net_ok(a.target);
}

int gymrl_ddqn_pack_images(const gymrl_ddqn_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_ddqn_update_args& a = *args;
  if (!pack_args_ok(a) || a.dueling || !all_set({a.policy.w[1], a.target.w[1]})) return -22;      // (the dueling net has no H x H layer)
  hipLaunchKernelGGL(pack_images_kernel, dim3((a.H * a.H + 255) / 256, QNet3Images::kCount), dim3(256), 0, (hipStream_t)stream_, QNet3Images::sources(a), a.images, a.H);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_ddqn_update(const gymrl_ddqn_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_ddqn_update_args& a = *args;
  if (!ddqn_update_args_ok(a)) return -22;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = ddqn_set_lds_attr()) return rc;
  QNet3Ws ws;
  QNet3Ws::carve(&ws, align256(a.workspace), a.B, a.D, a.A, a.H);
  const int H = a.H, slabs = (a.B + 15) / 16;
  if (a.dueling) hipLaunchKernelGGL(H == 256 ? ddqn_duel_r1_kernel<256> : ddqn_duel_r1_kernel<0>, dim3(slabs), dim3(kThreads), lds_bytes(H, 3), stream, a, ws);
  else hipLaunchKernelGGL(H == 256 ? ddqn_r1_kernel<256> : ddqn_r1_kernel<0>, dim3(slabs), dim3(kThreads), lds_bytes(H, kDdqnSlabs), stream, a, ws);
  launch_qnet3_dw(a, ws, a.dueling != 0, stream);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_ddqn_duel_act_step(const gymrl_dqn_act_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_dqn_act_args& a = *args;
  if (!act_args_ok(a, GYMRL_ENV_CARTPOLE, /*refuse_neg_cursor=*/true) || !net_ok(a.policy)) return -22;
  if (const int rc = ddqn_set_lds_attr()) return rc;
  hipLaunchKernelGGL(a.H == 256 ? ddqn_duel_act_kernel<256> : ddqn_duel_act_kernel<0>, dim3((a.N + 15) / 16), dim3(kThreads), lds_bytes(a.H, 1), (hipStream_t)stream_, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
