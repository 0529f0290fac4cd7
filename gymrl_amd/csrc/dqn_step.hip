// dqn_step.hip — DQN's CartPole vector step (dqn_cartpole.py:124-133, :135-168) on the row-slab stages of
// slab_step_device.hpp, in dsac_step.hip's scheme:
//
//   dqn_act_kernel  N/16 workgroups: policy net Q values, epsilon-greedy, CartPole step, replay row               (acting)
//   dqn_r1_kernel   B/16 workgroups: draw + gather, policy(s) | target(s'), TD target, loss gradient, dX chain    (rows)
//   sac_dw_kernel   the policy net's tiles + the +-1 gradient clamp + Adam, the loss sum                         (tiles)
//
// Discrete SAC's step with ONE online network and a hard-copied target: two chains in the row phase where dSAC runs five, no
// second row phase, no Polyak twins in the tile phase (the segments carry none: the hard copy is the trainer's), and the
// reference's clamp of every gradient element to +-1 (:163-165) as DwArgs.clamp_abs.  ONE workgroup carries a slab through the
// whole row phase — policy(s) and target(s') ride along as items of the same stages — so nothing here waits for another
// workgroup: no flag, no counter; launch order on one stream is the only ordering.
#include "value_step_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::slab;

constexpr int kDqnMaxBatch = 256;      // (ops.DQN_FUSED_MAX_BATCH) one grid of at most 16 slabs in the row phase: the loss sum is one block's
// (gymrl_dqn_update_args.images and the workspace: QNet3Images / QNet3Ws of value_step_device.hpp)

// ---- R1: draw + gather, policy(s) next to target(s'), the TD target and the loss gradient, the policy net's dX chain ----
template <int HC>
__global__ __launch_bounds__(kThreads) void dqn_r1_kernel(const gymrl_dqn_update_args a, const QNet3Ws ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  // four activation slabs: the target's first (T1) is dead once its second layer is out and carries dL/dz2 then
  const int P1 = L.big, T1 = P1 + 16 * ld, P2 = T1 + 16 * ld, T2 = P2 + 16 * ld;
  const int Z0 = T1;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD;
  const QNet3Images im(a.images, H);
  const gymrl_td3_actor_params &p = a.policy, &tg = a.target;
  // ---- index draw + ring gather: one thread per row, rows beyond the batch are zero ----
  if (t < 16) {
    const int b = row0 + t;
    const int64_t row = t < nrows ? replay_draw_row(a, b) : -1;       // (not checked against the ring: `checked` below)
    gather_ring_row(a, lds, L, t, b, t < nrows, row, /*checked=*/false, ws.s);
  }
  __syncthreads();
  // ---- policy_net(s) (:150) and target_net(s') (:154): two independent chains, layer by layer ----
  {
    const FwdItem st[2] = {fwd_item(L.S, kD, -1, 0, D, D, H, p.w[0], p.b[0], P1, ld, ws.H1, H, R),
                           fwd_item(L.S2, kD, -1, 0, D, D, H, tg.w[0], tg.b[0], T1, ld, nullptr, 0, R)};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[2] = {fwd_item(P1, ld, -1, 0, H, H, H, p.w[1], p.b[1], P2, ld, ws.H2, H, R, 0.0f, 0.0f, im.pf),
                           fwd_item(T1, ld, -1, 0, H, H, H, tg.w[1], tg.b[1], T2, ld, nullptr, 0, R, 0.0f, 0.0f, im.tf)};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[2] = {fwd_item(P2, ld, -1, 0, H, H, A, p.w[2], p.b[2], L.Cq0, 4, nullptr, 0, NA),
                           fwd_item(T2, ld, -1, 0, H, H, A, tg.w[2], tg.b[2], L.Q0, 4, nullptr, 0, NA)};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 16) {                           // offpolicy.hip dqn_td_kernel (:155-161) with qn_online == nullptr, w == nullptr, gamma_n = gamma
    const float* qt = lds + L.Q0 + t * 4;       // (the target row picks a* itself)
    float td, dq[4];
    const float term = td_row<false>(lds + L.Cq0 + t * 4, qt, qt, A, lds + L.Misc + t * 4, a.gamma, 1.0f, 1.0f / (float)a.B, td, dq);
    for (int k = 0; k < 4; ++k) {
      lds[L.Dq0 + t * 4 + k] = dq[k];
      if (t < nrows && k < A) ws.dq[(size_t)(row0 + t) * A + k] = dq[k];
    }
    if (t < nrows) ws.terms[(size_t)(row0 + t) * 3] = (double)term;
  }
  __syncthreads();
  // ---- the policy net's input-gradient chain (what backward() computes before the weight gradients) ----
  bwd_one(lds, {BwdItem{L.Dq0, 4, A, p.w[2], H, -1, nullptr, P2, ld, R, Z0, ld, ws.Z2, H, nullptr}}, row0, nrows);
  bwd_stage(lds, {BwdItem{Z0, ld, H, p.w[1], H, -1, nullptr, P1, ld, R, -1, 0, ws.Z1, H, im.pb}}, row0, nrows);      // (the last stage: no barrier behind it)
}

// ---- acting: the policy net's Q values, the epsilon-greedy choice (gymrl_epsilon_greedy's keys), the env's step, replay row ----
// KIND: CartPole-v1 (gymrl_dqn_act_step, and gymrl_dqn_act_step_classic's kind 0), MountainCar-v0, Acrobot-v1
template <int HC, int KIND>
__global__ __launch_bounds__(kThreads) void dqn_act_kernel(const gymrl_dqn_act_args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int X0 = L.big, X1 = X0 + 16 * ld;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.N - row0);
  const int t = threadIdx.x;
  act_load_obs(a, lds, L, t, row0, nrows);
  const int R = GYMRL_ACT_RELU, kD = kMaxD, kA = kMaxA;
  const float* pf = (a.images && (H & 15) == 0) ? a.images : nullptr;
  fwd_one(lds, {fwd_item(L.S, kD, -1, 0, D, D, H, a.policy.w[0], a.policy.b[0], X0, ld, nullptr, 0, R)}, row0, nrows);
  fwd_one(lds, {fwd_item(X0, ld, -1, 0, H, H, H, a.policy.w[1], a.policy.b[1], X1, ld, nullptr, 0, R, 0.0f, 0.0f, pf)}, row0, nrows);
  fwd_one(lds, {fwd_item(X1, ld, -1, 0, H, H, A, a.policy.w[2], a.policy.b[2], L.Mean, kA, nullptr, 0, GYMRL_ACT_NONE)}, row0, nrows);
  // one lane per env: the choice, the env's step with auto-reset, replay row (the first wave: 16 lanes busy)
  if (t < 64) {
    int act = 0;
    if (t < nrows) act = epsilon_greedy_lane(a, lds + L.Mean + t * kMaxA, t, row0);
    classic_act_tail<KIND>(a, lds, L, t, row0, nrows, act);
  }
}
// the instance of (hidden width, env kind); nullptr for a kind without one
using DqnActKernel = void (*)(const gymrl_dqn_act_args);
template <int KIND>
DqnActKernel dqn_act_instance(bool wide) { return wide ? dqn_act_kernel<256, KIND> : dqn_act_kernel<0, KIND>; }
DqnActKernel dqn_act_pick(int env_kind, bool wide) {
  switch (env_kind) {
    case GYMRL_ENV_CARTPOLE: return dqn_act_instance<GYMRL_ENV_CARTPOLE>(wide);
    case GYMRL_ENV_MOUNTAINCAR: return dqn_act_instance<GYMRL_ENV_MOUNTAINCAR>(wide);
    case GYMRL_ENV_ACROBOT: return dqn_act_instance<GYMRL_ENV_ACROBOT>(wide);
    default: return nullptr;
  }
}

}  // namespace

extern "C" {

size_t gymrl_dqn_update_workspace_bytes(int B, int D, int A, int H) { return workspace_bytes<QNet3Ws>(B, D, A, H); }
size_t gymrl_dqn_args_bytes(int which) { return which == 0 ? sizeof(gymrl_dqn_act_args) : which == 1 ? sizeof(gymrl_dqn_update_args) : 0; }

static int dqn_set_lds_attr() {
  static bool done = false;
  return set_max_lds_once(done, {(const void*)dqn_r1_kernel<0>, (const void*)dqn_r1_kernel<256>, (const void*)dqn_act_pick(GYMRL_ENV_CARTPOLE, false),
                                 (const void*)dqn_act_pick(GYMRL_ENV_CARTPOLE, true)}, (int)lds_bytes(256, 4));
}
// (the MountainCar and Acrobot instances: raised on gymrl_dqn_act_step_classic's first call, so that a CartPole run's set-up is the parent's)
static int dqn_set_lds_attr_classic() {
  static bool done = false;
  return set_max_lds_once(done, {(const void*)dqn_act_pick(GYMRL_ENV_MOUNTAINCAR, false), (const void*)dqn_act_pick(GYMRL_ENV_MOUNTAINCAR, true),
                                 (const void*)dqn_act_pick(GYMRL_ENV_ACROBOT, false), (const void*)dqn_act_pick(GYMRL_ENV_ACROBOT, true)}, (int)lds_bytes(256, 4));
}
static int dqn_act_launch(const gymrl_dqn_act_args& a, void* stream_) {
  hipLaunchKernelGGL(dqn_act_pick(a.env_kind, a.H == 256), dim3((a.N + 15) / 16), dim3(kThreads), lds_bytes(a.H, 2), (hipStream_t)stream_, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_dqn_act_step(const gymrl_dqn_act_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_dqn_act_args& a = *args;
  if (!act_args_ok(a, GYMRL_ENV_CARTPOLE, /*refuse_neg_cursor=*/true) || !net_ok(a.policy)) return -22;
  if (const int rc = dqn_set_lds_attr()) return rc;
  return dqn_act_launch(a, stream_);
}

// the same launch for the env kind the block names: CartPole-v1, MountainCar-v0 or Acrobot-v1, each with its own (D, A)
int gymrl_dqn_act_step_classic(const gymrl_dqn_act_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_dqn_act_args& a = *args;
  if (!classic_act_kind_ok(a.env_kind) || !act_args_ok(a, a.env_kind, /*refuse_neg_cursor=*/true) || !net_ok(a.policy)) return -22;
  if (const int rc = dqn_set_lds_attr()) return rc;
  if (const int rc = dqn_set_lds_attr_classic()) return rc;
  return dqn_act_launch(a, stream_);
}

static bool dqn_update_args_ok(const gymrl_dqn_update_args& a) {
  if (!slab_shape_ok(a.B, kDqnMaxBatch, a.D, a.A, a.H)) return false;
  if (!ring_ok(a) || !all_set({a.workspace, a.loss_sum, a.policy_p, a.policy_m, a.policy_v}) || !draw_ok(a, /*idx_dev_counts=*/true) ||
      !(a.clamp_abs >= 0.0f))
    return false;
  return net_ok(a.policy) && net_ok(a.target);
}

int gymrl_dqn_pack_images(const gymrl_dqn_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_dqn_update_args& a = *args;
  if (!pack_args_ok(a) || !all_set({a.policy.w[1], a.target.w[1]})) return -22;
  hipLaunchKernelGGL(pack_images_kernel, dim3((a.H * a.H + 255) / 256, QNet3Images::kCount), dim3(256), 0, (hipStream_t)stream_, QNet3Images::sources(a), a.images, a.H);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_dqn_update(const gymrl_dqn_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_dqn_update_args& a = *args;
  if (!dqn_update_args_ok(a)) return -22;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = dqn_set_lds_attr()) return rc;
  QNet3Ws ws;
  QNet3Ws::carve(&ws, align256(a.workspace), a.B, a.D, a.A, a.H);
  hipLaunchKernelGGL(a.H == 256 ? dqn_r1_kernel<256> : dqn_r1_kernel<0>, dim3((a.B + 15) / 16), dim3(kThreads), lds_bytes(a.H, 4), stream, a, ws);
  launch_qnet3_dw(a, ws, /*dueling=*/false, stream);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
