// dsac_step.hip — discrete SAC's CartPole vector step (sac_cartpole.py:127-138, :148-227) on the row-slab stages of
// slab_step_device.hpp, in td3_step.hip's scheme:
//
//   dsac_act_kernel  N/16 workgroups: actor logits, categorical draw, CartPole step, replay row                       (acting)
//   dsac_r1_kernel   B/16 workgroups: draw + gather, actor(s') | critic targets(s'), softmax, y, critics(s), dX chains  (rows)
//   dsac_dw2_kernel  sac_dw_body over two tile lists: both critics' tiles + Adam + Polyak, each on its own flat buffer  (tiles)
//   dsac_r3_kernel   B/16 workgroups: actor(s) | updated critics(s), softmax, actor loss, softmax backward, dX chain    (rows)
//   sac_dw_kernel    actor tiles + Adam, the two actor sums, the float32 temperature step                               (tiles)
//
// TD3's step with three-layer networks that end in A columns, an expectation over the actions (offpolicy.hip's dsac_*
// expressions) in place of a sampled action, twin critics that are separate modules with separate optimisers, no actor
// target, and the actor phase on every step.  ONE workgroup carries a slab through a whole row phase — the independent
// chains ride along as items of the same stages — so nothing here waits for another workgroup: no flag, no counter.
#include "softmax_device.hpp"
#include "value_step_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::slab;

constexpr int kDsacMaxBatch = 256;     // (ops.DSAC_FUSED_MAX_BATCH) one grid of at most 16 slabs per row phase
struct DsacImages {                    // gymrl_dsac_update_args.images, f32[8][H*H]: five forward images, then three input-gradient images
  const float *af, *cf[2], *tf[2], *ab, *cb[2];
  __host__ __device__ DsacImages(const float* base, int H) {
    const ImageSlots at(base, H);
    af = at(0); cf[0] = at(1); cf[1] = at(2); tf[0] = at(3); tf[1] = at(4); ab = at(5); cb[0] = at(6); cb[1] = at(7);
  }
  // the same slots as the layers they are packed from
  static constexpr int kCount = 8;
  static PackTable sources(const gymrl_dsac_update_args& a) {
    return PackTable{{a.actor.w[1], a.critic1.w[1], a.critic2.w[1], a.critic1_target.w[1], a.critic2_target.w[1],
                      a.actor.w[1], a.critic1.w[1], a.critic2.w[1], nullptr}, 5};
  }
};

// hand-off between the row phases and the tile phases (caller-owned workspace)
struct DsacWs {
  float* s;                                          // [B][D]: the gathered states
  float *H1[2], *Z1[2], *H2[2], *Z2[2], *dq[2];      // critic i: activations and dL/dz per layer ([B][H]; dq [B][A])
  float *aH1, *aZ1, *aH2, *aZ2, *dlogit;             // actor ([B][H]; dlogit [B][A])
  double* terms;                                     // [B][3]: R1 critic1, critic2 terms in columns 0, 1; R3 actor, entropy terms in 1, 2
  __host__ __device__ static size_t carve(DsacWs* w, void* base, int B, int D, int A, int H) {
    carve_taker take{base};
    float* s = take((size_t)B * D);
    float* h[12];
    for (int i = 0; i < 12; ++i) h[i] = take((size_t)B * H);
    float* dq0 = take((size_t)B * A); float* dq1 = take((size_t)B * A); float* dl = take((size_t)B * A);
    double* terms = reinterpret_cast<double*>(take((size_t)B * 6));
    if (w) {
      w->s = s;
      w->H1[0] = h[0]; w->H1[1] = h[1]; w->Z1[0] = h[2]; w->Z1[1] = h[3]; w->H2[0] = h[4]; w->H2[1] = h[5]; w->Z2[0] = h[6]; w->Z2[1] = h[7];
      w->aH1 = h[8]; w->aZ1 = h[9]; w->aH2 = h[10]; w->aZ2 = h[11];
      w->dq[0] = dq0; w->dq[1] = dq1; w->dlogit = dl; w->terms = terms;
    }
    return take.off;
  }
};

// ---- R1: draw + gather, actor(s') next to both critic targets(s'), softmax, y, both critics(s), loss gradient, dX chains ----
template <int HC>
__global__ __launch_bounds__(kThreads) void dsac_r1_kernel(const gymrl_dsac_update_args a, const DsacWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  // six activation slabs: the s' chains' (X0, X1 actor; T0 .. T3 targets) are dead once y is formed and carry the critics' then
  const int X0 = L.big, X1 = X0 + 16 * ld, T0 = X1 + 16 * ld, T1 = T0 + 16 * ld, T2 = T1 + 16 * ld, T3 = T2 + 16 * ld;
  const int C1a = X0, C2a = X1, C1b = T0, C2b = T1, Z0 = T2, Z1 = T3;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD, kA = kMaxA;
  const DsacImages im(a.images, H);
  const gymrl_td3_actor_params &p = a.actor, &c1 = a.critic1, &c2 = a.critic2, &t1 = a.critic1_target, &t2 = a.critic2_target;
  // ---- index draw + ring gather: one thread per row, rows beyond the batch are zero ----
  // (value_step_device.hpp gather_ring_row with an unchecked row and no weight is this text; called from here this kernel's
  // registers came out differently and the N = 64 step measured 0.4 % outside the parent's range, so the text stays)
  if (t < 16) {
    const int b = row0 + t;
    const bool ok = t < nrows;
    const int64_t row = ok ? replay_draw_row(a, b) : 0;
    for (int k = 0; k < kMaxD; ++k) {
      const float sv = (ok && k < D) ? a.r_state[row * D + k] : 0.0f;
      lds[L.S + t * kMaxD + k] = sv;
      lds[L.S2 + t * kMaxD + k] = (ok && k < D) ? a.r_next[row * D + k] : 0.0f;
      if (ok && k < D) ws.s[(size_t)b * D + k] = sv;
    }
    lds[L.Misc + t * 4 + 0] = ok ? a.r_reward[row] : 0.0f;
    lds[L.Misc + t * 4 + 1] = ok ? (float)a.r_flag[row] : 0.0f;            // dones become float32
    lds[L.Misc + t * 4 + 2] = ok ? __int_as_float((int)a.r_action[row]) : 0.0f;
  }
  __syncthreads();
  // ---- actor(s'), critic1_target(s'), critic2_target(s') (:173, :177-178): three independent chains, layer by layer ----
  {
    const FwdItem st[3] = {fwd_item(L.S2, kD, -1, 0, D, D, H, p.w[0], p.b[0], X0, ld, nullptr, 0, R),
                           fwd_item(L.S2, kD, -1, 0, D, D, H, t1.w[0], t1.b[0], T0, ld, nullptr, 0, R),
                           fwd_item(L.S2, kD, -1, 0, D, D, H, t2.w[0], t2.b[0], T1, ld, nullptr, 0, R)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[3] = {fwd_item(X0, ld, -1, 0, H, H, H, p.w[1], p.b[1], X1, ld, nullptr, 0, R, 0.0f, 0.0f, im.af),
                           fwd_item(T0, ld, -1, 0, H, H, H, t1.w[1], t1.b[1], T2, ld, nullptr, 0, R, 0.0f, 0.0f, im.tf[0]),
                           fwd_item(T1, ld, -1, 0, H, H, H, t2.w[1], t2.b[1], T3, ld, nullptr, 0, R, 0.0f, 0.0f, im.tf[1])};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[3] = {fwd_item(X1, ld, -1, 0, H, H, A, p.w[2], p.b[2], L.Mean, kA, nullptr, 0, NA),
                           fwd_item(T2, ld, -1, 0, H, H, A, t1.w[2], t1.b[2], L.Q0, 4, nullptr, 0, NA),
                           fwd_item(T3, ld, -1, 0, H, H, A, t2.w[2], t2.b[2], L.Q1, 4, nullptr, 0, NA)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 16) {                           // y (:170-183): softmax_device.hpp, then offpolicy.hip dsac_target_kernel
    float pr[kSoftmaxMaxA];
    softmax_row_fwd(lds + L.Mean + t * kMaxA, A, pr);
    const float alpha = det_expf(a.log_alpha[0]);
    float ent = 0.0f, minq = 0.0f;
    for (int k = 0; k < A; ++k) {
      const float pk = pr[k];
      ent += pk * det_logf(pk + 1e-8f);
      minq += pk * fminf(lds[L.Q0 + t * 4 + k], lds[L.Q1 + t * 4 + k]);
    }
    const float nv = minq + alpha * (-ent);
    lds[L.Misc + t * 4 + 3] = lds[L.Misc + t * 4 + 0] + a.gamma * (1.0f - lds[L.Misc + t * 4 + 1]) * nv;
  }
  __syncthreads();
  // ---- critic1(s), critic2(s) (:185-186) ----
  {
    const FwdItem st[2] = {fwd_item(L.S, kD, -1, 0, D, D, H, c1.w[0], c1.b[0], C1a, ld, ws.H1[0], H, R),
                           fwd_item(L.S, kD, -1, 0, D, D, H, c2.w[0], c2.b[0], C1b, ld, ws.H1[1], H, R)};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[2] = {fwd_item(C1a, ld, -1, 0, H, H, H, c1.w[1], c1.b[1], C2a, ld, ws.H2[0], H, R, 0.0f, 0.0f, im.cf[0]),
                           fwd_item(C1b, ld, -1, 0, H, H, H, c2.w[1], c2.b[1], C2b, ld, ws.H2[1], H, R, 0.0f, 0.0f, im.cf[1])};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[2] = {fwd_item(C2a, ld, -1, 0, H, H, A, c1.w[2], c1.b[2], L.Cq0, 4, nullptr, 0, NA),
                           fwd_item(C2b, ld, -1, 0, H, H, A, c2.w[2], c2.b[2], L.Cq1, 4, nullptr, 0, NA)};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 16) {                           // the loss gradient (:187-188): offpolicy.hip dsac_critic_kernel
    const int act = __float_as_int(lds[L.Misc + t * 4 + 2]);
    const float y = lds[L.Misc + t * 4 + 3];
    const float invB = 1.0f / (float)a.B;
    for (int n = 0; n < 2; ++n) {
      const float e = lds[(n ? L.Cq1 : L.Cq0) + t * 4 + act] - y;
      for (int k = 0; k < 4; ++k) {
        const float d = k == act ? 2.0f * e * invB : 0.0f;
        lds[(n ? L.Dq1 : L.Dq0) + t * 4 + k] = d;
        if (t < nrows && k < A) ws.dq[n][(size_t)(row0 + t) * A + k] = d;
      }
      if (t < nrows) ws.terms[(size_t)(row0 + t) * 3 + n] = (double)(e * e);
    }
  }
  __syncthreads();
  // ---- both critics' input-gradient chains (what backward() computes before the weight gradients) ----
  {
    const BwdItem st[2] = {BwdItem{L.Dq0, 4, A, c1.w[2], H, -1, nullptr, C2a, ld, R, Z0, ld, ws.Z2[0], H, nullptr},
                           BwdItem{L.Dq1, 4, A, c2.w[2], H, -1, nullptr, C2b, ld, R, Z1, ld, ws.Z2[1], H, nullptr}};
    bwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const BwdItem st[2] = {BwdItem{Z0, ld, H, c1.w[1], H, -1, nullptr, C1a, ld, R, -1, 0, ws.Z1[0], H, im.cb[0]},
                           BwdItem{Z1, ld, H, c2.w[1], H, -1, nullptr, C1b, ld, R, -1, 0, ws.Z1[1], H, im.cb[1]}};
    bwd_stage<2>(lds, st, row0, nrows);
  }
}

// ---- R3: actor(s) next to the updated critics(s), softmax, the actor loss's terms and dL/dprobs, softmax backward, the actor's chain ----
template <int HC>
__global__ __launch_bounds__(kThreads) void dsac_r3_kernel(const gymrl_dsac_update_args a, const DsacWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int AH1 = L.big, AH2 = AH1 + 16 * ld, H1a = AH2 + 16 * ld, H1b = H1a + 16 * ld, H2a = H1b + 16 * ld, H2b = H2a + 16 * ld;
  const int X0 = H1a;                     // the critics' slabs are dead once their Q columns are out
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD, kA = kMaxA;
  const DsacImages im(a.images, H);
  const gymrl_td3_actor_params &p = a.actor, &c1 = a.critic1, &c2 = a.critic2;
  if (t < 16) {
    const int b = row0 + t;
    for (int k = 0; k < kMaxD; ++k) lds[L.S + t * kMaxD + k] = (t < nrows && k < D) ? ws.s[(size_t)b * D + k] : 0.0f;
  }
  __syncthreads();
  // ---- actor(s) (:198) and critic1(s), critic2(s) with the parameters T2 has just written (:202-203; forward only) ----
  {
    const FwdItem st[3] = {fwd_item(L.S, kD, -1, 0, D, D, H, p.w[0], p.b[0], AH1, ld, ws.aH1, H, R),
                           fwd_item(L.S, kD, -1, 0, D, D, H, c1.w[0], c1.b[0], H1a, ld, nullptr, 0, R),
                           fwd_item(L.S, kD, -1, 0, D, D, H, c2.w[0], c2.b[0], H1b, ld, nullptr, 0, R)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[3] = {fwd_item(AH1, ld, -1, 0, H, H, H, p.w[1], p.b[1], AH2, ld, ws.aH2, H, R, 0.0f, 0.0f, im.af),
                           fwd_item(H1a, ld, -1, 0, H, H, H, c1.w[1], c1.b[1], H2a, ld, nullptr, 0, R, 0.0f, 0.0f, im.cf[0]),
                           fwd_item(H1b, ld, -1, 0, H, H, H, c2.w[1], c2.b[1], H2b, ld, nullptr, 0, R, 0.0f, 0.0f, im.cf[1])};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[3] = {fwd_item(AH2, ld, -1, 0, H, H, A, p.w[2], p.b[2], L.Mean, kA, nullptr, 0, NA),
                           fwd_item(H2a, ld, -1, 0, H, H, A, c1.w[2], c1.b[2], L.Q0, 4, nullptr, 0, NA),
                           fwd_item(H2b, ld, -1, 0, H, H, A, c2.w[2], c2.b[2], L.Q1, 4, nullptr, 0, NA)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 16) {                           // offpolicy.hip dsac_actor_kernel (:199-205), then the softmax backward
    float pr[kSoftmaxMaxA], dp[kSoftmaxMaxA], dz[kSoftmaxMaxA];
    softmax_row_fwd(lds + L.Mean + t * kMaxA, A, pr);
    const float invB = 1.0f / (float)a.B;
    const float alpha = det_expf(a.log_alpha[0]);
    float ent = 0.0f, minq = 0.0f;
#pragma unroll
    for (int k = 0; k < kSoftmaxMaxA; ++k) {
      dp[k] = 0.0f; dz[k] = 0.0f;
      if (k < A) {
        const float pk = pr[k];
        const float lp = det_logf(pk + 1e-8f);
        const float m = fminf(lds[L.Q0 + t * 4 + k], lds[L.Q1 + t * 4 + k]);
        ent += pk * lp;
        minq += pk * m;
        dp[k] = (alpha * (lp + pk / (pk + 1e-8f)) - m) * invB;
      }
    }
    ent = -ent;
    softmax_row_bwd(pr, dp, A, dz);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lds[L.Dq1 + t * 4 + k] = k < A ? dz[k] : 0.0f;
      if (t < nrows && k < A) ws.dlogit[(size_t)(row0 + t) * A + k] = dz[k];
    }
    if (t < nrows) {
      ws.terms[(size_t)(row0 + t) * 3 + 1] = (double)(-alpha * ent - minq);
      ws.terms[(size_t)(row0 + t) * 3 + 2] = (double)ent;
    }
  }
  __syncthreads();
  bwd_one(lds, {BwdItem{L.Dq1, 4, A, p.w[2], H, -1, nullptr, AH2, ld, R, X0, ld, ws.aZ2, H, nullptr}}, row0, nrows);
  bwd_stage(lds, {BwdItem{X0, ld, H, p.w[1], H, -1, nullptr, AH1, ld, R, -1, 0, ws.aZ1, H, im.ab}}, row0, nrows);      // (the last stage: no barrier behind it)
}

// T2: the two critics' tile lists in one launch, blocks [0, na) critic1's group, the rest critic2's (each group's last block
// closes that critic's loss sum)
struct Dw2 { DwArgs d[2]; int na; };
__global__ __launch_bounds__(256) void dsac_dw2_kernel(const Dw2 a) {
  __shared__ double sm[3][4];
  const int second = (int)blockIdx.x >= a.na;
  sac_dw_body(a.d[second], second ? (int)blockIdx.x - a.na : (int)blockIdx.x, second ? (int)gridDim.x - a.na : a.na, sm);
}

// ---- acting: actor logits, the categorical draw (gymrl_categorical_sample's keys), the env's step, replay row ----
// KIND: CartPole-v1 (gymrl_dsac_act_step, and gymrl_dsac_act_step_classic's kind 0), MountainCar-v0, Acrobot-v1
template <int HC, int KIND>
__global__ __launch_bounds__(kThreads) void dsac_act_kernel(const gymrl_dsac_act_args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int X0 = L.big, X1 = X0 + 16 * ld;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.N - row0);
  const int t = threadIdx.x;
  act_load_obs(a, lds, L, t, row0, nrows);
  const int R = GYMRL_ACT_RELU, kD = kMaxD, kA = kMaxA;
  const float* af = (a.images && (H & 15) == 0) ? a.images : nullptr;
  fwd_one(lds, {fwd_item(L.S, kD, -1, 0, D, D, H, a.actor.w[0], a.actor.b[0], X0, ld, nullptr, 0, R)}, row0, nrows);
  fwd_one(lds, {fwd_item(X0, ld, -1, 0, H, H, H, a.actor.w[1], a.actor.b[1], X1, ld, nullptr, 0, R, 0.0f, 0.0f, af)}, row0, nrows);
  fwd_one(lds, {fwd_item(X1, ld, -1, 0, H, H, A, a.actor.w[2], a.actor.b[2], L.Mean, kA, nullptr, 0, GYMRL_ACT_NONE)}, row0, nrows);
  // one lane per env: the draw, the env's step with auto-reset, replay row (the first wave: 16 lanes busy)
  if (t < 64) {
    constexpr int kActs = ClassicDims<KIND>::kActions;
    int act = 0;
    if (t < nrows) {
      float z[kActs];
#pragma unroll
      for (int k = 0; k < kActs; ++k) z[k] = lds[L.Mean + t * kMaxA + k];
      const uint64_t counter = a.counter_dev ? a.counter_dev[0] : a.counter;
      float lp, ent;
      act = categorical_pick<kActs>(z, a.noise_exp ? a.noise_exp + (size_t)(row0 + t) * kActs : nullptr, a.seed, (uint64_t)(a.env_id0 + row0 + t),
                                 counter, 0, lp, ent);
    }
    classic_act_tail<KIND>(a, lds, L, t, row0, nrows, act);
  }
}
// the instance of (hidden width, env kind); nullptr for a kind without one
using DsacActKernel = void (*)(const gymrl_dsac_act_args);
template <int KIND>
DsacActKernel dsac_act_instance(bool wide) { return wide ? dsac_act_kernel<256, KIND> : dsac_act_kernel<0, KIND>; }
DsacActKernel dsac_act_pick(int env_kind, bool wide) {
  switch (env_kind) {
    case GYMRL_ENV_CARTPOLE: return dsac_act_instance<GYMRL_ENV_CARTPOLE>(wide);
    case GYMRL_ENV_MOUNTAINCAR: return dsac_act_instance<GYMRL_ENV_MOUNTAINCAR>(wide);
    case GYMRL_ENV_ACROBOT: return dsac_act_instance<GYMRL_ENV_ACROBOT>(wide);
    default: return nullptr;
  }
}

__global__ __launch_bounds__(256) void softmax_rows_fwd_kernel(const float* __restrict__ z, int B, int A, float* __restrict__ p) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) softmax_row_fwd(z + (size_t)b * A, A, p + (size_t)b * A);
}
__global__ __launch_bounds__(256) void softmax_rows_bwd_kernel(const float* __restrict__ p, const float* __restrict__ g, int B, int A,
                                                               float* __restrict__ dz) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) softmax_row_bwd(p + (size_t)b * A, g + (size_t)b * A, A, dz + (size_t)b * A);
}

}  // namespace

extern "C" {

size_t gymrl_dsac_update_workspace_bytes(int B, int D, int A, int H) { return workspace_bytes<DsacWs>(B, D, A, H); }
size_t gymrl_dsac_args_bytes(int which) { return which == 0 ? sizeof(gymrl_dsac_act_args) : which == 1 ? sizeof(gymrl_dsac_update_args) : 0; }

static int dsac_set_lds_attr() {
  static bool done = false;
  return set_max_lds_once(done, {(const void*)dsac_r1_kernel<0>, (const void*)dsac_r1_kernel<256>, (const void*)dsac_r3_kernel<0>, (const void*)dsac_r3_kernel<256>,
                                 (const void*)dsac_act_pick(GYMRL_ENV_CARTPOLE, false), (const void*)dsac_act_pick(GYMRL_ENV_CARTPOLE, true)}, (int)lds_bytes(256, 6));
}
// (the MountainCar and Acrobot instances: raised on gymrl_dsac_act_step_classic's first call, so that a CartPole run's set-up is the parent's)
static int dsac_set_lds_attr_classic() {
  static bool done = false;
  return set_max_lds_once(done, {(const void*)dsac_act_pick(GYMRL_ENV_MOUNTAINCAR, false), (const void*)dsac_act_pick(GYMRL_ENV_MOUNTAINCAR, true),
                                 (const void*)dsac_act_pick(GYMRL_ENV_ACROBOT, false), (const void*)dsac_act_pick(GYMRL_ENV_ACROBOT, true)}, (int)lds_bytes(256, 6));
}
static int dsac_act_launch(const gymrl_dsac_act_args& a, void* stream_) {
  hipLaunchKernelGGL(dsac_act_pick(a.env_kind, a.H == 256), dim3((a.N + 15) / 16), dim3(kThreads), lds_bytes(a.H, 2), (hipStream_t)stream_, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_dsac_act_step(const gymrl_dsac_act_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_dsac_act_args& a = *args;
  if (!act_args_ok(a, GYMRL_ENV_CARTPOLE, /*refuse_neg_cursor=*/true) || !net_ok(a.actor)) return -22;
  if (const int rc = dsac_set_lds_attr()) return rc;
  return dsac_act_launch(a, stream_);
}

// the same launch for the env kind the block names: CartPole-v1, MountainCar-v0 or Acrobot-v1, each with its own (D, A)
int gymrl_dsac_act_step_classic(const gymrl_dsac_act_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_dsac_act_args& a = *args;
  if (!classic_act_kind_ok(a.env_kind) || !act_args_ok(a, a.env_kind, /*refuse_neg_cursor=*/true) || !net_ok(a.actor)) return -22;
  if (const int rc = dsac_set_lds_attr()) return rc;
  if (const int rc = dsac_set_lds_attr_classic()) return rc;
  return dsac_act_launch(a, stream_);
}

static bool dsac_update_args_ok(const gymrl_dsac_update_args& a) {
  if (!slab_shape_ok(a.B, kDsacMaxBatch, a.D, a.A, a.H)) return false;
  if (!ring_ok(a) || !all_set({a.workspace, a.sums, a.actor_p, a.actor_m, a.actor_v, a.critic1_p, a.critic1_m, a.critic1_v, a.critic2_p, a.critic2_m,
                               a.critic2_v, a.log_alpha, a.alpha_m, a.alpha_v}) ||
      !draw_ok(a, /*idx_dev_counts=*/true) || (!a.alpha_bias_dev && a.alpha_t <= 0))
    return false;
  return net_ok(a.actor) && net_ok(a.critic1) && net_ok(a.critic2) && net_ok(a.critic1_target) && net_ok(a.critic2_target);
}

int gymrl_dsac_pack_images(const gymrl_dsac_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_dsac_update_args& a = *args;
  if (!pack_args_ok(a) || !all_set({a.actor.w[1], a.critic1.w[1], a.critic2.w[1], a.critic1_target.w[1], a.critic2_target.w[1]})) return -22;
  hipLaunchKernelGGL(pack_images_kernel, dim3((a.H * a.H + 255) / 256, DsacImages::kCount), dim3(256), 0, (hipStream_t)stream_, DsacImages::sources(a), a.images, a.H);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_dsac_update(const gymrl_dsac_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_dsac_update_args& a = *args;
  if (!dsac_update_args_ok(a)) return -22;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = dsac_set_lds_attr()) return rc;
  DsacWs ws;
  DsacWs::carve(&ws, align256(a.workspace), a.B, a.D, a.A, a.H);
  const int B = a.B, D = a.D, A = a.A, H = a.H, slabs = (B + 15) / 16;
  const DsacImages im(a.images, H);
  const float tau = (float)a.tau, omt = (float)(1.0 - a.tau);
  // the tile lists of T2 (critic1, critic2) and T4 (actor)
  Dw2 c{};
  const gymrl_td3_actor_params* cn[2] = {&a.critic1, &a.critic2};
  const gymrl_td3_actor_params* tn[2] = {&a.critic1_target, &a.critic2_target};
  for (int i = 0; i < 2; ++i) {
    DwBuilder cb{c.d[i], B};
    cb.seg(ws.Z1[i], H, H, ws.s, D, nullptr, 0, D, D, cn[i]->w[0], cn[i]->b[0], tn[i]->w[0], tn[i]->b[0]);
    cb.seg(ws.Z2[i], H, H, ws.H1[i], H, nullptr, 0, H, H, cn[i]->w[1], cn[i]->b[1], tn[i]->w[1], tn[i]->b[1], im.cf[i], im.cb[i], im.tf[i]);
    cb.seg(ws.dq[i], A, A, ws.H2[i], H, nullptr, 0, H, H, cn[i]->w[2], cn[i]->b[2], tn[i]->w[2], tn[i]->b[2]);
    // (at most 256 rows: no slice partials)
    if (i == 0) cb.close(a, nullptr, a.critic1_p, a.critic1_m, a.critic1_v, a.adam_critic1, a.adam_critic1_dev, tau, omt, ws.terms, nullptr, 0, 1, a.sums);
    else cb.close(a, nullptr, a.critic2_p, a.critic2_m, a.critic2_v, a.adam_critic2, a.adam_critic2_dev, tau, omt, ws.terms, nullptr, 1, 1, a.sums);
  }
  const int nb0 = (c.d[0].total_waves + 3) / 4 + 1, nb1 = (c.d[1].total_waves + 3) / 4 + 1;
  c.na = nb0;
  DwArgs p{};
  DwBuilder pb{p, B};
  pb.seg(ws.aZ1, H, H, ws.s, D, nullptr, 0, D, D, a.actor.w[0], a.actor.b[0]);
  pb.seg(ws.aZ2, H, H, ws.aH1, H, nullptr, 0, H, H, a.actor.w[1], a.actor.b[1], nullptr, nullptr, im.af, im.ab);
  pb.seg(ws.dlogit, A, A, ws.aH2, H, nullptr, 0, H, H, a.actor.w[2], a.actor.b[2]);
  // (R3's terms sit in columns 1, 2 and go to sums[2], sums[3]: the body writes sums[term0 + k])
  pb.close(a, nullptr, a.actor_p, a.actor_m, a.actor_v, a.adam_actor, a.adam_actor_dev, tau, omt, ws.terms, nullptr, 1, 2, a.sums + 1);
  p.alpha_step = 2;                         // slab_step_device.hpp: dsac_alpha_kernel's float32 step in the block that closes the sums
  p.log_alpha_f = a.log_alpha; p.alpha_m_f = a.alpha_m; p.alpha_v_f = a.alpha_v; p.target_entropy_f = a.target_entropy;
  p.lr_alpha = a.lr_alpha; p.abeta1 = a.alpha_beta1; p.abeta2 = a.alpha_beta2; p.aeps = a.alpha_eps;
  p.alpha_t = a.alpha_t; p.alpha_bias_dev = a.alpha_bias_dev; p.alpha_loss = a.alpha_loss;
  const bool wide = H == 256;            // the instances built for the reference's hidden width
  hipLaunchKernelGGL(wide ? dsac_r1_kernel<256> : dsac_r1_kernel<0>, dim3(slabs), dim3(kThreads), lds_bytes(H, 6), stream, a, ws);
  hipLaunchKernelGGL(dsac_dw2_kernel, dim3(nb0 + nb1), dim3(256), 0, stream, c);
  hipLaunchKernelGGL(wide ? dsac_r3_kernel<256> : dsac_r3_kernel<0>, dim3(slabs), dim3(kThreads), lds_bytes(H, 6), stream, a, ws);
  hipLaunchKernelGGL(sac_dw_kernel, dim3((p.total_waves + 3) / 4 + 1), dim3(256), 0, stream, p);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_softmax_rows_fwd(const float* z, int B, int A, float* p_out, void* stream_) {
  if (!z || !p_out || B <= 0 || A <= 0 || A > kSoftmaxMaxA) return -22;
  hipLaunchKernelGGL(softmax_rows_fwd_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream_, z, B, A, p_out);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_softmax_rows_bwd(const float* p, const float* g, int B, int A, float* dz_out, void* stream_) {
  if (!p || !g || !dz_out || B <= 0 || A <= 0 || A > kSoftmaxMaxA) return -22;
  hipLaunchKernelGGL(softmax_rows_bwd_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream_, p, g, B, A, dz_out);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
