// td3_step.hip — TD3's and DDPG's Pendulum vector step (td3_pendulum.py:171-228, ddpg_pendulum.py:150-194) on the row-slab
// stages of slab_step_device.hpp:
//
//   td3_act_kernel   N/16 workgroups: actor forward, exploration noise, Pendulum step, replay row                   (acting)
//   td3_r1_kernel    B/16 workgroups: draw + gather, actor_target(s'), target critic(s), y, critic(s), dX chain     (rows)
//   td3_dw_kernel    sac_dw_body behind a delayed-step word: critic tiles + Adam (+ Polyak on delayed steps)        (tiles)
//   td3_r3_kernel    B/16 workgroups, delayed steps: actor(s), Q1(s, actor(s)), the chain back to the actor         (rows)
//   td3_dw_kernel    delayed steps: actor tiles + Adam + Polyak                                                     (tiles)
//
// SAC's step (offpolicy_step.hip) with a deterministic tanh actor,
// clipped Gaussian noise (offpolicy.hip noisy_action_kernel's two expressions) in place of the reparameterised sample, no
// temperature, one critic or two, and an actor phase that runs on the delayed steps only.  ONE workgroup carries a slab
// through a whole row phase: the chains that SAC deals to four workgroups ride along as items of the same stages (up to
// three H x H layers per stage on one compute unit), so nothing in these kernels waits for another workgroup — no flag, no
// counter — and a step that is not delayed can drop its actor phases by a return that is uniform over the grid.
#include "slab_step_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::slab;

constexpr int kTd3MaxBatch = 256;      // (ops.TD3_FUSED_MAX_BATCH) one grid of at most 16 slabs per row phase
struct Td3Images {                     // gymrl_td3_update_args.images, f32[9][H*H]: six forward images, then three input-gradient images
  const float *af, *cf[2], *tf[2], *atf, *ab, *cb[2];
  __host__ __device__ Td3Images(const float* base, int H) {
    const ImageSlots at(base, H);
    af = at(0); cf[0] = at(1); cf[1] = at(2); tf[0] = at(3); tf[1] = at(4); atf = at(5); ab = at(6); cb[0] = at(7); cb[1] = at(8);
  }
  // the same slots as the layers they are packed from (DDPG: the second network's stay null and are left alone)
  static constexpr int kCount = 9;
  static PackTable sources(const gymrl_td3_update_args& a) {
    return PackTable{{a.actor.w[1], a.critic.w[1], a.critic.w[4], a.critic_target.w[1], a.critic_target.w[4], a.actor_target.w[1],
                      a.actor.w[1], a.critic.w[1], a.critic.w[4]}, 6};
  }
};
__device__ __forceinline__ int td3_delayed(const gymrl_td3_update_args& a) { return a.delayed_dev ? a.delayed_dev[0] : a.delayed; }

// ---- R1: draw + gather, actor_target(s'), smoothing noise, target critic(s), y, critic(s) on (s, a), loss gradient, dX chain ----
template <int HC>
__global__ __launch_bounds__(kThreads) void td3_r1_kernel(const gymrl_td3_update_args a, const SacWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int X0 = L.big, X1 = X0 + 16 * ld, C1a = X1 + 16 * ld, C1b = C1a + 16 * ld, C2a = C1b + 16 * ld, C2b = C2a + 16 * ld;
  const int T0 = C2b + 16 * ld, T1 = T0 + 16 * ld;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const bool twin = a.n_critics == 2;
  const int Hn = twin ? H : 0, On = twin ? 1 : 0;      // the second network's items: no tiles when there is one critic
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD, kA = kMaxA;
  const Td3Images im(a.images, H);
  const gymrl_sac_critic_params &c = a.critic, &ct = a.critic_target;
  // ---- index draw + ring gather: one thread per row, rows beyond the batch are zero ----
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
    for (int j = 0; j < kMaxA; ++j) {
      const float av = (ok && j < A) ? __uint_as_float(a.r_action[row * A + j]) : 0.0f;
      lds[L.A + t * kMaxA + j] = av;
      if (ok && j < A) ws.a[(size_t)b * A + j] = av;
    }
    lds[L.Misc + t * 4 + 0] = ok ? a.r_reward[row] : 0.0f;
    lds[L.Misc + t * 4 + 1] = ok ? (float)a.r_flag[row] : 0.0f;            // dones become float32
  }
  __syncthreads();
  // ---- actor_target(s') next to critic(s, a): three independent chains, layer by layer ----
  {
    const FwdItem st[3] = {fwd_item(L.S2, kD, -1, 0, D, D, H, a.actor_target.w[0], a.actor_target.b[0], X0, ld, nullptr, 0, R),
                           fwd_item(L.S, kD, L.A, kA, D + A, D, H, c.w[0], c.b[0], C1a, ld, ws.H1[0], H, R),
                           fwd_item(L.S, kD, L.A, kA, D + A, D, Hn, c.w[3], c.b[3], C1b, ld, ws.H1[1], H, R)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[3] = {fwd_item(X0, ld, -1, 0, H, H, H, a.actor_target.w[1], a.actor_target.b[1], X1, ld, nullptr, 0, R, 0.0f, 0.0f, im.atf),
                           fwd_item(C1a, ld, -1, 0, H, H, H, c.w[1], c.b[1], C2a, ld, ws.H2[0], H, R, 0.0f, 0.0f, im.cf[0]),
                           fwd_item(C1b, ld, -1, 0, H, H, Hn, c.w[4], c.b[4], C2b, ld, ws.H2[1], H, R, 0.0f, 0.0f, im.cf[1])};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[3] = {fwd_item(X1, ld, -1, 0, H, H, A, a.actor_target.w[2], a.actor_target.b[2], L.Mean, kA, nullptr, 0, GYMRL_ACT_TANH),
                           fwd_item(C2a, ld, -1, 0, H, H, 1, c.w[2], c.b[2], L.Cq0, 4, nullptr, 0, NA),
                           fwd_item(C2b, ld, -1, 0, H, H, On, c.w[5], c.b[5], L.Cq1, 4, nullptr, 0, NA)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 16) {                           // a' (:191-196): offpolicy.hip noisy_action_kernel, mode 1
    const int b = row0 + t;
    const bool smooth = twin && a.policy_noise != 0.0;
    const uint64_t ncounter = a.noise_counter_dev ? a.noise_counter_dev[0] : a.noise_counter;
    for (int j = 0; j < kMaxA; ++j) {
      float v = 0.0f;
      if (t < nrows && j < A) {
        const float mu = lds[L.Mean + t * kMaxA + j] * a.bound;
        v = mu;
        if (smooth) {
          const int i = b * A + j;
          const double e = a.eps ? a.eps[i] : (double)box_muller(a.noise_seed, ncounter, 2u, (uint32_t)i);
          float nz = (float)e * (float)a.policy_noise;
          nz = fminf(fmaxf(nz, -a.noise_clip), a.noise_clip);
          v = fminf(fmaxf(mu + nz, -a.bound), a.bound);
        }
      }
      lds[L.A2 + t * kMaxA + j] = v;
    }
  }
  __syncthreads();
  // ---- the target critic(s) on (s', a') (:197) ----
  {
    const FwdItem st[2] = {fwd_item(L.S2, kD, L.A2, kA, D + A, D, H, ct.w[0], ct.b[0], X0, ld, nullptr, 0, R),
                           fwd_item(L.S2, kD, L.A2, kA, D + A, D, Hn, ct.w[3], ct.b[3], T0, ld, nullptr, 0, R)};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[2] = {fwd_item(X0, ld, -1, 0, H, H, H, ct.w[1], ct.b[1], X1, ld, nullptr, 0, R, 0.0f, 0.0f, im.tf[0]),
                           fwd_item(T0, ld, -1, 0, H, H, Hn, ct.w[4], ct.b[4], T1, ld, nullptr, 0, R, 0.0f, 0.0f, im.tf[1])};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[2] = {fwd_item(X1, ld, -1, 0, H, H, 1, ct.w[2], ct.b[2], L.Q0, 4, nullptr, 0, NA),
                           fwd_item(T1, ld, -1, 0, H, H, On, ct.w[5], ct.b[5], L.Q1, 4, nullptr, 0, NA)};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 16) {
    // y (:198-199; offpolicy.hip sac_target_kernel with log_alpha = 0 and a zero log-prob: alpha = 1, DDPG passes Q' twice), then
    // the loss gradient (:203-204; sac_critic_kernel / mse_kernel)
    const float alpha = (float)exp(0.0);
    const float q0 = lds[L.Q0 + t * 4], q1 = twin ? lds[L.Q1 + t * 4] : q0;
    const float tq = fminf(q0, q1) - alpha * 0.0f;
    const float y = lds[L.Misc + t * 4 + 0] + a.gamma * (1.0f - lds[L.Misc + t * 4 + 1]) * tq;
    const float invB = 1.0f / (float)a.B;
    for (int n = 0; n < a.n_critics; ++n) {
      const float e = lds[(n ? L.Cq1 : L.Cq0) + t * 4] - y;
      const float d = 2.0f * e * invB;
      for (int k = 0; k < 4; ++k) lds[(n ? L.Dq1 : L.Dq0) + t * 4 + k] = k == 0 ? d : 0.0f;
      if (t < nrows) {
        ws.dq[n][row0 + t] = d;
        if (n == 0) ws.terms[(size_t)(row0 + t) * 3 + 0] = (double)(e * e);
        else ws.terms2[row0 + t] = (double)(e * e);
      }
    }
  }
  __syncthreads();
  // ---- the critics' input-gradient chain (what backward() computes before the weight gradients) ----
  {
    const BwdItem st[2] = {BwdItem{L.Dq0, 4, 1, c.w[2], H, -1, nullptr, C2a, ld, R, X0, ld, ws.Z2[0], H, nullptr},
                           BwdItem{L.Dq1, 4, 1, c.w[5], Hn, -1, nullptr, C2b, ld, R, T0, ld, ws.Z2[1], H, nullptr}};
    bwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const BwdItem st[2] = {BwdItem{X0, ld, H, c.w[1], H, -1, nullptr, C1a, ld, R, -1, 0, ws.Z1[0], H, im.cb[0]},
                           BwdItem{T0, ld, H, c.w[4], Hn, -1, nullptr, C1b, ld, R, -1, 0, ws.Z1[1], H, im.cb[1]}};
    bwd_stage<2>(lds, st, row0, nrows);
  }
}

// ---- R3 (delayed steps): actor(s), Q1(s, actor(s)) of the updated critic, -mean's gradient back to the actor's first layer ----
template <int HC>
__global__ __launch_bounds__(kThreads) void td3_r3_kernel(const gymrl_td3_update_args a, const SacWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (!td3_delayed(a)) return;            // one word, the same for every workgroup of the grid
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int X0 = L.big, AH1 = X0 + 16 * ld, AH2 = AH1 + 16 * ld, H1 = AH2 + 16 * ld, H2 = H1 + 16 * ld;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD, kA = kMaxA;
  const Td3Images im(a.images, H);
  const gymrl_sac_critic_params& c = a.critic;
  if (t < 16) {
    const int b = row0 + t;
    for (int k = 0; k < kMaxD; ++k) lds[L.S + t * kMaxD + k] = (t < nrows && k < D) ? ws.s[(size_t)b * D + k] : 0.0f;
  }
  __syncthreads();
  fwd_one(lds, {fwd_item(L.S, kD, -1, 0, D, D, H, a.actor.w[0], a.actor.b[0], AH1, ld, ws.aH1, H, R)}, row0, nrows);
  fwd_one(lds, {fwd_item(AH1, ld, -1, 0, H, H, H, a.actor.w[1], a.actor.b[1], AH2, ld, ws.aH2, H, R, 0.0f, 0.0f, im.af)}, row0, nrows);
  fwd_one(lds, {fwd_item(AH2, ld, -1, 0, H, H, A, a.actor.w[2], a.actor.b[2], L.Mean, kA, nullptr, 0, GYMRL_ACT_TANH)}, row0, nrows);
  if (t < 16)
    for (int j = 0; j < kMaxA; ++j) lds[L.A + t * kMaxA + j] = (t < nrows && j < A) ? lds[L.Mean + t * kMaxA + j] * a.bound : 0.0f;
  __syncthreads();
  // ---- critic.q1(s, actor(s)) (:213): the parameters T2 has just written ----
  fwd_one(lds, {fwd_item(L.S, kD, L.A, kA, D + A, D, H, c.w[0], c.b[0], H1, ld, nullptr, 0, R)}, row0, nrows);
  fwd_one(lds, {fwd_item(H1, ld, -1, 0, H, H, H, c.w[1], c.b[1], H2, ld, nullptr, 0, R, 0.0f, 0.0f, im.cf[0])}, row0, nrows);
  fwd_one(lds, {fwd_item(H2, ld, -1, 0, H, H, 1, c.w[2], c.b[2], L.Q0, 4, nullptr, 0, NA)}, row0, nrows);
  if (t < 16) {                           // offpolicy.hip neg_mean_kernel
    const float g = -1.0f / (float)a.B;
    for (int k = 0; k < 4; ++k) lds[L.Dq0 + t * 4 + k] = k == 0 ? g : 0.0f;
    if (t < nrows) ws.terms[(size_t)(row0 + t) * 3 + 1] = (double)lds[L.Q0 + t * 4];
  }
  __syncthreads();
  // ---- back through the frozen critic to the action ----
  bwd_one(lds, {BwdItem{L.Dq0, 4, 1, c.w[2], H, -1, nullptr, H2, ld, R, X0, ld, nullptr, 0, nullptr}}, row0, nrows);
  bwd_one(lds, {BwdItem{X0, ld, H, c.w[1], H, -1, nullptr, H1, ld, R, H2, ld, nullptr, 0, im.cb[0]}}, row0, nrows);
  {
    const int lane = t & 63, wave = t >> 6, r = lane & 15, q = lane >> 4;
    if (wave == 0) {                      // d action = the action columns of dZ1 . W1
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      acc = lin::tile_bwd_input(acc, lds + H2, ld, H, c.w[0], D + A, 0, lane);
      if (r >= D && r < D + A) {
#pragma unroll
        for (int g = 0; g < 4; ++g) lds[L.A2 + (4 * q + g) * kMaxA + (r - D)] = acc[g];
      }
    }
  }
  __syncthreads();
  if (t < 16) {                           // through `* action_bound` and fc3's tanh (its dL/dz, from the saved output)
    for (int j = 0; j < 4; ++j) {
      float dz = 0.0f;
      if (j < A) {
        const float dy = lds[L.A2 + t * kMaxA + j] * a.bound;
        dz = dy * act_bwd(lds[L.Mean + t * kMaxA + j], GYMRL_ACT_TANH, 0.0f, 0.0f);
        if (t < nrows) ws.dmean[(size_t)(row0 + t) * A + j] = dz;
      }
      lds[L.Dq1 + t * 4 + j] = dz;
    }
  }
  __syncthreads();
  bwd_one(lds, {BwdItem{L.Dq1, 4, A, a.actor.w[2], H, -1, nullptr, AH2, ld, R, X0, ld, ws.aZ2, H, nullptr}}, row0, nrows);
  bwd_stage(lds, {BwdItem{X0, ld, H, a.actor.w[1], H, -1, nullptr, AH1, ld, R, -1, 0, ws.aZ1, H, im.ab}}, row0, nrows);      // (the last stage: no barrier behind it)
}

// T2 (gate = 0: every step; the target twins move on delayed steps only) and T4 (gate = 1: delayed steps only)
__global__ __launch_bounds__(256) void td3_dw_kernel(const DwArgs a, const int32_t* delayed_dev, const int delayed_host, const int gate) {
  __shared__ double sm[3][4];
  const int delayed = delayed_dev ? delayed_dev[0] : delayed_host;
  if (gate && !delayed) return;
  sac_dw_body(a, blockIdx.x, gridDim.x, sm, delayed != 0);
}

// ---- acting: actor forward, exploration noise (noisy_action_kernel mode 0), Pendulum step, replay row ----
template <int HC>
__global__ __launch_bounds__(kThreads) void td3_act_kernel(const gymrl_td3_act_args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int X0 = L.big, X1 = X0 + 16 * ld;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.N - row0);
  const int t = threadIdx.x;
  if (t < 16) {
    const int i = row0 + t;
    for (int k = 0; k < kMaxD; ++k) lds[L.S + t * kMaxD + k] = (t < nrows && k < D) ? a.obs[(size_t)i * D + k] : 0.0f;
  }
  __syncthreads();
  const int R = GYMRL_ACT_RELU, kD = kMaxD, kA = kMaxA;
  const float* af = (a.images && (H & 15) == 0) ? a.images : nullptr;
  fwd_one(lds, {fwd_item(L.S, kD, -1, 0, D, D, H, a.actor.w[0], a.actor.b[0], X0, ld, nullptr, 0, R)}, row0, nrows);
  fwd_one(lds, {fwd_item(X0, ld, -1, 0, H, H, H, a.actor.w[1], a.actor.b[1], X1, ld, nullptr, 0, R, 0.0f, 0.0f, af)}, row0, nrows);
  fwd_one(lds, {fwd_item(X1, ld, -1, 0, H, H, A, a.actor.w[2], a.actor.b[2], L.Mean, kA, nullptr, 0, GYMRL_ACT_TANH)}, row0, nrows);
  // one lane per env: noise, Pendulum step with auto-reset, replay row (the first wave: 16 lanes busy)
  if (t < 64) {
    float act[kMaxA];
    if (t < nrows) {
      const uint64_t ncounter = a.noise_counter_dev ? a.noise_counter_dev[0] : a.noise_counter;
      for (int j = 0; j < A; ++j) {
        const int e_i = (row0 + t) * A + j;
        const float mu = lds[L.Mean + t * kMaxA + j] * a.bound;
        const double e = a.eps ? a.eps[e_i] : (double)box_muller(a.noise_seed, ncounter, 2u, (uint32_t)e_i);
        double v = (double)mu + e * a.noise_std;
        v = v < -(double)a.bound ? -(double)a.bound : (v > (double)a.bound ? (double)a.bound : v);
        act[j] = (float)v;
      }
    }
    pendulum_act_tail(a, lds, L, t, row0, nrows, act);
  }
}

}  // namespace

extern "C" {

// (SAC's hand-off layout: the same slabs per network)
size_t gymrl_td3_update_workspace_bytes(int B, int D, int A, int H) { return workspace_bytes<SacWs>(B, D, A, H); }
size_t gymrl_td3_args_bytes(int which) { return which == 0 ? sizeof(gymrl_td3_act_args) : which == 1 ? sizeof(gymrl_td3_update_args) : 0; }

static int td3_set_lds_attr() {
  static bool done = false;
  return set_max_lds_once(done, {(const void*)td3_r1_kernel<0>, (const void*)td3_r1_kernel<256>, (const void*)td3_r3_kernel<0>, (const void*)td3_r3_kernel<256>,
                                 (const void*)td3_act_kernel<0>, (const void*)td3_act_kernel<256>}, (int)lds_bytes(256, 8));
}

int gymrl_td3_act_step(const gymrl_td3_act_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_td3_act_args& a = *args;
  if (!act_args_ok(a, GYMRL_ENV_PENDULUM, /*refuse_neg_cursor=*/true) || !net_ok(a.actor)) return -22;
  if (const int rc = td3_set_lds_attr()) return rc;
  hipLaunchKernelGGL(a.H == 256 ? td3_act_kernel<256> : td3_act_kernel<0>, dim3((a.N + 15) / 16), dim3(kThreads), lds_bytes(a.H, 2), (hipStream_t)stream_, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

static bool td3_update_args_ok(const gymrl_td3_update_args& a) {
  if (!slab_shape_ok(a.B, kTd3MaxBatch, a.D, a.A, a.H) || (a.n_critics != 1 && a.n_critics != 2)) return false;
  if (!ring_ok(a) || !all_set({a.workspace, a.sums, a.actor_p, a.actor_m, a.actor_v, a.critic_p, a.critic_m, a.critic_v}) ||
      !draw_ok(a, /*idx_dev_counts=*/true))
    return false;
  return net_ok(a.actor) && net_ok(a.actor_target) && net_ok(a.critic, 3 * a.n_critics) && net_ok(a.critic_target, 3 * a.n_critics);
}

int gymrl_td3_pack_images(const gymrl_td3_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_td3_update_args& a = *args;
  if (!pack_args_ok(a) || (a.n_critics != 1 && a.n_critics != 2)) return -22;
  if (!a.actor.w[1] || !a.actor_target.w[1] || !a.critic.w[1] || !a.critic_target.w[1] || (a.n_critics == 2 && (!a.critic.w[4] || !a.critic_target.w[4]))) return -22;
  hipLaunchKernelGGL(pack_images_kernel, dim3((a.H * a.H + 255) / 256, Td3Images::kCount), dim3(256), 0, (hipStream_t)stream_, Td3Images::sources(a), a.images, a.H);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_td3_update(const gymrl_td3_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_td3_update_args& a = *args;
  if (!td3_update_args_ok(a)) return -22;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = td3_set_lds_attr()) return rc;
  SacWs ws;
  SacWs::carve(&ws, align256(a.workspace), a.B, a.D, a.A, a.H);
  const int B = a.B, D = a.D, A = a.A, H = a.H, slabs = (B + 15) / 16;
  // the tile lists of T2 (critic: c) and T4 (actor: p), as sac_build_dw's
  const Td3Images im(a.images, H);
  const float tau = (float)a.tau, omt = (float)(1.0 - a.tau);
  DwArgs c{}, p{};
  DwBuilder cb{c, B}, pb{p, B};
  for (int i = 0; i < a.n_critics; ++i) {
    cb.seg(ws.Z1[i], H, H, ws.s, D, ws.a, A, D + A, D, a.critic.w[3 * i], a.critic.b[3 * i], a.critic_target.w[3 * i], a.critic_target.b[3 * i]);
    cb.seg(ws.Z2[i], H, H, ws.H1[i], H, nullptr, 0, H, H, a.critic.w[3 * i + 1], a.critic.b[3 * i + 1], a.critic_target.w[3 * i + 1], a.critic_target.b[3 * i + 1],
        im.cf[i], im.cb[i], im.tf[i]);
    cb.seg(ws.dq[i], 1, 1, ws.H2[i], H, nullptr, 0, H, H, a.critic.w[3 * i + 2], a.critic.b[3 * i + 2], a.critic_target.w[3 * i + 2], a.critic_target.b[3 * i + 2]);
  }
  cb.close(a, ws.dw_parts, a.critic_p, a.critic_m, a.critic_v, a.adam_critic, a.adam_critic_dev, tau, omt, ws.terms, a.n_critics == 2 ? ws.terms2 : nullptr, 0, 1, a.sums);
  pb.seg(ws.aZ1, H, H, ws.s, D, nullptr, 0, D, D, a.actor.w[0], a.actor.b[0], a.actor_target.w[0], a.actor_target.b[0]);
  pb.seg(ws.aZ2, H, H, ws.aH1, H, nullptr, 0, H, H, a.actor.w[1], a.actor.b[1], a.actor_target.w[1], a.actor_target.b[1], im.af, im.ab, im.atf);
  pb.seg(ws.dmean, A, A, ws.aH2, H, nullptr, 0, H, H, a.actor.w[2], a.actor.b[2], a.actor_target.w[2], a.actor_target.b[2]);
  pb.close(a, ws.dw_parts, a.actor_p, a.actor_m, a.actor_v, a.adam_actor, a.adam_actor_dev, tau, omt, ws.terms, nullptr, 1, 1, a.sums);
  const bool wide = H == 256;            // the instances built for the reference's hidden width
  hipLaunchKernelGGL(wide ? td3_r1_kernel<256> : td3_r1_kernel<0>, dim3(slabs), dim3(kThreads), lds_bytes(H, 8), stream, a, ws);
  hipLaunchKernelGGL(td3_dw_kernel, dim3((c.total_waves + 3) / 4 + 1), dim3(256), 0, stream, c, a.delayed_dev, a.delayed, 0);
  if (a.delayed_dev || a.delayed) {      // (a host-side zero: the actor phases are not even launched)
    hipLaunchKernelGGL(wide ? td3_r3_kernel<256> : td3_r3_kernel<0>, dim3(slabs), dim3(kThreads), lds_bytes(H, 5), stream, a, ws);
    hipLaunchKernelGGL(td3_dw_kernel, dim3((p.total_waves + 3) / 4 + 1), dim3(256), 0, stream, p, a.delayed_dev, a.delayed, 1);
  }
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
