// offpolicy_step.hip — a whole SAC vector step (sac_pendulum.py:269-310) in five launches.
//
// Round 3's step was ~60 launches of 4-14 us each (profiles/r03_sac_kernel_stats.csv: 0.325 ms per vector step, the acting
// forward at 0.03 of the f32-MFMA peak): every Linear of a 128-row batch is ~1 us of MFMA work behind a dispatch, a first
// load from L2 and a drain.  Nothing in a forward or input-gradient pass mixes batch rows, so here ONE workgroup of 16
// waves carries a 16-row slab of the batch through a whole chain of layers — activations in LDS, weights read from L2
// in nn.Linear's own layout, a workgroup barrier between layers — and only what reduces over the batch (weight
// gradients, loss sums) sits behind a kernel boundary:
//
//   sac_act_kernel   N/16 workgroups: Actor forward, reparameterised draw, Pendulum step, replay row         (acting)
//   sac_p1_kernel    B/16 workgroups: draw + gather, target chain, Q(s, a), loss gradient, critic dX chain    (rows)
//   sac_dw_kernel    one wave per 16 x 16 weight tile: dW tile, Adam on it, soft target update; loss sums    (tiles)
//   sac_p3_kernel    B/16 workgroups: actor forward + draw, Q(s, a) of the new critic, chain back to the actor (rows)
//   sac_dw_kernel    actor tiles + Adam; loss sums; the float64 temperature step                               (tiles)
//
// Every tile is computed by the device functions of lin_device.hpp — the MFMA sequence of gymrl_lin_fwd / _bwd_input /
// _bwd_weight — and every scalar expression is the one of the stand-alone kernels it replaces (offpolicy.hip sac_*,
// optim.hip adam_one / soft update, replay.hip, env_classic_device.hpp), so parameters, Adam moments, target network,
// temperature and replay ring after a step equal the layer-by-layer path's bit for bit (tests/test_fused_step_gpu.py).
//
// The stages, the LDS layout, the hand-off flags, the grid shapes and the tile kernel are slab_step_device.hpp's; Rainbow's
// step on them is rainbow_step.hip, TD3's and DDPG's td3_step.hip.
#include "slab_step_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::slab;

// Probe build only (make prof): 100 MHz wall-clock stamps at the stage boundaries of workgroup 0 (tools/probe_sac_stages.py)
#ifdef GYMRL_PROF_BUILD
__device__ long long g_step_prof[4][32];
#define STEP_MARK(k, i) do { if (threadIdx.x == 0 && bx == 0) g_step_prof[k][i] = (long long)wall_clock64(); } while (0)
#else
#define STEP_MARK(k, i) do {} while (0)
#endif
constexpr float kLogSqrt2Pi = 0.91893853320467274178f;   // math.log(math.sqrt(2*math.pi))

// Actor.sample's tail for one row (offpolicy.hip sac_sample_fwd_kernel, the same expressions)
__device__ __forceinline__ void sample_row(const float* mean, const float* log_std, const float* eps, int A, float bound, float* action,
                                           float& logp) {
  float lp = 0.0f;
  for (int j = 0; j < A; ++j) {
    const float mu = mean[j], std = det_expf(log_std[j]);
    const float x = mu + std * eps[j];
    const float t = det_tanhf(x);
    action[j] = t * bound;
    const float var = std * std, log_scale = det_logf(std);
    float l = -((x - mu) * (x - mu)) / (2.0f * var) - log_scale - kLogSqrt2Pi;
    l -= det_logf(bound * (1.0f - t * t) + 1e-6f);
    lp += l;
  }
  logp = lp;
}

struct Images {                        // gymrl_sac_update_args.images, f32[8][H*H]: five forward images, then three input-gradient images
  const float *af, *c1f, *c2f, *t1f, *t2f, *ab, *c1b, *c2b;
  __host__ __device__ Images(const float* base, int H) {
    const ImageSlots at(base, H);
    af = at(0); c1f = at(1); c2f = at(2); t1f = at(3); t2f = at(4); ab = at(5); c1b = at(6); c2b = at(7);
  }
  // the same slots as the layers they are packed from
  static constexpr int kCount = 8;
  static PackTable sources(const gymrl_sac_update_args& a) {
    return PackTable{{a.actor.w[1], a.critic.w[1], a.critic.w[4], a.target.w[1], a.target.w[4], a.actor.w[1], a.critic.w[1], a.critic.w[4]}, 5};
  }
};

// ======================================================================================================== P1 =====
// Four workgroups per 16-row slab (blockIdx.y): ONE compute unit's f32 MFMA rate is what a slab's stage costs, so every
// chain that does not depend on another runs on a compute unit of its own —
//   0 / 1  the target chain of target network 1 / 2: actor(s'), a' and logp' (both compute them: nothing is waited for), then
//          THEIR network's Q(s', a') (:233-236), posted with a release flag per consumer;
//   2 / 3  the critic chain of Q network 1 / 2: Q(s, a) (:239), then — both target columns taken — y (:237), the loss gradient
//          and the input-gradient chain of its network (:240-241).  Workgroup 2 also runs the ACTOR step's forward (:248) in
//          the time it would otherwise wait.
// All workgroups of every slab are resident (4 * B / 16 <= 64 of 256 CUs) and the producers wait for nobody: no deadlock.
// Every flag has one writer and one reader, who clears it.  Same layers, same order per element as the per-layer path.
//
// Each kernel of this file is a __forceinline__ body and the __global__ function that calls it, on purpose: with the body written
// into the kernel, where the argument struct is the by-value parameter itself and not a reference to it, hipcc gives the kernels
// scratch (sac_p1 / sac_p3 <256>: 0 -> 80 bytes per lane, sac_act: 56 -> 128; profiles/sac_one_launch_removal_ab.txt)
template <int HC>
__device__ __forceinline__ void sac_p1_body(const gymrl_sac_update_args& a, const SacWs& ws, float* lds, const int bx, const int role, const int S) {
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);      // HC: the hidden width this instance is built for (0: any)
  const int X0 = L.big, X1 = X0 + 16 * ld, H1a = X1 + 16 * ld, H1b = H1a + 16 * ld, H2a = H1b + 16 * ld, H2b = H2a + 16 * ld;
  const int T2a = H2b + 16 * ld, T2b = T2a + 16 * ld;
  const int row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const bool target_chain = role < 2;
  const int n = role & 1;                                // which of the twin networks this workgroup carries
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD, kA = kMaxA;
  const Images im(a.images, H);
  unsigned int* const f_t[2] = {ws.flag + (size_t)n * S + bx, ws.flag + (size_t)(5 + n) * S + bx};   // target net 1 / 2 -> critic workgroup n
#define P1_MARK_T(i) do { if (role == 0) STEP_MARK(3, i); } while (0)
#define P1_MARK_C(i) do { if (role == 2) STEP_MARK(0, i); } while (0)
  // ---- 0: index draw + ring gather (one thread per row; rows beyond the batch are zero); each workgroup takes what its chain reads ----
  P1_MARK_T(0); P1_MARK_C(0);
  // the narrow layers' parameters into slabs this role leaves free (Stager): target chain X0 / X1 / T2a busy, critic chain
  // H1a / H2a / X0 (+ T2a / T2b in the workgroup that also runs the actor step's forward)
  const float *aw0 = nullptr, *ab0 = nullptr, *aw2 = nullptr, *aw3 = nullptr, *ab2 = nullptr, *ab3 = nullptr;   // actor fc1, heads
  const float *qw0, *qb0, *qw2, *qb2;                                                                            // this role's Q network: fc1, fc3
  Stager sg{lds, target_chain ? H1a : X1};
  {
    const gymrl_sac_critic_params& net = target_chain ? a.target : a.critic;
    qw0 = sg.put(net.w[3 * n], H * (D + A)); qb0 = sg.put(net.b[3 * n], H);
    qw2 = sg.put(net.w[3 * n + 2], H); qb2 = sg.put(net.b[3 * n + 2], 1);
    if (target_chain || n == 0) {
      sg.at = H1b;
      aw0 = sg.put(a.actor.w[0], H * D); ab0 = sg.put(a.actor.b[0], H);
      sg.at = H2b;
      aw2 = sg.put(a.actor.w[2], A * H); aw3 = sg.put(a.actor.w[3], A * H);
      ab2 = sg.put(a.actor.b[2], A); ab3 = sg.put(a.actor.b[3], A);
    }
    sg.issue();
  }
  int64_t row = 0;
  if (t < nrows) row = replay_draw_row(a, row0 + t);
  sg.commit();
  if (t < 16) {
    const int b = row0 + t;
    const bool ok = t < nrows;
    if (target_chain) {
      for (int k = 0; k < kMaxD; ++k) lds[L.S2 + t * kMaxD + k] = (ok && k < D) ? a.r_next[row * D + k] : 0.0f;
      // (no explicit draws from the caller: NoisyNet's Box-Muller on the fused step's own stream ids — 2 acting, 3 a', 4 the actor step)
      const uint64_t ncounter = a.noise_counter_dev ? a.noise_counter_dev[0] : a.noise_counter;
      for (int j = 0; j < kMaxA; ++j) {
        float e = 0.0f;
        if (ok && j < A) e = a.eps_next ? a.eps_next[(size_t)b * A + j] : box_muller(a.noise_seed, ncounter, 3u, (uint32_t)(b * A + j));
        lds[L.Eps + t * kMaxA + j] = e;
      }
      lds[L.Misc + t * 4 + 0] = ok ? a.r_reward[row] : 0.0f;
      lds[L.Misc + t * 4 + 1] = ok ? (float)a.r_flag[row] : 0.0f;          // dones become float32 (dqn_cartpole.py:155)
    } else {
      for (int k = 0; k < kMaxD; ++k) {
        const float sv = (ok && k < D) ? a.r_state[row * D + k] : 0.0f;
        lds[L.S + t * kMaxD + k] = sv;
        if (n == 0 && ok && k < D) ws.s[(size_t)b * D + k] = sv;
      }
      for (int j = 0; j < kMaxA; ++j) {
        const float av = (ok && j < A) ? __uint_as_float(a.r_action[row * A + j]) : 0.0f;
        lds[L.A + t * kMaxA + j] = av;
        if (n == 0 && ok && j < A) ws.a[(size_t)b * A + j] = av;
      }
    }
  }
  __syncthreads();
  if (target_chain) {
    P1_MARK_T(1);
    // ---- the actor on s' (:233) ----
    fwd_one(lds, {fwd_item(L.S2, kD, -1, 0, D, D, H, aw0, ab0, X0, ld, nullptr, 0, R)}, row0, nrows);
    P1_MARK_T(2);
    fwd_one(lds, {fwd_item(X0, ld, -1, 0, H, H, H, a.actor.w[1], a.actor.b[1], X1, ld, nullptr, 0, R, 0.0f, 0.0f, im.af)}, row0, nrows);
    P1_MARK_T(3);
    {
      const FwdItem st[2] = {fwd_item(X1, ld, -1, 0, H, H, A, aw2, ab2, L.Mean, kA, nullptr, 0, NA),
                             fwd_item(X1, ld, -1, 0, H, H, A, aw3, ab3, L.Ls, kA, nullptr, 0, GYMRL_ACT_CLAMP, a.log_std_min, a.log_std_max)};
      fwd_stage<2>(lds, st, row0, nrows);
    }
    __syncthreads();
    P1_MARK_T(4);
    if (t < 16) {                         // a', logp' (:234)
      float lp;
      sample_row(lds + L.Mean + t * kMaxA, lds + L.Ls + t * kMaxA, lds + L.Eps + t * kMaxA, A, a.bound, lds + L.A2 + t * kMaxA, lp);
      lds[L.Misc + t * 4 + 2] = lp;
    }
    __syncthreads();
    P1_MARK_T(5);
    // ---- target Q(s', a') of this workgroup's network (:235-236) ----
    fwd_one(lds, {fwd_item(L.S2, kD, L.A2, kA, D + A, D, H, qw0, qb0, X0, ld, nullptr, 0, R)}, row0, nrows);
    P1_MARK_T(6);
    fwd_one(lds, {fwd_item(X0, ld, -1, 0, H, H, H, a.target.w[3 * n + 1], a.target.b[3 * n + 1], T2a, ld, nullptr, 0, R, 0.0f, 0.0f, n ? im.t2f : im.t1f)}, row0, nrows);
    P1_MARK_T(7);
    fwd_one(lds, {fwd_item(T2a, ld, -1, 0, H, H, 1, qw2, qb2, L.Q0, 4, nullptr, 0, NA)}, row0, nrows);
    P1_MARK_T(8);
    if (t < 16) {                         // (16 slots per slab: the columns are padded to whole slabs)
      xstore(ws.xtq[n] + row0 + t, lds[L.Q0 + t * 4]);
      if (n == 0) {
        for (int k = 0; k < 3; ++k) xstore(ws.xmisc + (size_t)(row0 + t) * 4 + k, lds[L.Misc + t * 4 + k]);
      }
    }
    __syncthreads();
    if (t == 0) { flag_post(ws.flag + (size_t)(n ? 5 : 0) * S + bx); flag_post(ws.flag + (size_t)(n ? 6 : 1) * S + bx); }
    P1_MARK_T(9);
    return;
  }
  P1_MARK_C(1);
  // ---- Q(s, a) of this workgroup's network (:239) ----
  fwd_one(lds, {fwd_item(L.S, kD, L.A, kA, D + A, D, H, qw0, qb0, H1a, ld, ws.H1[n], H, R)}, row0, nrows);
  P1_MARK_C(2);
  fwd_one(lds, {fwd_item(H1a, ld, -1, 0, H, H, H, a.critic.w[3 * n + 1], a.critic.b[3 * n + 1], H2a, ld, ws.H2[n], H, R, 0.0f, 0.0f, n ? im.c2f : im.c1f)}, row0, nrows);
  P1_MARK_C(3);
  fwd_one(lds, {fwd_item(H2a, ld, -1, 0, H, H, 1, qw2, qb2, L.Cq0, 4, nullptr, 0, NA)}, row0, nrows);
  P1_MARK_C(4);
  // ---- while the target chains are still on their way: a, logp = Actor.sample(s) of the ACTOR step (:248).  It reads the
  // actor's parameters only, which nothing touches before P4 — so it is the work of P3 that does not have to wait for the
  // critic's update (P2), done here in the first critic workgroup's idle time; P3 starts from what is saved. ----
  if (n == 0) {
    const int AH1 = T2a, AH2 = T2b;                    // (P3's slab positions)
    if (t < 16) {
      const int b = row0 + t;
      const bool ok = t < nrows;
      const uint64_t ncounter = a.noise_counter_dev ? a.noise_counter_dev[0] : a.noise_counter;
      for (int j = 0; j < kMaxA; ++j) {
        float e = 0.0f;
        if (ok && j < A) e = a.eps_cur ? a.eps_cur[(size_t)b * A + j] : box_muller(a.noise_seed, ncounter, 4u, (uint32_t)(b * A + j));
        lds[L.Eps + t * kMaxA + j] = e;
      }
    }
    fwd_one(lds, {fwd_item(L.S, kD, -1, 0, D, D, H, aw0, ab0, AH1, ld, ws.aH1, H, R)}, row0, nrows);
    fwd_one(lds, {fwd_item(AH1, ld, -1, 0, H, H, H, a.actor.w[1], a.actor.b[1], AH2, ld, ws.aH2, H, R, 0.0f, 0.0f, im.af)}, row0, nrows);
    {
      const FwdItem st[2] = {fwd_item(AH2, ld, -1, 0, H, H, A, aw2, ab2, L.Mean, kA, nullptr, 0, NA),
                             fwd_item(AH2, ld, -1, 0, H, H, A, aw3, ab3, L.Ls, kA, nullptr, 0, GYMRL_ACT_CLAMP, a.log_std_min, a.log_std_max)};
      fwd_stage<2>(lds, st, row0, nrows);
    }
    __syncthreads();
    if (t < 16) {
      float lp;
      sample_row(lds + L.Mean + t * kMaxA, lds + L.Ls + t * kMaxA, lds + L.Eps + t * kMaxA, A, a.bound, lds + L.A2 + t * kMaxA, lp);
      const size_t o = (size_t)(row0 + t) * kMaxA;
      for (int j = 0; j < kMaxA; ++j) {
        ws.xa[o + j] = lds[L.A2 + t * kMaxA + j]; ws.xmean[o + j] = lds[L.Mean + t * kMaxA + j];
        ws.xls[o + j] = lds[L.Ls + t * kMaxA + j]; ws.xeps[o + j] = lds[L.Eps + t * kMaxA + j];
      }
      ws.xlp[row0 + t] = lp;
    }
  }
  // ---- both target columns ----
  if (t == 0) { flag_wait(f_t[0]); flag_wait(f_t[1]); }
  __syncthreads();
  P1_MARK_C(5);
  if (t < 16) {
    // y (:237; offpolicy.hip sac_target_kernel), then the critic loss gradient (:240-241; sac_critic_kernel)
    const float alpha = (float)exp(a.log_alpha[0]);
    const float* mi = ws.xmisc + (size_t)(row0 + t) * 4;
    const float tq = fminf(xload(ws.xtq[0] + row0 + t), xload(ws.xtq[1] + row0 + t)) - alpha * xload(mi + 2);
    const float y = xload(mi + 0) + a.gamma * (1.0f - xload(mi + 1)) * tq;
    const float invB = 1.0f / (float)a.B;
    const float e = lds[L.Cq0 + t * 4] - y;
    const float d = 2.0f * e * invB;
    for (int k = 0; k < 4; ++k) lds[L.Dq0 + t * 4 + k] = k == 0 ? d : 0.0f;
    if (t < nrows) {
      ws.dq[n][row0 + t] = d;
      if (n == 0) ws.terms[(size_t)(row0 + t) * 3 + 0] = (double)(e * e);       // the row's critic term = this + terms2 (P2 adds them)
      else ws.terms2[row0 + t] = (double)(e * e);
    }
  }
  __syncthreads();
  if (t == 0) { flag_clear(f_t[0]); flag_clear(f_t[1]); }                        // consumed: ready for the next launch
  P1_MARK_C(6);
  // ---- input-gradient chain of this Q network (what q.backward() computes before the weight gradients) ----
  bwd_one(lds, {BwdItem{L.Dq0, 4, 1, qw2, H, -1, nullptr, H2a, ld, R, X0, ld, ws.Z2[n], H, nullptr}}, row0, nrows);
  P1_MARK_C(7);
  bwd_stage(lds, {BwdItem{X0, ld, H, a.critic.w[3 * n + 1], H, -1, nullptr, H1a, ld, R, -1, 0, ws.Z1[n], H, n ? im.c2b : im.c1b}}, row0, nrows);      // (the last stage: no barrier behind it)
  P1_MARK_C(8);
#undef P1_MARK_T
#undef P1_MARK_C
}

template <int HC>
__global__ __launch_bounds__(kThreads) void sac_p1_kernel(const gymrl_sac_update_args a, const SacWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int order[4] = {0, 1, 2, 3};                 // the two target chains wait for nobody; the critic chains wait for them
  const SlabGrid g = slab_grid<4>(ws.sync, order);
  sac_p1_body<HC>(a, ws, lds, g.slab, g.role, g.slabs);
  slab_grid_done(g);
}

// ======================================================================================================== P3 =====
// Two workgroups per slab here as well (blockIdx.y), both starting from the sample P1 saved: workgroup 0 carries Q2 and the
// way back through the actor, workgroup 1 (the helper) only Q1 — forward, backward to its first layer's dZ.  They exchange
// the two Q columns (both ways: the min's tie rule needs both) and the helper's half of d action (1 -> 0): d action is ONE
// accumulator chain over both networks in the per-layer path (Q1's terms, then Q2's), so the helper runs Q1's half and
// workgroup 0 goes on from its 16 x A partial sums.
template <int HC>
__device__ __forceinline__ void sac_p3_body(const gymrl_sac_update_args& a, const SacWs& ws, float* lds, const int bx, const int by, const int S) {
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);      // HC: the hidden width this instance is built for (0: any)
  const int X0 = L.big, X1 = X0 + 16 * ld, H1a = X1 + 16 * ld, H1b = H1a + 16 * ld, H2a = H1b + 16 * ld, H2b = H2a + 16 * ld;
  const int AH1 = H2b + 16 * ld, AH2 = AH1 + 16 * ld;
  const int row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const bool helper = by == 1;                           // the workgroup that carries Q1 only; workgroup 0: the actor and Q2
  unsigned int* f_q[2] = {ws.flag + 2 * S + bx, ws.flag + 3 * S + bx};
  unsigned int* f_dz = ws.flag + 4 * S + bx;
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD, kA = kMaxA;
  const Images im(a.images, H);
  if (!helper) STEP_MARK(1, 0);
  // the batch's states and the actor step's sample (a, logp, mean, log_std, eps: P1 computed them); workgroup 0 also takes the
  // actor's two activation slabs back for the way home
  if (t < 16) {
    const int b = row0 + t;
    const bool ok = t < nrows;
    for (int k = 0; k < kMaxD; ++k) lds[L.S + t * kMaxD + k] = (ok && k < D) ? ws.s[(size_t)b * D + k] : 0.0f;
    const size_t o = (size_t)(row0 + t) * kMaxA;
    for (int j = 0; j < kMaxA; ++j) {
      lds[L.A + t * kMaxA + j] = ws.xa[o + j];
      if (!helper) { lds[L.Mean + t * kMaxA + j] = ws.xmean[o + j]; lds[L.Ls + t * kMaxA + j] = ws.xls[o + j]; lds[L.Eps + t * kMaxA + j] = ws.xeps[o + j]; }
    }
    if (!helper) lds[L.Misc + t * 4 + 2] = ws.xlp[row0 + t];
  }
  if (!helper) {
    for (int e = t; e < 16 * H; e += kThreads) {
      const int rr = e / H, c = e % H;
      const bool ok = rr < nrows;
      lds[AH1 + rr * ld + c] = ok ? ws.aH1[(size_t)(row0 + rr) * H + c] : 0.0f;
      lds[AH2 + rr * ld + c] = ok ? ws.aH2[(size_t)(row0 + rr) * H + c] : 0.0f;
    }
  }
  // the narrow layers' parameters into a slab this workgroup leaves free (Stager): its Q network's fc1 and fc3 — forward, and
  // fc1 again as the d action chain's operand — and, for the way home, the actor's heads
  const int n = helper ? 0 : 1;
  const int H1n = n ? H1b : H1a, H2n = n ? H2b : H2a, Xn = n ? X1 : X0, Qn = n ? L.Q1 : L.Q0, Dqn = n ? L.Dq1 : L.Dq0;
  Stager sg{lds, n ? H1a : H1b};
  const float* qw0 = sg.put(a.critic.w[3 * n], H * (D + A)); const float* qb0 = sg.put(a.critic.b[3 * n], H);
  const float* qw2 = sg.put(a.critic.w[3 * n + 2], H); const float* qb2 = sg.put(a.critic.b[3 * n + 2], 1);
  const float *aw2 = nullptr, *aw3 = nullptr;
  if (!helper) { sg.at = H2a; aw2 = sg.put(a.actor.w[2], A * H); aw3 = sg.put(a.actor.w[3], A * H); }
  sg.run();
  __syncthreads();
  if (!helper) STEP_MARK(1, 1);
  // ---- Q(s, a) of the critic P2 has just updated (:249-250): this workgroup's network ----
  fwd_one(lds, {fwd_item(L.S, kD, L.A, kA, D + A, D, H, qw0, qb0, H1n, ld, nullptr, 0, R)}, row0, nrows);
  if (!helper) STEP_MARK(1, 2);
  fwd_one(lds, {fwd_item(H1n, ld, -1, 0, H, H, H, a.critic.w[3 * n + 1], a.critic.b[3 * n + 1], H2n, ld, nullptr, 0, R, 0.0f, 0.0f, n ? im.c2f : im.c1f)}, row0, nrows);
  if (!helper) STEP_MARK(1, 3);
  fwd_one(lds, {fwd_item(H2n, ld, -1, 0, H, H, 1, qw2, qb2, Qn, 4, nullptr, 0, NA)}, row0, nrows);
  if (!helper) STEP_MARK(1, 4);
  // the two Q columns meet: each workgroup posts its own, takes the other's
  if (t < 16) xstore(ws.xq[n] + row0 + t, lds[Qn + t * 4]);
  __syncthreads();
  if (t == 0) { flag_post(f_q[n]); flag_wait(f_q[1 - n]); }
  __syncthreads();
  float dlogp = 0.0f;
  if (t < 16) {                         // offpolicy.hip sac_actor_kernel
    const float other = xload(ws.xq[1 - n] + row0 + t);
    const float own = lds[Qn + t * 4];
    const float qa = n ? other : own, qc = n ? own : other;            // Q1, Q2
    const float invB = 1.0f / (float)a.B;
    const float w1 = qa < qc ? 1.0f : (qa == qc ? 0.5f : 0.0f);          // torch.min tie rule
    const float dn = n ? -(1.0f - w1) * invB : -w1 * invB;
    for (int k = 0; k < 4; ++k) lds[Dqn + t * 4 + k] = k == 0 ? dn : 0.0f;
    if (!helper) {
      const float alpha = (float)exp(a.log_alpha[0]);
      const float lp = lds[L.Misc + t * 4 + 2];
      dlogp = alpha * invB;
      if (t < nrows) {
        ws.terms[(size_t)(row0 + t) * 3 + 1] = (double)(alpha * lp - fminf(qa, qc));
        ws.terms[(size_t)(row0 + t) * 3 + 2] = (double)(lp + a.target_entropy);
      }
    }
  }
  __syncthreads();
  if (t == 0) flag_clear(f_q[1 - n]);
  if (!helper) STEP_MARK(1, 5);
  // ---- back through this workgroup's Q network to its first layer (the parameters are frozen here: no weight gradients) ----
  bwd_one(lds, {BwdItem{Dqn, 4, 1, qw2, H, -1, nullptr, H2n, ld, R, Xn, ld, nullptr, 0, nullptr}}, row0, nrows);
  if (!helper) STEP_MARK(1, 6);
  bwd_one(lds, {BwdItem{Xn, ld, H, a.critic.w[3 * n + 1], H, -1, nullptr, H1n, ld, R, H2n, ld, nullptr, 0, n ? im.c2b : im.c1b}}, row0, nrows);
  // d action = the action columns of (dZ1_Q1 . W1_Q1 + dZ1_Q2 . W1_Q2): ONE accumulator over both networks (the layers share their
  // input), network 1's terms first.  The helper runs its half of the chain and hands the 16 x A partial sums over (wave 0's own
  // stores, published by its lane 0's release); workgroup 0 goes on from them with network 2's terms — the same MFMA sequence
  // per element as the one-workgroup chain, and 16 x A floats cross instead of a 16 x H slab.
  {
    const int lane = t & 63, wave = t >> 6, r = lane & 15, q = lane >> 4;
    const bool mine = r >= D && r < D + A;
    if (helper) {
      if (wave == 0) {
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        acc = lin::tile_bwd_input(acc, lds + H2n, ld, H, qw0, D + A, 0, lane);
        if (mine) {
#pragma unroll
          for (int g = 0; g < 4; ++g) xstore(ws.xpart + (size_t)(row0 + 4 * q + g) * kMaxA + (r - D), acc[g]);
        }
        if (lane == 0) flag_post(f_dz);
      }
      return;
    }
    STEP_MARK(1, 7);
    if (wave == 0) {
      if (lane == 0) flag_wait(f_dz);
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      if (mine) {
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = xload(ws.xpart + (size_t)(row0 + 4 * q + g) * kMaxA + (r - D));
      }
      acc = lin::tile_bwd_input(acc, lds + H2n, ld, H, qw0, D + A, 0, lane);
      if (mine) {
#pragma unroll
        for (int g = 0; g < 4; ++g) lds[L.A2 + (4 * q + g) * kMaxA + (r - D)] = acc[g];
      }
      if (lane == 0) flag_clear(f_dz);
    }
  }
  __syncthreads();
  STEP_MARK(1, 8);
  if (t < 16) {                         // offpolicy.hip sac_sample_bwd_kernel, then the heads' dL/dz (log_std through its clamp)
    for (int j = 0; j < kMaxA; ++j) {
      float dm = 0.0f, dl = 0.0f;
      if (j < A) {
        const float mu = lds[L.Mean + t * kMaxA + j], ls = lds[L.Ls + t * kMaxA + j], e = lds[L.Eps + t * kMaxA + j];
        const float std = det_expf(ls);
        const float x = mu + std * e;
        const float th = det_tanhf(x);
        const float omt = 1.0f - th * th;
        const float ga = lds[L.A2 + t * kMaxA + j], gl = dlogp;
        const float dx = ga * a.bound * omt + gl * (2.0f * th * a.bound * omt / (a.bound * omt + 1e-6f));
        dm = dx;
        dl = (dx * (std * e) - gl) * act_bwd(ls, GYMRL_ACT_CLAMP, a.log_std_min, a.log_std_max);
        if (t < nrows) { ws.dmean[(size_t)(row0 + t) * A + j] = dm; ws.dls[(size_t)(row0 + t) * A + j] = dl; }
      }
      lds[L.Dq0 + t * 4 + j] = dm; lds[L.Dq1 + t * 4 + j] = dl;
    }
  }
  __syncthreads();
  STEP_MARK(1, 9);
  // ---- back through the actor: heads (one summed input gradient), fc2 ----
  bwd_one(lds, {BwdItem{L.Dq0, 4, A, aw2, H, L.Dq1, aw3, AH2, ld, R, X0, ld, ws.aZ2, H, nullptr}}, row0, nrows);
  STEP_MARK(1, 10);
  bwd_stage(lds, {BwdItem{X0, ld, H, a.actor.w[1], H, -1, nullptr, AH1, ld, R, -1, 0, ws.aZ1, H, im.ab}}, row0, nrows);      // (the last stage: no barrier behind it)
  STEP_MARK(1, 11);
}

template <int HC>
__global__ __launch_bounds__(kThreads) void sac_p3_kernel(const gymrl_sac_update_args a, const SacWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int order[2] = {0, 1};                       // they exchange both ways: case (b) of slab_grid's comment
  const SlabGrid g = slab_grid<2>(ws.sync + 2, order);
  sac_p3_body<HC>(a, ws, lds, g.slab, g.role, g.slabs);
  slab_grid_done(g);
}

// ==================================================================================================== acting =====
template <int HC>
__device__ __forceinline__ void sac_act_body(const gymrl_sac_act_args& a, float* lds, const int bx) {
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);      // HC: the hidden width this instance is built for (0: any)
  const int X0 = L.big, X1 = X0 + 16 * ld;
  const int row0 = bx * 16, nrows = min(16, a.N - row0);
  const int t = threadIdx.x;
  STEP_MARK(2, 0);
  Stager sg{lds, X1 + 16 * ld};                          // (slabs 2, 3)
  const float* w0 = sg.put(a.actor.w[0], H * D); const float* b0 = sg.put(a.actor.b[0], H);
  const float* w2 = sg.put(a.actor.w[2], A * H); const float* w3 = sg.put(a.actor.w[3], A * H);
  const float* b2 = sg.put(a.actor.b[2], A); const float* b3 = sg.put(a.actor.b[3], A);
  sg.run();
  if (t < 16) {
    const int i = row0 + t;
    const bool ok = t < nrows;
    for (int k = 0; k < kMaxD; ++k) lds[L.S + t * kMaxD + k] = (ok && k < D) ? a.obs[(size_t)i * D + k] : 0.0f;
    const uint64_t ncounter = a.noise_counter_dev ? a.noise_counter_dev[0] : a.noise_counter;
    for (int j = 0; j < kMaxA; ++j) {
      float e = 0.0f;
      if (ok && j < A) e = a.eps ? a.eps[(size_t)i * A + j] : box_muller(a.noise_seed, ncounter, 2u, (uint32_t)(i * A + j));
      lds[L.Eps + t * kMaxA + j] = e;
    }
  }
  __syncthreads();
  STEP_MARK(2, 1);
  const int R = GYMRL_ACT_RELU, kD = kMaxD, kA = kMaxA;
  const Images im(a.images, H);
  fwd_one(lds, {fwd_item(L.S, kD, -1, 0, D, D, H, w0, b0, X0, ld, nullptr, 0, R)}, row0, nrows);
  STEP_MARK(2, 2);
  fwd_one(lds, {fwd_item(X0, ld, -1, 0, H, H, H, a.actor.w[1], a.actor.b[1], X1, ld, nullptr, 0, R, 0.0f, 0.0f, im.af)}, row0, nrows);
  STEP_MARK(2, 3);
  {
    const FwdItem st[2] = {fwd_item(X1, ld, -1, 0, H, H, A, w2, b2, L.Mean, kA, nullptr, 0, GYMRL_ACT_NONE),
                           fwd_item(X1, ld, -1, 0, H, H, A, w3, b3, L.Ls, kA, nullptr, 0, GYMRL_ACT_CLAMP, a.log_std_min, a.log_std_max)};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  STEP_MARK(2, 4);
  // one lane per env: draw, Pendulum step with auto-reset, replay row (the first wave: 16 lanes busy)
  if (t < 64) {
    float act[kMaxA], lp;
    if (t < nrows) sample_row(lds + L.Mean + t * kMaxA, lds + L.Ls + t * kMaxA, lds + L.Eps + t * kMaxA, A, a.bound, act, lp);
    pendulum_act_tail(a, lds, L, t, row0, nrows, act);
  }
  STEP_MARK(2, 5);
}

template <int HC>
__global__ __launch_bounds__(kThreads) void sac_act_kernel(const gymrl_sac_act_args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  sac_act_body<HC>(a, lds, blockIdx.x);
}

}  // namespace

extern "C" {

size_t gymrl_sac_update_workspace_bytes(int B, int D, int A, int H) { return workspace_bytes<SacWs>(B, D, A, H); }

#ifdef GYMRL_PROF_BUILD
int gymrl_step_prof_read(long long* out_host) {      // probe build only: [4][32] stamps of the last launches (workgroup 0)
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_step_prof), sizeof(long long) * 128) == hipSuccess ? 0 : -1;
}
#endif

size_t gymrl_sac_args_bytes(int which) { return which == 0 ? sizeof(gymrl_sac_act_args) : which == 1 ? sizeof(gymrl_sac_update_args) : 0; }

int gymrl_sac_act_step(const gymrl_sac_act_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_sac_act_args& a = *args;
  if (!act_args_ok(a, GYMRL_ENV_PENDULUM, /*refuse_neg_cursor=*/false) || !net_ok(a.actor)) return -22;
  static bool done = false;
  if (const int rc = set_max_lds_once(done, {(const void*)sac_act_kernel<0>, (const void*)sac_act_kernel<256>}, (int)lds_bytes(256, 4))) return rc;
  hipLaunchKernelGGL(a.H == 256 ? sac_act_kernel<256> : sac_act_kernel<0>, dim3((a.N + 15) / 16), dim3(kThreads), lds_bytes(a.H, 4), (hipStream_t)stream_, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_sac_pack_images(const gymrl_sac_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_sac_update_args& a = *args;
  if (!pack_args_ok(a) || !all_set({a.actor.w[1], a.critic.w[1], a.critic.w[4], a.target.w[1], a.target.w[4]})) return -22;
  hipLaunchKernelGGL(pack_images_kernel, dim3((a.H * a.H + 255) / 256, Images::kCount), dim3(256), 0, (hipStream_t)stream_, Images::sources(a), a.images, a.H);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

static bool sac_update_args_ok(const gymrl_sac_update_args& a) {
  if (!slab_shape_ok(a.B, kMaxBatch, a.D, a.A, a.H)) return false;
  if (!ring_ok(a) || !all_set({a.workspace, a.sums, a.log_alpha, a.alpha_m, a.alpha_v, a.actor_p, a.actor_m, a.actor_v, a.critic_p, a.critic_m, a.critic_v}) ||
      !draw_ok(a, /*idx_dev_counts=*/false))      // (this check has never counted the device's draw record)
    return false;
  return net_ok(a.actor) && net_ok(a.critic) && net_ok(a.target);
}

static int sac_set_lds_attr() {
  static bool done = false;
  return set_max_lds_once(done, {(const void*)sac_p1_kernel<0>, (const void*)sac_p1_kernel<256>, (const void*)sac_p3_kernel<0>, (const void*)sac_p3_kernel<256>},
                          (int)lds_bytes(256, 8));
}

// The tile lists of P2 (critic: c) and P4 (actor + temperature: p)
static void sac_build_dw(const gymrl_sac_update_args& a, const SacWs& ws, DwArgs& c, DwArgs& p) {
  const int B = a.B, D = a.D, A = a.A, H = a.H;
  const Images im(a.images, H);
  const float *cf[2] = {im.c1f, im.c2f}, *cbk[2] = {im.c1b, im.c2b}, *tf[2] = {im.t1f, im.t2f};      // network i's images
  // critic: launch order of the layer-by-layer backward is irrelevant here (tiles are independent); fc1/fc4, fc2/fc5, fc3/fc6
  c = DwArgs{};
  DwBuilder cb{c, B};
  for (int i = 0; i < 2; ++i) {
    cb.seg(ws.Z1[i], H, H, ws.s, D, ws.a, A, D + A, D, a.critic.w[3 * i], a.critic.b[3 * i], a.target.w[3 * i], a.target.b[3 * i]);
    cb.seg(ws.Z2[i], H, H, ws.H1[i], H, nullptr, 0, H, H, a.critic.w[3 * i + 1], a.critic.b[3 * i + 1], a.target.w[3 * i + 1], a.target.b[3 * i + 1],
        cf[i], cbk[i], tf[i]);
    cb.seg(ws.dq[i], 1, 1, ws.H2[i], H, nullptr, 0, H, H, a.critic.w[3 * i + 2], a.critic.b[3 * i + 2], a.target.w[3 * i + 2], a.target.b[3 * i + 2]);
  }
  cb.close(a, ws.dw_parts, a.critic_p, a.critic_m, a.critic_v, a.adam_critic, a.adam_critic_dev, (float)a.tau, (float)(1.0 - a.tau), ws.terms, ws.terms2, 0, 1, a.sums);

  p = DwArgs{};
  DwBuilder pb{p, B};
  pb.seg(ws.aZ1, H, H, ws.s, D, nullptr, 0, D, D, a.actor.w[0], a.actor.b[0]);
  pb.seg(ws.aZ2, H, H, ws.aH1, H, nullptr, 0, H, H, a.actor.w[1], a.actor.b[1], nullptr, nullptr, im.af, im.ab);
  pb.seg(ws.dmean, A, A, ws.aH2, H, nullptr, 0, H, H, a.actor.w[2], a.actor.b[2]);
  pb.seg(ws.dls, A, A, ws.aH2, H, nullptr, 0, H, H, a.actor.w[3], a.actor.b[3]);
  pb.close(a, ws.dw_parts, a.actor_p, a.actor_m, a.actor_v, a.adam_actor, a.adam_actor_dev, 0.0f, 0.0f, ws.terms, nullptr, 1, 2, a.sums);
  p.alpha_step = 1;
  p.log_alpha = a.log_alpha; p.alpha_m = a.alpha_m; p.alpha_v = a.alpha_v; p.lr_alpha = a.lr_alpha;
  p.abeta1 = 0.9; p.abeta2 = 0.999; p.aeps = 1e-8;
  p.alpha_bias[0] = a.alpha_bias[0]; p.alpha_bias[1] = a.alpha_bias[1]; p.alpha_bias_dev = a.alpha_bias_dev; p.alpha_loss = a.alpha_loss;
}

int gymrl_sac_update(const gymrl_sac_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_sac_update_args& a = *args;
  if (!sac_update_args_ok(a)) return -22;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = sac_set_lds_attr()) return rc;
  SacWs ws;
  SacWs::carve(&ws, align256(a.workspace), a.B, a.D, a.A, a.H);
  const int H = a.H, slabs = (a.B + 15) / 16;
  DwArgs c, p;
  sac_build_dw(a, ws, c, p);
  // (the instances built for the reference's hidden width 256 know every reduction length at compile time)
  hipLaunchKernelGGL(H == 256 ? sac_p1_kernel<256> : sac_p1_kernel<0>, slab_launch_grid(slabs, 4), dim3(kThreads), lds_bytes(H, 8), stream, a, ws);   // y / role: the two target chains, the two critic chains
  launch_dw(c, stream);
  hipLaunchKernelGGL(H == 256 ? sac_p3_kernel<256> : sac_p3_kernel<0>, slab_launch_grid(slabs, 2), dim3(kThreads), lds_bytes(H, 8), stream, a, ws);   // y / role: the actor + Q2, then Q1
  launch_dw(p, stream);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
