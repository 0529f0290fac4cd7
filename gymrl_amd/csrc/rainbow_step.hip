// rainbow_step.hip — Rainbow's CartPole vector step (rainbow_dqn_cartpole.py:363-405) on the row-slab stages of
// slab_step_device.hpp, as offpolicy_step.hip runs SAC's:
//
//   rainbow_act_kernel   N/16 (N/32) workgroups: greedy action on the noisy Q, CartPole step, the n-step window, replay row
//   rainbow_rows_kernel  three workgroups per 16-row slab: policy(s), policy(s'), target(s'); double-DQN target, IS-weighted
//                        loss gradient, the input-gradient chain
//   sac_dw_kernel        one wave per 16 x 16 weight tile: the gradients, stored (clip_grad_norm_ needs them all before Adam
//                        may run; the stacked noisy head's is split into mu / sigma here)
//
// Bit for bit the layer-by-layer path's results (tests/test_fused_step_gpu.py).
#include "duel_device.hpp"
#include "slab_step_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::slab;

struct RbWs {
  float *s, *h1, *h2, *dS, *dZ2, *dZ1;      // [B][D], [B][H], [B][H], [B][A+1], [B][H], [B][H]
  double* terms;                             // [B][3] (column 0: w * td^2)
  float* xz;                                 // [2][16 S][4]: head outputs of policy(s') and target(s') on their way to the policy(s) workgroup
  unsigned int* flag;                        // [2][S]: their hand-off flags (zero before the first launch, left zero)
  unsigned int* tk;                          // [2]: slab_grid's next ticket / finished count of the large-batch row kernel (zero between launches)
  float* dw_parts;                           // B > 512: the weight-gradient tiles' slice partials (DwArgs)
  __host__ __device__ static size_t carve(RbWs* w, void* base, int B, int D, int A, int H) {
    carve_taker take{base};
    float* s_ = take((size_t)B * D); float* h1 = take((size_t)B * H); float* h2 = take((size_t)B * H); float* dS = take((size_t)B * (A + 1));
    float* z2 = take((size_t)B * H); float* z1 = take((size_t)B * H);
    double* terms = reinterpret_cast<double*>(take((size_t)B * 6));
    const size_t S16 = (size_t)(B + 15) / 16 * 16;
    float* xz = take(2 * S16 * 4);
    unsigned int* fl = reinterpret_cast<unsigned int*>(take(2 * S16 / 16));
    unsigned int* tk = reinterpret_cast<unsigned int*>(take(2));
    const size_t dw_tiles = B > 512 ? (size_t)((A + 1 + 15) / 16) * ((H + 15) / 16) + (size_t)((H + 15) / 16) * ((H + 15) / 16) + (size_t)((H + 15) / 16) * ((D + 15) / 16) : 0;
    float* dwp = take(dw_tiles * kDwMaxSlices * 320);
    if (w) { w->s = s_; w->h1 = h1; w->h2 = h2; w->dS = dS; w->dZ2 = z2; w->dZ1 = z1; w->terms = terms; w->xz = xz; w->flag = fl;
             w->tk = tk; w->dw_parts = dwp; }
    return take.off;
  }
};

// (the dueling combination of one row, dueling_row: duel_device.hpp)
constexpr int kRbMaxA = 3;

// Three workgroups per 16-row slab (blockIdx.y): policy(s) — the pass the gradient flows through —, policy(s') and target(s')
// are independent chains until the double-DQN target meets the TD error (:320-334), and a slab's stage costs what ONE compute
// unit's f32 MFMA rate makes of its items (three 256 x 256 layers per stage on one CU before).  Workgroups 1 and 2 publish
// their head outputs ([16][4]) with release flags; workgroup 0, whose own forward takes as long, consumes them, clears the
// flags and runs the loss and the way back.  The producers wait for nobody and come first in the launch (slab_grid: y / slot
// 0, 1 -> passes 1, 2; the waiting pass 0 last), so the pass that waits always finds its producers started.
template <int HC>                       // HC: the hidden width this instance is built for (0: any), as the SAC kernels'
__device__ __forceinline__ void rainbow_rows_body(const gymrl_rainbow_update_args& a, const RbWs& ws, float* lds, const SlabGrid& sg_) {
  const Lds L;
  const int D = a.D, A = a.A, A1 = a.A + 1, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int H1 = L.big, H2 = H1 + 16 * ld, X0 = H2 + 16 * ld;
  // head outputs of the three passes: [16][4] slabs in the small area (Q0, Q1, Cq0), dS in Dq0
  const int Za = L.Q0, Zb = L.Q1, Zc = L.Cq0, DS = L.Dq0;
  const int bx = sg_.slab;
  const int row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const int pass = sg_.role;            // 0: policy(s) [second draw], 1: policy(s') [first draw], 2: target(s') [means]
  const int S = sg_.slabs;
  if (t < 16) {                         // gather (replay.hip replay_gather_kernel): what this workgroup's pass reads
    const int b = row0 + t;
    const bool ok = t < nrows;
    const int64_t row = ok ? a.idx[b] : 0;
    const float* src = pass == 0 ? a.r_state : a.r_next;
    for (int k = 0; k < kMaxD; ++k) {
      const float sv = (ok && k < D) ? src[row * D + k] : 0.0f;
      lds[L.S + t * kMaxD + k] = sv;
      if (pass == 0 && ok && k < D) ws.s[(size_t)b * D + k] = sv;
    }
    if (pass == 0) {
      lds[L.Misc + t * 4 + 0] = ok ? a.r_reward[row] : 0.0f;
      lds[L.Misc + t * 4 + 1] = ok ? (float)a.r_flag[row] : 0.0f;
      lds[L.Misc + t * 4 + 2] = ok ? __int_as_float((int)a.r_action[row]) : 0.0f;
      lds[L.Misc + t * 4 + 3] = (ok && a.is_weight) ? a.is_weight[b] : 1.0f;
    }
  }
  __syncthreads();
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD;
  const size_t hw = (size_t)A1 * H;
  const bool tgt = pass == 2;
  const int hslot = pass == 0 ? 2 : (pass == 1 ? 0 : 1);            // the stacked heads: first draw | target means | second draw
  const int Zme = pass == 0 ? Zc : (pass == 1 ? Za : Zb);
  fwd_one(lds, {fwd_item(L.S, kD, -1, 0, D, D, H, tgt ? a.t_fc1_w : a.p_fc1_w, tgt ? a.t_fc1_b : a.p_fc1_b, H1, ld, pass == 0 ? ws.h1 : nullptr, H, R)}, row0, nrows);
  fwd_one(lds, {fwd_item(H1, ld, -1, 0, H, H, H, tgt ? a.t_fc2_w : a.p_fc2_w, tgt ? a.t_fc2_b : a.p_fc2_b, H2, ld, pass == 0 ? ws.h2 : nullptr, H, R,
          0.0f, 0.0f, tgt ? a.t_fc2_img_f : a.p_fc2_img_f)}, row0, nrows);
  fwd_one(lds, {fwd_item(H2, ld, -1, 0, H, H, A1, a.head_w + hslot * hw, a.head_b + hslot * A1, Zme, 4, nullptr, 0, NA)}, row0, nrows);
  if (pass != 0) {                      // the head outputs go to workgroup 0
    float* xz = ws.xz + ((size_t)(pass - 1) * S * 16 + row0) * 4;
    if (t < 64) xstore(xz + t, lds[Zme + t]);
    __syncthreads();
    if (t == 0) flag_post(ws.flag + (pass - 1) * S + bx);
    return;
  }
  if (t == 0) { flag_wait(ws.flag + bx); flag_wait(ws.flag + S + bx); }
  __syncthreads();
  if (t < 64) {
    lds[Za + t] = xload(ws.xz + ((size_t)row0) * 4 + t);
    lds[Zb + t] = xload(ws.xz + ((size_t)S * 16 + row0) * 4 + t);
  }
  __syncthreads();
  if (t == 0) { flag_clear(ws.flag + bx); flag_clear(ws.flag + S + bx); }
  if (t < 16) {
    // dueling heads, the double-DQN target and the IS-weighted loss gradient (offpolicy.hip dqn_td_kernel), dueling backward (lin.hip)
    float q_no[kRbMaxA], q_nt[kRbMaxA], q[kRbMaxA];
    const int astar = dueling_row(lds + Za + t * 4, A, q_no);
    dueling_row(lds + Zb + t * 4, A, q_nt);
    dueling_row(lds + Zc + t * 4, A, q);
    const float invB = 1.0f / (float)a.B;
    const float nq = q_nt[astar];
    const float y = lds[L.Misc + t * 4 + 0] + a.gamma_n * nq * (1.0f - lds[L.Misc + t * 4 + 1]);
    const int act = __float_as_int(lds[L.Misc + t * 4 + 2]);
    const float td = q[act] - y;
    const float wb = lds[L.Misc + t * 4 + 3];
    float dq[kRbMaxA], sum = 0.0f;
    for (int k = 0; k < A; ++k) { dq[k] = (k == act) ? (2.0f * td) * wb * invB : 0.0f; sum += dq[k]; }
    const float m = sum / (float)A;
    for (int k = 0; k < 4; ++k) {
      const float v = k < A ? dq[k] - m : (k == A ? sum : 0.0f);
      lds[DS + t * 4 + k] = v;
      if (t < nrows && k < A1) ws.dS[(size_t)(row0 + t) * A1 + k] = v;
    }
    if (t < nrows) {
      a.td_out[row0 + t] = td;
      ws.terms[(size_t)(row0 + t) * 3 + 0] = (double)((td * td) * wb);
    }
  }
  __syncthreads();
  // loss.backward() of this pass: head -> fc2 (the input gradients; the weight gradients are the tile launch's)
  bwd_one(lds, {BwdItem{DS, 4, A1, a.head_w + 2 * hw, H, -1, nullptr, H2, ld, R, X0, ld, ws.dZ2, H, nullptr}}, row0, nrows);
  bwd_stage(lds, {BwdItem{X0, ld, H, a.p_fc2_w, H, -1, nullptr, H1, ld, R, -1, 0, ws.dZ1, H, a.p_fc2_img_b}}, row0, nrows);      // (the last stage: no barrier behind it)
}

template <int HC>
__global__ __launch_bounds__(kThreads) void rainbow_rows_kernel(const gymrl_rainbow_update_args a, const RbWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int order[3] = {1, 2, 0};                    // policy(s') and target(s') first: pass 0 waits for them
  const SlabGrid g = slab_grid<3>(ws.tk, order);
  rainbow_rows_body<HC>(a, ws, lds, g);
  slab_grid_done(g);
}

// Greedy acting on the noisy Q + CartPole + the n-step window: one lane per env after the network.  NS slabs of 16 envs per
// workgroup: at N = 8192 the 16-row form is 512 workgroups = two rounds over the 256 compute units, each streaming every
// weight again (45 us per launch); 32 rows per workgroup stream them once for two MFMA chains.
template <int NS>
__device__ __forceinline__ void act_layer(float* lds, int X, int ldx, int K, const float* W, const float* b, int N, int Ys, int ldy, int act,
                                          const float* Wimg = nullptr) {       // Wimg: forward image of a square W (K == N, % 16)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  const int ntiles = (N + 15) >> 4;
  for (int t = wave; t < ntiles; t += kWaves) {
    const int nb = t * 16;
    f32x4 acc[2];
    if (Wimg) {
      if (NS == 2) lin::tile_fwd_img_x2_t<0>(lds + X, lds + X + 16 * ldx, ldx, K >> 4, Wimg, t, lane, acc[0], acc[1]);
      else acc[0] = lin::tile_fwd_img(lds + X, ldx, K >> 4, Wimg, t, lane);
    } else if (NS == 2) lin::tile_fwd_x2(lds + X, lds + X + 16 * ldx, ldx, K, W, N, nb, lane, acc[0], acc[1]);
    else acc[0] = lin::tile_fwd(lds + X, ldx, nullptr, 0, K, K, W, N, nb, lane);
    const int n = nb + r;
    if (n < N) {
      const float bv = b ? b[n] : 0.0f;
#pragma unroll
      for (int sl = 0; sl < NS; ++sl)
#pragma unroll
        for (int g = 0; g < 4; ++g) lds[Ys + (16 * sl + 4 * q + g) * ldy + n] = act_fwd(acc[sl][g] + bv, act, 0.0f, 0.0f);
    }
  }
}

template <int NS, int HC>
__global__ __launch_bounds__(kThreads) void rainbow_act_kernel(const gymrl_rainbow_act_args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int kRows = 16 * NS;
  const int D = a.D, A = a.A, A1 = a.A + 1, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int S = 0, Q = S + kRows * kMaxD, X0 = Q + kRows * 4, X1 = X0 + kRows * ld;
  const int row0 = blockIdx.x * kRows, nrows = min(kRows, a.N - row0);
  const int t = threadIdx.x;
  if (t < kRows) {
    const int i = row0 + t;
    for (int k = 0; k < kMaxD; ++k) lds[S + t * kMaxD + k] = (t < nrows && k < D) ? a.obs[(size_t)i * D + k] : 0.0f;
  }
  __syncthreads();
  act_layer<NS>(lds, S, kMaxD, D, a.fc1_w, a.fc1_b, H, X0, ld, GYMRL_ACT_RELU);
  __syncthreads();
  act_layer<NS>(lds, X0, ld, H, a.fc2_w, a.fc2_b, H, X1, ld, GYMRL_ACT_RELU, a.fc2_img);
  __syncthreads();
  act_layer<NS>(lds, X1, ld, H, a.head_w, a.head_b, A1, Q, 4, GYMRL_ACT_NONE);
  __syncthreads();
  if (t < 64) {
    const bool ok = t < nrows;
    ClassicStep<4> r;
    r.done = false; r.ret = 0.0; r.len = 0;
    if (ok) {
      const int e = row0 + t;
      float q[kRbMaxA];
      const int act = dueling_row(lds + Q + t * 4, A, q);
      const CartPoleState st(a.env_state, a.N);
      cartpole_step_one(st, e, a.env_seed, a.env_id0, act, r);
      for (int k = 0; k < D; ++k) a.obs_out[(size_t)e * D + k] = r.o_next[k];
      if (a.action_out) a.action_out[e] = act;
      if (a.rew_out) a.rew_out[e] = r.reward;
      if (a.done_out) a.done_out[e] = r.done;
      if (r.done && a.ep_ret_out) a.ep_ret_out[e] = (float)r.ret;
      // ---- replay.hip nstep_push_kernel for env e (deque.append :186-187, _get_n_step_transition :207-218) ----
      const int N = a.N, n_steps = a.n_steps;
      int64_t pushes = a.pushes, cursor = a.cursor;
      if (a.push_dev) { pushes = a.push_dev[0]; cursor = a.push_dev[1]; }
      const int slot = (int)(pushes % n_steps);
      const bool emit = pushes + 1 >= n_steps;
      const size_t so = (size_t)slot * N + e;
      for (int k = 0; k < D; ++k) {
        a.w_state[so * D + k] = lds[S + t * kMaxD + k];
        a.w_next[so * D + k] = r.o_term[k];
      }
      a.w_action[so] = act; a.w_reward[so] = r.reward;
      // :376 terminal = done and step != max_steps_per_episode - 1, by the step INDEX inside the episode
      const uint8_t term_now = (uint8_t)((r.done && r.len != a.max_episode_steps) ? 1 : 0);
      a.w_terminal[so] = term_now;
      a.w_done[so] = r.done;
      if (emit) {
        const int oldest = (slot + 1) % n_steps;
        int src = slot;
        double Rr = 0.0;
        for (int i = n_steps - 1; i >= 0; --i) {
          const int sidx = (oldest + i) % n_steps;
          const size_t o = (size_t)sidx * N + e;
          // this push's own slot comes from the registers that have just been stored (same lane)
          const bool dn = sidx == slot ? r.done : (a.w_done[o] != 0);
          const float rw = sidx == slot ? r.reward : a.w_reward[o];
          const double d = dn ? 1.0 : 0.0;
          Rr = (double)rw + a.gamma * (1.0 - d) * Rr;
          if (dn) src = sidx;
        }
        const int64_t row = (cursor + e) % a.cap;
        const size_t oo = (size_t)oldest * N + e, ss = (size_t)src * N + e;
        for (int k = 0; k < D; ++k) {
          a.r_state[row * D + k] = oldest == slot ? lds[S + t * kMaxD + k] : a.w_state[oo * D + k];
          a.r_next[row * D + k] = src == slot ? r.o_term[k] : a.w_next[ss * D + k];
        }
        a.r_action[row] = (uint32_t)(oldest == slot ? act : a.w_action[oo]);
        a.r_reward[row] = (float)Rr;
        a.r_flag[row] = src == slot ? term_now : a.w_terminal[ss];
      }
    }
    accumulate_ep_stats(a.ep_stats, r.done && ok, r.ret, r.len);
  }
}

inline bool rb_shape_ok(int B, int D, int A, int H) {
  return B > 0 && B <= kMaxBatch && D > 0 && D <= kMaxD && A > 0 && A <= kRbMaxA && H >= 4 && H <= 256 && (H & 3) == 0;
}

}  // namespace

extern "C" {

size_t gymrl_rainbow_update_workspace_bytes(int B, int D, int A, int H) { return workspace_bytes<RbWs>(B, D, A, H); }
size_t gymrl_rainbow_args_bytes(int which) { return which == 0 ? sizeof(gymrl_rainbow_act_args) : which == 1 ? sizeof(gymrl_rainbow_update_args) : 0; }

int gymrl_rainbow_act_step(const gymrl_rainbow_act_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_rainbow_act_args& a = *args;
  if (a.N <= 0 || !rb_shape_ok(1, a.D, a.A, a.H) || a.env_kind != GYMRL_ENV_CARTPOLE || a.D != 4 || a.A != 2) return -22;
  if (!a.env_state || !a.obs || !a.obs_out || !a.fc1_w || !a.fc1_b || !a.fc2_w || !a.fc2_b || !a.head_w || !a.head_b) return -22;
  if (!a.w_state || !a.w_action || !a.w_reward || !a.w_next || !a.w_terminal || !a.w_done || a.n_steps <= 0 || a.pushes < 0 ||
      !a.r_state || !a.r_action || !a.r_reward || !a.r_next || !a.r_flag || a.cap < a.N || a.cursor < 0)
    return -22;
  if (a.fc2_img && (a.H & 15) != 0) return -22;
  auto act_lds = [](int H, int ns) { return sizeof(float) * (size_t)(16 * ns * (kMaxD + 4 + 2 * lin::slab_ld(H))); };
  static bool done1 = false, done2 = false;
  if (const int rc = set_max_lds_once(done1, {(const void*)rainbow_act_kernel<1, 0>, (const void*)rainbow_act_kernel<1, 256>}, (int)act_lds(256, 1))) return rc;
  if (const int rc = set_max_lds_once(done2, {(const void*)rainbow_act_kernel<2, 0>, (const void*)rainbow_act_kernel<2, 256>}, (int)act_lds(256, 2))) return rc;
  using ActK = void (*)(const gymrl_rainbow_act_args);
  const ActK k1 = rainbow_act_kernel<1, 0>, k2 = rainbow_act_kernel<2, 0>, k1w = rainbow_act_kernel<1, 256>, k2w = rainbow_act_kernel<2, 256>;
  const bool wide = a.H == 256;      // the instances built for the reference's hidden width
  // more envs than one round of 16-row workgroups over the 256 compute units: 32 rows per workgroup (weights streamed once)
  if (a.N > 16 * 256 && (a.D & 3) == 0 && (a.H & 3) == 0)
    hipLaunchKernelGGL(wide ? k2w : k2, dim3((a.N + 31) / 32), dim3(kThreads), act_lds(a.H, 2), (hipStream_t)stream_, a);
  else
    hipLaunchKernelGGL(wide ? k1w : k1, dim3((a.N + 15) / 16), dim3(kThreads), act_lds(a.H, 1), (hipStream_t)stream_, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_rainbow_update(const gymrl_rainbow_update_args* args, int phase, void* stream_) {
  if (!args || phase < 0 || phase > 2) return -22;
  const gymrl_rainbow_update_args& a = *args;
  if (!rb_shape_ok(a.B, a.D, a.A, a.H)) return -22;
  if (!a.r_state || !a.r_action || !a.r_reward || !a.r_next || !a.r_flag || !a.idx || !a.p_fc1_w || !a.p_fc1_b || !a.p_fc2_w || !a.p_fc2_b ||
      !a.t_fc1_w || !a.t_fc1_b || !a.t_fc2_w || !a.t_fc2_b || !a.head_w || !a.head_b || !a.td_out || !a.loss_sum || !a.d_fc1_w || !a.d_fc1_b ||
      !a.d_fc2_w || !a.d_fc2_b || (!a.split_heads && (!a.d_head_w || !a.d_head_b)) || !a.workspace)
    return -22;
  if ((a.p_fc2_img_f || a.p_fc2_img_b || a.t_fc2_img_f) && (a.H & 15) != 0) return -22;
  hipStream_t stream = (hipStream_t)stream_;
  static bool done = false;
  if (const int rc = set_max_lds_once(done, {(const void*)rainbow_rows_kernel<0>, (const void*)rainbow_rows_kernel<256>}, (int)lds_bytes(256, 7))) return rc;
  RbWs ws;
  RbWs::carve(&ws, align256(a.workspace), a.B, a.D, a.A, a.H);
  const int B = a.B, D = a.D, A1 = a.A + 1, H = a.H;
  if (phase != 2) hipLaunchKernelGGL(H == 256 ? rainbow_rows_kernel<256> : rainbow_rows_kernel<0>, slab_launch_grid((B + 15) / 16, 3), dim3(kThreads), lds_bytes(H, 7), stream, a, ws);
  if (phase == 1) { GYMRL_CHECK_LAUNCH(); return 0; }
  DwArgs d{};
  DwBuilder bd{d, B};
  bd.seg(ws.dS, A1, A1, ws.h2, H, nullptr, 0, H, H, a.d_head_w, a.d_head_b);       // the stacked noisy heads (gymrl_noisy_split takes it from here)
  bd.seg(ws.dZ2, H, H, ws.h1, H, nullptr, 0, H, H, a.d_fc2_w, a.d_fc2_b);
  bd.seg(ws.dZ1, H, H, ws.s, D, nullptr, 0, D, D, a.d_fc1_w, a.d_fc1_b);
  bd.finish(ws.dw_parts);
  d.store_grads = 1;
  d.split_heads = a.split_heads ? 1 : 0; d.split_A = a.A;
  for (int l = 0; l < 2; ++l) {
    d.dw_mu[l] = a.dw_mu[l]; d.dw_sigma[l] = a.dw_sigma[l]; d.db_mu[l] = a.db_mu[l]; d.db_sigma[l] = a.db_sigma[l];
    d.w_eps[l] = a.w_eps[l]; d.b_eps[l] = a.b_eps[l];
    if (a.split_heads && (!a.dw_mu[l] || !a.dw_sigma[l] || !a.db_mu[l] || !a.db_sigma[l] || !a.w_eps[l] || !a.b_eps[l])) return -22;
  }
  d.terms = ws.terms; d.term0 = 0; d.nterms = 1; d.sums = a.loss_sum; d.alpha_step = 0;
  launch_dw(d, stream);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
