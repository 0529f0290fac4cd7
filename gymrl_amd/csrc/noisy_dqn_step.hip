// noisy_dqn_step.hip — NoisyNet dueling DQN's CartPole vector step (noisy_dqn_cartpole.py: select_action :198-212, update
// :214-257) on the row-slab stages of slab_step_device.hpp, in ddqn_step.hip's scheme.  All four layers of the network are
// NoisyLinear (fc1 D -> H, fc2 H -> H, value_stream H -> 1, advantage_stream H -> A), so a step first forms EFFECTIVE
// parameters W = mu + sigma * (eps_out (x) eps_in), b = mu + sigma * eps_out, and every later launch reads those:
//
//   ndqn_combine_kernel  elementwise: the effective parameters of all four layers for the step's three draws — set C (acting),
//                        set A (policy(s): the gradient flows through it), set B (policy(s'): the double-Q choice) — into the
//                        workspace; set A's eps vectors are kept for the backward                                (parameters)
//   ndqn_act_kernel      N/16 workgroups: forward on set C, dueling combine, argmax (first maximum), CartPole step with
//                        auto-reset, replay row: dqn_act_kernel without the epsilon draw                              (acting)
//   ndqn_r1_kernel       B/16 workgroups: draw + gather, policy(s) on set A | policy(s') on set B | target(s') on the target's
//                        mu, three dueling combines, the double-Q target, td, dq = 2 td / B, the row's td^2, the combine's
//                        backward, set A's dX chain back to fc1                                                         (rows)
//   sac_dw_kernel        dW / db of set A's effective parameters (store_grads: nothing is stepped here), the loss sum  (tiles)
//   ndqn_adam_kernel     elementwise: d mu = dW, d sigma = dW * eps_A (biases: db * eps_out), Adam on mu and sigma   (optimiser)
//
// The split + Adam is a launch of its own and not the tile kernel's epilogue: sac_dw_kernel's store-grads hook splits ONE
// stacked segment with materialised [N][K] eps arrays and stores the halves (Rainbow clips the gradient norm before Adam may
// run); carrying four layers' eps vectors and two parameters per tile element through DwArgs would grow the argument block
// and the epilogue of a kernel every off-policy step shares.  ONE workgroup carries a slab through the whole row phase, so
// nothing here waits for another workgroup: no flag, no counter; launch order on one stream is the only ordering.
//
// LDS per workgroup of ndqn_r1_kernel: the small per-row slabs (kSmallFloats floats = 4,096 B) + six [16][slab_ld(H)] activation
// slabs — P1, N1, T1 (fc1 of the three chains) and P2, N2, T2 (fc2).  N2 and T2 are dead once their heads are out and take the
// two heads' input gradients; T1 is dead after fc2 and carries dL/dz2.  At H = 64 (slab_ld = 68): 6 * 16 * 68 * 4 = 26,112 B +
// 4,096 B = 30,208 B; at H = 256: 103,936 B (one workgroup per compute unit; the grid is at most 16 workgroups).
// ndqn_act_kernel: two slabs, 12,800 B at H = 64.  fc2 is read from the combine's workspace: no weight images here.
#include "value_step_device.hpp"

namespace {

using namespace gymrl;
using namespace gymrl::slab;

constexpr int kNdqnMaxBatch = 256;     // (ops.NDQN_FUSED_MAX_BATCH) one grid of at most 16 slabs in the row phase: the loss sum is one block's
constexpr int kNdqnSlabs = 6;
constexpr int kLayers = 4;             // fc1, fc2, value_stream, advantage_stream

__host__ __device__ __forceinline__ void ndqn_dims(int l, int D, int A, int H, int& N, int& K) {
  N = l < 2 ? H : l == 2 ? 1 : A;
  K = l == 0 ? D : H;
}
// elements (weights + biases) of one effective parameter set
__host__ __device__ __forceinline__ int ndqn_count(int D, int A, int H) { return H * (D + 1) + H * (H + 1) + (H + 1) + A * (H + 1); }
// first element of layer l's input-side vector in a raw-draw row: per layer the K input-side draws, then the N output-side ones
__host__ __device__ __forceinline__ int ndqn_raw_off(int l, int D, int A, int H) {
  return l == 0 ? 0 : l == 1 ? D + H : l == 2 ? D + 3 * H : D + 4 * H + 1;
}

// The workspace: what the combine launch leaves for the act and row launches, and the hand-off between rows, tiles and Adam
struct NdqnWs {
  float* w[3][kLayers]; float* b[3][kLayers];      // effective parameters of set 0 = C (acting), 1 = A, 2 = B
  float* eps_in[kLayers]; float* eps_out[kLayers]; // set A's f(raw) vectors
  float* gw[kLayers]; float* gb[kLayers];          // dL/dW, dL/db of set A's effective parameters
  float* s;                                        // [B][D]: the gathered states
  float *H1, *Z1, *H2, *Z2, *dv, *da;              // set A's activations and dL/dz ([B][H]; dv [B], da [B][A])
  double* terms;                                   // [B][3]: the row's td^2 in column 0 (sac_dw_body's row pitch)
  __host__ __device__ static size_t carve(NdqnWs* w, void* base, int B, int D, int A, int H) {
    carve_taker take{base};
    NdqnWs o;
    for (int set = 0; set < 3; ++set)
      for (int l = 0; l < kLayers; ++l) {
        int N, K;
        ndqn_dims(l, D, A, H, N, K);
        o.w[set][l] = take((size_t)N * K); o.b[set][l] = take(N);
      }
    for (int l = 0; l < kLayers; ++l) {
      int N, K;
      ndqn_dims(l, D, A, H, N, K);
      o.eps_in[l] = take(K); o.eps_out[l] = take(N);
      o.gw[l] = take((size_t)N * K); o.gb[l] = take(N);
    }
    o.s = take((size_t)B * D);
    o.H1 = take((size_t)B * H); o.Z1 = take((size_t)B * H); o.H2 = take((size_t)B * H); o.Z2 = take((size_t)B * H);
    o.dv = take(B); o.da = take((size_t)B * A);
    o.terms = reinterpret_cast<double*>(take((size_t)B * 6));
    if (w) *w = o;
    return take.off;
  }
};

// ---- the effective parameters of the step's three draws; NoisyLinear.reset_noise() of those forwards happens here ----
__global__ __launch_bounds__(256) void ndqn_combine_kernel(const gymrl_ndqn_combine_args a, const NdqnWs ws) {
  const int D = a.D, A = a.A, H = a.H;
  const int P = ndqn_count(D, A, H);
  for (int t = blockIdx.x * 256 + threadIdx.x; t < 3 * P; t += gridDim.x * 256) {
    const int set = t / P;
    int r = t - set * P, l = 0, N = 0, K = 0;
    for (;; ++l) {
      ndqn_dims(l, D, A, H, N, K);
      if (l == kLayers - 1 || r < N * (K + 1)) break;
      r -= N * (K + 1);
    }
    const int n = r / (K + 1), k = r - n * (K + 1);
    const float* raw = a.raw[set];
    const uint64_t ctr = a.counter_dev ? a.counter_dev[set] : a.counter[set];
    const int ro = ndqn_raw_off(l, D, A, H);
    // gymrl_noisy_noise's values: Box-Muller on Philox(seed, counter; stream 1 = output side, 0 = input side; element)
    const float fj = scale_noise(raw ? raw[ro + K + n] : box_muller(a.seed[l], ctr, 1u, (uint32_t)n));
    if (k < K) {
      const float fi = scale_noise(raw ? raw[ro + k] : box_muller(a.seed[l], ctr, 0u, (uint32_t)k));
      const float e = fj * fi;                                       // torch.outer(epsilon_j, epsilon_i)
      const size_t o = (size_t)n * K + k;
      ws.w[set][l][o] = a.policy.w_mu[l][o] + a.policy.w_sigma[l][o] * e;
      if (set == 1 && n == 0) ws.eps_in[l][k] = fi;
    } else {
      ws.b[set][l][n] = a.policy.b_mu[l][n] + a.policy.b_sigma[l][n] * fj;
      if (set == 1) ws.eps_out[l][n] = fj;
    }
  }
}

// ---- acting: the noisy Q of set C, the greedy choice (torch.argmax: the first maximum), CartPole step, replay row ----
__global__ __launch_bounds__(kThreads) void ndqn_act_kernel(const gymrl_ndqn_act_args a, const NdqnWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = a.H, ld = lin::slab_ld(H);
  const int X0 = L.big, X1 = X0 + 16 * ld;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.N - row0);
  const int t = threadIdx.x;
  act_load_obs(a, lds, L, t, row0, nrows);
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD;
  fwd_one(lds, {fwd_item(L.S, kD, -1, 0, D, D, H, ws.w[0][0], ws.b[0][0], X0, ld, nullptr, 0, R)}, row0, nrows);
  fwd_one(lds, {fwd_item(X0, ld, -1, 0, H, H, H, ws.w[0][1], ws.b[0][1], X1, ld, nullptr, 0, R)}, row0, nrows);
  {
    const FwdItem st[2] = {fwd_item(X1, ld, -1, 0, H, H, 1, ws.w[0][2], ws.b[0][2], L.Cq1, 4, nullptr, 0, NA),
                           fwd_item(X1, ld, -1, 0, H, H, A, ws.w[0][3], ws.b[0][3], L.Cq0, 4, nullptr, 0, NA)};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 64) {
    int act = 0;
    if (t < nrows) {
      float q[kMaxA];
      duel_combine(lds + L.Cq0 + t * 4, lds[L.Cq1 + t * 4], A, q);
      float best = q[0];
      for (int k = 1; k < A; ++k) if (q[k] > best) { best = q[k]; act = k; }
    }
    cartpole_act_tail(a, lds, L, t, row0, nrows, act);
  }
}

__global__ __launch_bounds__(kThreads) void ndqn_r1_kernel(const gymrl_ndqn_update_args a, const NdqnWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = a.H, ld = lin::slab_ld(H);
  const int P1 = L.big, N1 = P1 + 16 * ld, T1 = N1 + 16 * ld, P2 = T1 + 16 * ld, N2 = P2 + 16 * ld, T2 = N2 + 16 * ld;
  const int Z0 = T1;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const int R = GYMRL_ACT_RELU, kD = kMaxD;
  const gymrl_ndqn_params& tg = a.target;
  // ---- index draw + ring gather: one thread per row, rows beyond the batch or outside the ring are zero ----
  if (t < 16) {
    const int b = row0 + t;
    const int64_t row = checked_ring_row(t < nrows, [&] { return replay_draw_row(a, b); }, a.cap);
    gather_ring_row(a, lds, L, t, b, t < nrows, row, /*checked=*/true, ws.s, RowWeight::kUnit);
  }
  __syncthreads();
  // ---- policy_net(s) on set A, policy_net(s') on set B, target_net(s') on the target's mu: three chains, layer by layer ----
  {
    const FwdItem st[3] = {fwd_item(L.S, kD, -1, 0, D, D, H, ws.w[1][0], ws.b[1][0], P1, ld, ws.H1, H, R),
                           fwd_item(L.S2, kD, -1, 0, D, D, H, ws.w[2][0], ws.b[2][0], N1, ld, nullptr, 0, R),
                           fwd_item(L.S2, kD, -1, 0, D, D, H, tg.w_mu[0], tg.b_mu[0], T1, ld, nullptr, 0, R)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[3] = {fwd_item(P1, ld, -1, 0, H, H, H, ws.w[1][1], ws.b[1][1], P2, ld, ws.H2, H, R),
                           fwd_item(N1, ld, -1, 0, H, H, H, ws.w[2][1], ws.b[2][1], N2, ld, nullptr, 0, R),
                           fwd_item(T1, ld, -1, 0, H, H, H, tg.w_mu[1], tg.b_mu[1], T2, ld, nullptr, 0, R)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  // the heads, the loss (dqn_td_kernel with qn_online set and no weights: a live row weighs 1) and set A's input-gradient chain:
  // N2 and T2 take the two heads' input gradients, their sum under fc2's ReLU derivative goes to ws.Z2 and to Z0 for fc2's own dX
  const DuelHeads hp[3] = {{ws.w[1][2], ws.b[1][2], ws.w[1][3], ws.b[1][3]}, {ws.w[2][2], ws.b[2][2], ws.w[2][3], ws.b[2][3]},
                           {tg.w_mu[2], tg.b_mu[2], tg.w_mu[3], tg.b_mu[3]}};
  duel_heads_segment(lds, L, A, H, ld, row0, nrows, a.gamma, a.B, {P2, N2, T2}, hp, /*Xv=*/N2, /*Xa=*/T2, ws.dv, ws.da, /*td_out=*/nullptr,
                     ws.terms, /*Zs=*/Z0, ws.Z2);
  __syncthreads();
  bwd_stage(lds, {BwdItem{Z0, ld, H, ws.w[1][1], H, -1, nullptr, P1, ld, R, -1, 0, ws.Z1, H, nullptr}}, row0, nrows);      // (the last stage: no barrier behind it)
}

// ---- d mu = dW, d sigma = dW * eps_A per layer (biases: db * eps_out), Adam on both (optim.hip adam_one's arithmetic, no clamp) ----
struct NdqnAdamArgs {
  gymrl_ndqn_params p;
  int D, A, H;
  float* base; float* m; float* v;                 // the flat parameter buffer and its moments
  float adam[4]; const float* adam_dev;
  float omb1, beta2, omb2, eps;
};
__global__ __launch_bounds__(256) void ndqn_adam_kernel(const NdqnAdamArgs a, const NdqnWs ws) {
  const int D = a.D, A = a.A, H = a.H;
  const int P = ndqn_count(D, A, H);
  lin::AdamScalars ad;
  ad.step_size = a.adam_dev ? a.adam_dev[0] : a.adam[0];
  ad.bc2_sqrt = a.adam_dev ? a.adam_dev[2] : a.adam[2];
  ad.omb1 = a.omb1; ad.beta2 = a.beta2; ad.omb2 = a.omb2; ad.eps = a.eps;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < P; t += gridDim.x * 256) {
    int r = t, l = 0, N = 0, K = 0;
    for (;; ++l) {
      ndqn_dims(l, D, A, H, N, K);
      if (l == kLayers - 1 || r < N * (K + 1)) break;
      r -= N * (K + 1);
    }
    const int n = r / (K + 1), k = r - n * (K + 1);
    float g, e, *mu, *sigma;
    if (k < K) {
      const size_t o = (size_t)n * K + k;
      g = ws.gw[l][o]; e = ws.eps_out[l][n] * ws.eps_in[l][k];
      mu = a.p.w_mu[l] + o; sigma = a.p.w_sigma[l] + o;
    } else {
      g = ws.gb[l][n]; e = ws.eps_out[l][n];
      mu = a.p.b_mu[l] + n; sigma = a.p.b_sigma[l] + n;
    }
    const size_t om = (size_t)(mu - a.base), os = (size_t)(sigma - a.base);
    float Pm = *mu, Mm = a.m[om], Vm = a.v[om];
    lin::adam_elem(Pm, g, Mm, Vm, ad);
    *mu = Pm; a.m[om] = Mm; a.v[om] = Vm;
    float Ps = *sigma, Ms = a.m[os], Vs = a.v[os];
    lin::adam_elem(Ps, g * e, Ms, Vs, ad);
    *sigma = Ps; a.m[os] = Ms; a.v[os] = Vs;
  }
}

bool ndqn_shape_ok(int B, int D, int A, int H) { return slab_shape_ok(B, kNdqnMaxBatch, D, A, H) && A == 2; }     // duel_combine's order is pinned for two actions
bool ndqn_net_ok(const gymrl_ndqn_params& n, bool sigma) {
  for (int l = 0; l < kLayers; ++l)
    if (!n.w_mu[l] || !n.b_mu[l] || (sigma && (!n.w_sigma[l] || !n.b_sigma[l]))) return false;
  return true;
}

}  // namespace

extern "C" {

size_t gymrl_ndqn_update_workspace_bytes(int B, int D, int A, int H) { return workspace_bytes<NdqnWs>(B, D, A, H); }
size_t gymrl_ndqn_args_bytes(int which) {
  return which == 0 ? sizeof(gymrl_ndqn_act_args) : which == 1 ? sizeof(gymrl_ndqn_update_args) : which == 2 ? sizeof(gymrl_ndqn_combine_args) : 0;
}

static int ndqn_set_lds_attr() {
  static bool done = false;
  return set_max_lds_once(done, {(const void*)ndqn_r1_kernel, (const void*)ndqn_act_kernel}, (int)lds_bytes(256, kNdqnSlabs));
}

int gymrl_ndqn_combine(const gymrl_ndqn_combine_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_ndqn_combine_args& a = *args;
  if (!ndqn_shape_ok(1, a.D, a.A, a.H) || !a.workspace || !ndqn_net_ok(a.policy, true)) return -22;
  NdqnWs ws;
  NdqnWs::carve(&ws, align256(a.workspace), 1, a.D, a.A, a.H);      // (the parameter sets come first: no B in their places)
  const int total = 3 * ndqn_count(a.D, a.A, a.H);
  hipLaunchKernelGGL(ndqn_combine_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream_, a, ws);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_ndqn_act_step(const gymrl_ndqn_act_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_ndqn_act_args& a = *args;
  if (!act_args_ok(a, GYMRL_ENV_CARTPOLE, /*refuse_neg_cursor=*/true) || !a.workspace) return -22;
  if (const int rc = ndqn_set_lds_attr()) return rc;
  NdqnWs ws;
  NdqnWs::carve(&ws, align256(const_cast<void*>(a.workspace)), 1, a.D, a.A, a.H);
  hipLaunchKernelGGL(ndqn_act_kernel, dim3((a.N + 15) / 16), dim3(kThreads), lds_bytes(a.H, 2), (hipStream_t)stream_, a, ws);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_ndqn_update(const gymrl_ndqn_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_ndqn_update_args& a = *args;
  if (!ndqn_shape_ok(a.B, a.D, a.A, a.H)) return -22;
  if (!ring_ok(a) || !all_set({a.workspace, a.loss_sum, a.policy_p, a.policy_m, a.policy_v}) || !draw_ok(a, /*idx_dev_counts=*/true) || a.cap < 1)
    return -22;
  if (!ndqn_net_ok(a.policy, true) || !ndqn_net_ok(a.target, false)) return -22;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = ndqn_set_lds_attr()) return rc;
  NdqnWs ws;
  NdqnWs::carve(&ws, align256(a.workspace), a.B, a.D, a.A, a.H);
  const int B = a.B, D = a.D, A = a.A, H = a.H, slabs = (B + 15) / 16;
  // set A's tile list: the gradients of the EFFECTIVE parameters are stored (store_grads), the optimiser runs behind them
  DwArgs p{};
  DwBuilder pb{p, B};
  pb.seg(ws.Z1, H, H, ws.s, D, nullptr, 0, D, D, ws.gw[0], ws.gb[0]);
  pb.seg(ws.Z2, H, H, ws.H1, H, nullptr, 0, H, H, ws.gw[1], ws.gb[1]);
  pb.seg(ws.dv, 1, 1, ws.H2, H, nullptr, 0, H, H, ws.gw[2], ws.gb[2]);              // the value head: dv [B][1]
  pb.seg(ws.da, A, A, ws.H2, H, nullptr, 0, H, H, ws.gw[3], ws.gb[3]);              // the advantage head: da [B][A]
  // (at most 256 rows: no slice partials, and the loss sum closes in this launch's last block — dqn_td_kernel's one block)
  pb.close(a, nullptr, a.policy_p, a.policy_m, a.policy_v, a.adam_policy, a.adam_policy_dev, 0.0f, 0.0f, ws.terms, nullptr, 0, 1, a.loss_sum);
  p.store_grads = 1;
  NdqnAdamArgs ad{};
  ad.p = a.policy; ad.D = D; ad.A = A; ad.H = H;
  ad.base = a.policy_p; ad.m = a.policy_m; ad.v = a.policy_v;
  for (int k = 0; k < 4; ++k) ad.adam[k] = a.adam_policy[k];
  ad.adam_dev = a.adam_policy_dev;
  ad.omb1 = (float)(1.0 - a.beta1); ad.beta2 = (float)a.beta2; ad.omb2 = (float)(1.0 - a.beta2); ad.eps = (float)a.eps_adam;
  hipLaunchKernelGGL(ndqn_r1_kernel, dim3(slabs), dim3(kThreads), lds_bytes(H, kNdqnSlabs), stream, a, ws);
  launch_dw(p, stream);
  hipLaunchKernelGGL(ndqn_adam_kernel, dim3((ndqn_count(D, A, H) + 255) / 256), dim3(256), 0, stream, ad, ws);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
