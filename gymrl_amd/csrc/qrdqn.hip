// qrdqn.hip — the quantile-regression (QR-DQN, Dabney et al. 2018) value head: mean quantiles for acting, and the quantile-Huber
// loss forward / backward in one launch over the rows (the loss sum's finalize launch follows when more than one workgroup ran,
// as in gymrl_c51_loss).
//
//   gymrl_qr_q     quant f32[B][A][N] -> q f32[B][A] = mean_i quant[b, a, i], first-maximum action
//   gymrl_qr_loss  double-Q / plain target selection, the Bellman map of the target row's quantiles, the N x N quantile-Huber
//                  loss against quant[b, act_b, :], d loss / d quant, float64 loss sum
//
// c51.hip's launch shape (row_loss_device.hpp): one wave64 per batch row, quantile i in lane i (1 <= N <= 64), four rows per
// 256-thread workgroup, rows dealt to workgroups by a grid-stride loop.  The arithmetic is qrdqn_device.hpp's; its header states
// the two sum orders (the 64-slot butterfly over a row's lanes, j ascending for the pairwise terms) and where 1 / kappa and
// 1 / N sit.  Neither order depends on B or on the grid: a row's outputs are the same bits wherever in a batch it sits, dquant's
// factor w_b * (1 / B) aside.  The row's targets T_j = rew + g * next_target[b, a*, j] go to LDS once (256 B per wave) and come
// back as broadcasts, every lane the same address: N^2 pairwise terms per row, no atomics, no [B, N, N] tensor.
#include "qrdqn_device.hpp"
#include "../../include/gymrl.h"

using namespace gymrl;

namespace {

using rowloss::kBlock;
using rowloss::kRows;
using rowloss::grid_for;
using rowloss::block_partial;

__global__ __launch_bounds__(kBlock) void qr_q_kernel(const float* __restrict__ quant, int B, int A, int N,
                                                      float* __restrict__ q_out, int32_t* __restrict__ argmax_out) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * kRows + wid; row < B; row += (int64_t)gridDim.x * kRows) {
    const int arg = qr::greedy_action(quant + (size_t)row * A * N, A, N, lane, q_out + (size_t)row * A);
    if (argmax_out && lane == 0) argmax_out[row] = arg;
  }
}

__global__ __launch_bounds__(kBlock) void qr_loss_kernel(
    const float* __restrict__ quant, const float* __restrict__ next_online, const float* __restrict__ next_target,
    const int32_t* __restrict__ act, const float* __restrict__ rew, const float* __restrict__ flag,
    const float* __restrict__ w, int B, int A, int N, float kappa, float gamma_n, float* __restrict__ row_loss_out,
    float* __restrict__ dquant_out, double* __restrict__ partials, double* __restrict__ direct) {
  __shared__ float sT[kRows][qr::kMaxQuantiles];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool on = lane < N;
  const float tau_i = qr::tau(lane, N), fN = (float)N;
  const float invB = 1.0f / (float)B;
  double acc = 0.0;
  // every wave of a workgroup makes the same number of trips (the barriers below), a wave past the batch's end idles
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < B; base += (int64_t)gridDim.x * kRows) {
    const int64_t row = base + wid;
    const bool live = row < B;
    if (live) {
      const float* sel = (next_online ? next_online : next_target) + (size_t)row * A * N;
      const int astar = qr::greedy_action(sel, A, N, lane, nullptr);
      const float g = gamma_n * (1.0f - flag[row]);
      sT[wid][lane] = on ? rew[row] + g * next_target[((size_t)row * A + astar) * N + lane] : 0.0f;
    }
    __syncthreads();
    if (live) {
      const int a = act[row];
      const bool valid = (unsigned)a < (unsigned)A;      // an action outside [0, A) reads and writes nothing out of range:
      float l = 0.0f, g = 0.0f;                          // the row's loss is NaN and its gradient 0
      if (valid) qr::pair_sums(sT[wid], N, on ? quant[((size_t)row * A + a) * N + lane] : 0.0f, tau_i, kappa, l, g);
      const float row_loss = valid ? qr::wave_allsum(on ? (l / kappa) / fN : 0.0f) : __builtin_nanf("");
      const float wb = w ? w[row] : 1.0f;
      const float d = (wb * invB) * -((g / kappa) / fN);
      if (on)
        for (int k = 0; k < A; ++k) dquant_out[((size_t)row * A + k) * N + lane] = (valid && k == a) ? d : 0.0f;
      if (lane == 0) {
        row_loss_out[row] = row_loss;
        acc += (double)(row_loss * wb);
      }
    }
    __syncthreads();
  }
  if (partials) block_partial(acc, partials, direct);
}

inline bool shape_ok(int B, int A, int N, float kappa) {
  return B >= 0 && A >= 1 && A <= qr::kMaxActions && N >= 1 && N <= qr::kMaxQuantiles && kappa > 0.0f &&
         kappa < __builtin_inff();
}

}  // namespace

extern "C" {

int gymrl_qr_q(const float* quant, int B, int A, int N, float* q_out, int32_t* argmax_out, void* stream_) {
  if (!quant || !q_out || !shape_ok(B, A, N, 1.0f)) return -22;
  if (B == 0) return 0;
  hipLaunchKernelGGL(qr_q_kernel, dim3(grid_for(B)), dim3(kBlock), 0, (hipStream_t)stream_, quant, B, A, N, q_out,
                     argmax_out);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_qr_loss(const float* quant, const float* next_online, const float* next_target, const int32_t* act,
                  const float* rew, const float* flag, const float* w, int B, int A, int N, float kappa, double gamma_n,
                  float* row_loss_out, float* dquant_out, double* loss_sum, void* workspace, void* stream_) {
  if (!quant || !next_target || !act || !rew || !flag || !row_loss_out || !dquant_out || !shape_ok(B, A, N, kappa) ||
      (loss_sum && !workspace))
    return -22;
  if (B == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  const int nb = grid_for(B);
  double* parts = loss_sum ? (double*)workspace : nullptr;
  hipLaunchKernelGGL(qr_loss_kernel, dim3(nb), dim3(kBlock), 0, stream, quant, next_online, next_target, act, rew, flag, w, B,
                     A, N, kappa, (float)gamma_n, row_loss_out, dquant_out, parts,
                     (loss_sum && nb == 1) ? loss_sum : nullptr);
  if (loss_sum && nb > 1) hipLaunchKernelGGL(rowloss::finalize_kernel, dim3(1), dim3(kBlock), 0, stream, parts, nb, loss_sum);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
