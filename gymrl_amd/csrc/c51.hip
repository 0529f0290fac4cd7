// c51.hip — the categorical (C51, Bellemare et al. 2017) value head: expected values for acting, and the projected
// cross-entropy loss forward / backward in one launch over the rows (the loss sum's finalize launch follows when more than one
// workgroup ran, as in gymrl_dqn_td_loss).
//
//   gymrl_c51_q     logits f32[B][A][M] -> q f32[B][A] = sum_j softmax(logits[b, a, :])_j z_j, first-maximum action
//   gymrl_c51_loss  double-Q / plain target selection, softmax of the target row, projection onto the support, cross-entropy
//                   against log_softmax(logits[b, act_b, :]), d loss / d logits, float64 loss sum
//
// One wave64 per batch row, atom j in lane j (2 <= M <= 64), four rows per 256-thread workgroup, rows dealt to workgroups
// by a grid-stride loop.  The arithmetic is c51_device.hpp's; its header states the two sum orders (the 64-slot butterfly for
// sums over a row's atoms, j ascending for the projection).  Neither depends on B or on the grid: a row's outputs are the
// same bits wherever in a batch it sits, dlogits' factor w_b * (1 / B) aside.  The projection is the GATHER form
//   m_i = sum_j p*_j max(0, 1 - |b_j - i|)
// of the textbook floor / ceil scatter: no atomics, hence no scheduling in the bits; p*_j and b_j are read from LDS as
// broadcasts (every lane the same address), M^2 multiply-adds per row.
// The loss sum is the float64 reduction of the other loss kernels (offpolicy.hip): lane 0 of a row's wave carries
// (double)(row_loss_b * w_b), a workgroup adds its four waves ascending, one workgroup adds to loss_sum itself, more write
// partials that finalize sums in a fixed order (row_loss_device.hpp, shared with qrdqn.hip).
#include "c51_device.hpp"
#include "../../include/gymrl.h"

using namespace gymrl;

namespace {

using rowloss::kBlock;
using rowloss::kRows;
using rowloss::grid_for;
using rowloss::block_partial;

__global__ __launch_bounds__(kBlock) void c51_q_kernel(const float* __restrict__ logits, int B, int A, int M, float vmin,
                                                       float dz, float* __restrict__ q_out,
                                                       int32_t* __restrict__ argmax_out) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float z = c51::atom(vmin, dz, lane);
  for (int64_t row = (int64_t)blockIdx.x * kRows + wid; row < B; row += (int64_t)gridDim.x * kRows) {
    const int arg = c51::greedy_action(logits + (size_t)row * A * M, A, M, lane, z, q_out + (size_t)row * A);
    if (argmax_out && lane == 0) argmax_out[row] = arg;
  }
}

__global__ __launch_bounds__(kBlock) void c51_loss_kernel(
    const float* __restrict__ logits, const float* __restrict__ next_online, const float* __restrict__ next_target,
    const int32_t* __restrict__ act, const float* __restrict__ rew, const float* __restrict__ flag,
    const float* __restrict__ w, int B, int A, int M, float vmin, float vmax, float dz, float gamma_n,
    float* __restrict__ row_loss_out, float* __restrict__ dlogits_out, double* __restrict__ partials,
    double* __restrict__ direct) {
  __shared__ float sp[kRows][c51::kMaxAtoms], sb[kRows][c51::kMaxAtoms];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool on = lane < M;
  const float z = c51::atom(vmin, dz, lane);
  const float invB = 1.0f / (float)B;
  double acc = 0.0;
  // every wave of a workgroup makes the same number of trips (the barriers below), a wave past the batch's end idles
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < B; base += (int64_t)gridDim.x * kRows) {
    const int64_t row = base + wid;
    const bool live = row < B;
    if (live) {
      const float* sel = (next_online ? next_online : next_target) + (size_t)row * A * M;
      const int astar = c51::greedy_action(sel, A, M, lane, z, nullptr);
      sp[wid][lane] = c51::prob_lane(next_target + ((size_t)row * A + astar) * M, M, lane);
      sb[wid][lane] = c51::project_pos(rew[row], gamma_n * (1.0f - flag[row]), z, vmin, vmax, dz);
    }
    __syncthreads();
    if (live) {
      const float m = c51::project_mass(sp[wid], sb[wid], M, lane);
      const int a = act[row];
      const bool valid = (unsigned)a < (unsigned)A;      // an action outside [0, A) reads and writes nothing out of range:
      float d = 0.0f, e = 0.0f, s = 1.0f;                // the row's loss is NaN and its gradient 0
      if (valid) c51::softmax_lane(on ? logits[((size_t)row * A + a) * M + lane] : 0.0f, on, d, e, s);
      const float logp = d - det_logf(s);
      const float row_loss = valid ? -c51::wave_allsum(on ? m * logp : 0.0f) : __builtin_nanf("");
      const float wb = w ? w[row] : 1.0f;
      const float g = (wb * invB) * (e / s - m);
      if (on)
        for (int k = 0; k < A; ++k) dlogits_out[((size_t)row * A + k) * M + lane] = (valid && k == a) ? g : 0.0f;
      if (lane == 0) {
        row_loss_out[row] = row_loss;
        acc += (double)(row_loss * wb);
      }
    }
    __syncthreads();
  }
  if (partials) block_partial(acc, partials, direct);
}

inline bool shape_ok(int B, int A, int M, float vmin, float vmax) {
  if (B < 0 || A < 1 || A > c51::kMaxActions || M < 2 || M > c51::kMaxAtoms || !(vmax > vmin)) return false;
  const float dz = (vmax - vmin) / (float)(M - 1);
  return dz > 0.0f && dz < __builtin_inff();
}

}  // namespace

extern "C" {

int gymrl_c51_q(const float* logits, int B, int A, int M, float vmin, float vmax, float* q_out, int32_t* argmax_out,
                void* stream_) {
  if (!logits || !q_out || !shape_ok(B, A, M, vmin, vmax)) return -22;
  if (B == 0) return 0;
  const float dz = (vmax - vmin) / (float)(M - 1);
  hipLaunchKernelGGL(c51_q_kernel, dim3(grid_for(B)), dim3(kBlock), 0, (hipStream_t)stream_, logits, B, A, M, vmin, dz,
                     q_out, argmax_out);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_c51_loss(const float* logits, const float* next_online, const float* next_target, const int32_t* act,
                   const float* rew, const float* flag, const float* w, int B, int A, int M, float vmin, float vmax,
                   double gamma_n, float* row_loss_out, float* dlogits_out, double* loss_sum, void* workspace,
                   void* stream_) {
  if (!logits || !next_target || !act || !rew || !flag || !row_loss_out || !dlogits_out || !shape_ok(B, A, M, vmin, vmax) ||
      (loss_sum && !workspace))
    return -22;
  if (B == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  const float dz = (vmax - vmin) / (float)(M - 1);
  const int nb = grid_for(B);
  double* parts = loss_sum ? (double*)workspace : nullptr;
  hipLaunchKernelGGL(c51_loss_kernel, dim3(nb), dim3(kBlock), 0, stream, logits, next_online, next_target, act, rew, flag, w,
                     B, A, M, vmin, vmax, dz, (float)gamma_n, row_loss_out, dlogits_out, parts,
                     (loss_sum && nb == 1) ? loss_sum : nullptr);
  if (loss_sum && nb > 1) hipLaunchKernelGGL(rowloss::finalize_kernel, dim3(1), dim3(kBlock), 0, stream, parts, nb, loss_sum);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
