// row_loss_device.hpp — the launch shape and the float64 loss sum of the row-per-wave loss kernels (c51.hip, qrdqn.hip),
// stated once: 256 threads = four wave64s = four batch rows per workgroup, rows dealt to workgroups by a grid-stride loop, the
// grid capped so that one partial per workgroup fits gymrl_reduce_workspace_bytes().
//
// The sum is offpolicy.hip's block_partials<1> / finalize_kernel<1>: the same loads and float64 additions in the same order.
// Lane 0 of a row's wave carries (double)(row_loss_b * w_b) summed over the wave's trips, block_partial adds a workgroup's four
// waves ascending; ONE workgroup adds the result to the caller's slot itself (`direct`), more write partials[blockIdx.x] and
// finalize_kernel (one workgroup) sums them: thread t takes partials t, t + 256, ... ascending, then the same wave / block sum.
#pragma once
#include "gymrl_device.hpp"

namespace gymrl {
namespace rowloss {
namespace {

constexpr int kBlock = 256;
constexpr int kRows = kBlock / GYMRL_WAVE;      // rows per workgroup and grid-stride step
constexpr int kMaxBlocks = 4096;                // <= gymrl_reduce_workspace_bytes() / sizeof(double)
inline int grid_for(int B) {
  const int64_t nb = ((int64_t)B + kRows - 1) / kRows;
  return nb < 1 ? 1 : (nb > kMaxBlocks ? kMaxBlocks : (int)nb);
}

__device__ __forceinline__ void block_partial(double v, double* __restrict__ partials, double* __restrict__ direct) {
  __shared__ double sm[kRows];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const double s = wave_sum(v);
  if (lane == 0) sm[wid] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kRows; ++w) t += sm[w];
    if (direct) direct[0] += t;
    else partials[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(kBlock) void finalize_kernel(const double* __restrict__ partials, int nblocks,
                                                          double* __restrict__ out) {
  __shared__ double sm[kRows];
  double v = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += kBlock) v += partials[i];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const double s = wave_sum(v);
  if (lane == 0) sm[wid] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kRows; ++w) t += sm[w];
    out[0] += t;
  }
}

// the 64-slot butterfly: v_l <- v_l + v_(l ^ 32), then ^ 16, 8, 4, 2, 1.  Every lane ends with the same bits (each level adds
// the same two values in either order), those of the halving tree v[0:off] + v[off:2 off] for off = 32 ... 1 read at slot 0
__device__ __forceinline__ float wave_allsum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

}  // namespace
}  // namespace rowloss
}  // namespace gymrl
