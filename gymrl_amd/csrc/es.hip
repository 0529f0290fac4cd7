// es.hip — the three small stages of OpenAI-ES around the one-launch population evaluators.
//
//   gymrl_es_perturb     theta -> the population stack: row 2k = theta + sigma eps_k, row 2k + 1 = theta - sigma eps_k (mirrored
//                        sampling), one Philox call per four elements of a pair, float4 stores, nothing else touched
//   gymrl_es_shape_grad  returns -> fitness -> centred ranks (by counting, ties averaged) -> the search gradient
//                        -(1 / (P sigma)) sum_k (w_2k - w_2k+1) eps_k, the eps drawn again in registers
//   gymrl_es_noise       eps itself, for tests and tools
//
// eps is es_noise_device.hpp's and nothing else.  The gradient's float64 sum has a fixed order: pairs in consecutive chunks of
// GYMRL_ES_PAIR_CHUNK, a chunk summed by ONE thread in ascending k, the chunk partials added in ascending chunk order by one
// thread from LDS — no atomics, so the same bits whatever the grid.  A workgroup owns kGradThreads / CY quads of elements and
// CY chunk slots (CY: the chunk count rounded up to a power of two, at most 256 = 4096 pairs / 16).
//
// Ranks need every fitness and the gradient needs every rank.  Up to kFusedMaxP policies every gradient workgroup recounts the
// ranks itself in LDS (P^2 / 256 comparisons per thread: below a launch's latency) and the entry point is ONE launch; above,
// a rank kernel of P / 256 workgroups runs first, each with all P fitness values in LDS (64 KB at the cap) and one policy per
// thread — one workgroup alone would spend P^2 / 1024 dependent LDS reads per thread, 2 ms at P = 8192.
#include "es_noise_device.hpp"
#include "../../include/gymrl.h"

#include <cmath>

namespace {

using namespace gymrl;

constexpr int kChunk = GYMRL_ES_PAIR_CHUNK;
constexpr int kMaxP = 8192, kFusedMaxP = 256, kThreads = 256, kGradThreads = 256;
static_assert(kMaxP / 2 / kChunk <= kGradThreads, "one chunk slot per thread at the cap");

// ------------------------------------------------------------------ noise ---
__global__ void __launch_bounds__(kThreads) es_noise_kernel(const gymrl_es_noise_args a) {
  const uint32_t nq = ((uint32_t)a.n + 3u) >> 2;
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x, row = blockIdx.y;
  if (j >= nq) return;
  const es_quad q = es_eps4(a.seed, a.generation, (uint32_t)a.k0 + row, j);
  float* out = a.out + (size_t)row * (size_t)a.n + 4u * (size_t)j;
  const int left = a.n - (int)(4u * j);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < left) out[e] = q.z[e];
}

// ---------------------------------------------------------------- perturb ---
__global__ void __launch_bounds__(kThreads) es_perturb_kernel(const gymrl_es_perturb_args a) {
  const uint32_t nq = ((uint32_t)a.n + 3u) >> 2;
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x, k = blockIdx.y;
  if (j >= nq) return;
  const es_quad q = es_eps4(a.seed, a.generation, k, j);
  const float* th = a.theta + 4u * (size_t)j;
  float* plus = a.params + (size_t)(2u * k) * (size_t)a.stride + 4u * (size_t)j;
  float* minus = plus + a.stride;
  const int left = a.n - (int)(4u * j);
  if (left >= 4) {                                           // theta and the rows are 16-byte aligned, stride % 4 == 0
    const float4 t = *reinterpret_cast<const float4*>(th);
    const float s0 = a.sigma * q.z[0], s1 = a.sigma * q.z[1], s2 = a.sigma * q.z[2], s3 = a.sigma * q.z[3];
    *reinterpret_cast<float4*>(plus) = make_float4(t.x + s0, t.y + s1, t.z + s2, t.w + s3);
    *reinterpret_cast<float4*>(minus) = make_float4(t.x - s0, t.y - s1, t.z - s2, t.w - s3);
    return;
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    if (e >= left) break;
    const float t = th[e], s = a.sigma * q.z[e];
    plus[e] = t + s;
    minus[e] = t - s;
  }
}

// ------------------------------------------------------- fitness and ranks ---
// F[p] = the float64 sum of row p in ascending e, for every p, by the calling workgroup
template <int T>
__device__ __forceinline__ void fitness_to_lds(const float* __restrict__ returns, int P, int E, double* F) {
  for (int p = threadIdx.x; p < P; p += T) {
    const float* row = returns + (size_t)p * (size_t)E;
    double s = 0.0;
    for (int e = 0; e < E; ++e) s += (double)row[e];
    F[p] = s;
  }
  __syncthreads();
}

// the centred rank of policy p among F[0 .. P): counting, ties averaged
__device__ __forceinline__ float centred_rank(const double* F, int P, int p) {
  const double f = F[p];
  int less = 0, equal = 0;
#pragma unroll 8
  for (int q = 0; q < P; ++q) {
    const double g = F[q];
    less += g < f;
    equal += g == f;
  }
  return (float)(2 * less + equal - 1) / (float)(2 * (P - 1)) - 0.5f;
}

__global__ void __launch_bounds__(kThreads) es_rank_kernel(const gymrl_es_shape_grad_args a) {
  __shared__ double F[kMaxP];
  fitness_to_lds<kThreads>(a.returns, a.P, a.E, F);
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p < a.P) a.weights[p] = centred_rank(F, a.P, p);
}

// --------------------------------------------------------------- gradient ---
// CY chunk slots x (kGradThreads / CY) quads per workgroup.  kFused: the ranks are counted here (P <= kFusedMaxP), workgroup 0
// writes them out; otherwise they are es_rank_kernel's in a.weights.
template <bool kFused>
__global__ void __launch_bounds__(kGradThreads) es_grad_kernel(const gymrl_es_shape_grad_args a, int cy_log2) {
  __shared__ double part[kGradThreads * 4];
  __shared__ double F[kFused ? kFusedMaxP : 1];
  __shared__ float u_lds[kFused ? kFusedMaxP / 2 : 1];
  const int pairs = a.P >> 1, n_chunks = (pairs + kChunk - 1) / kChunk;
  const int CY = 1 << cy_log2, QX = kGradThreads >> cy_log2;
  if (kFused) {
    fitness_to_lds<kGradThreads>(a.returns, a.P, a.E, F);
    float w = 0.0f;
    if ((int)threadIdx.x < a.P) {
      w = centred_rank(F, a.P, threadIdx.x);
      if (blockIdx.x == 0) a.weights[threadIdx.x] = w;
    }
    const float w_odd = __shfl_down(w, 1, 64);               // lanes 2k and 2k + 1 sit in one wave
    if ((int)threadIdx.x < a.P && (threadIdx.x & 1u) == 0) u_lds[threadIdx.x >> 1] = w - w_odd;
    __syncthreads();
  }
  const int c = threadIdx.x & (CY - 1), ql = threadIdx.x >> cy_log2;
  const uint32_t nq = ((uint32_t)a.n + 3u) >> 2, j = blockIdx.x * (uint32_t)QX + (uint32_t)ql;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (c < n_chunks && j < nq) {
    const int k_end = min(pairs, (c + 1) * kChunk);
    for (int k = c * kChunk; k < k_end; ++k) {
      const double u = (double)(kFused ? u_lds[k] : a.weights[2 * k] - a.weights[2 * k + 1]);
      const es_quad q = es_eps4(a.seed, a.generation, (uint32_t)k, j);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = acc[e] + u * (double)q.z[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) part[(c * QX + ql) * 4 + e] = acc[e];
  __syncthreads();
  const double coef = -(1.0 / ((double)a.P * (double)a.sigma));
  for (int t = threadIdx.x; t < QX * 4; t += kGradThreads) {                // element (ql, e) = t of this workgroup
    const uint32_t i = 4u * (blockIdx.x * (uint32_t)QX) + (uint32_t)t;
    if (i >= (uint32_t)a.n) break;
    double S = 0.0;
    for (int cc = 0; cc < n_chunks; ++cc) S = S + part[cc * QX * 4 + t];
    a.grad[i] = (float)(coef * S);
  }
}

bool sigma_ok(float s) { return std::isfinite(s) && s > 0.0f; }
bool population_ok(int P) { return P >= 2 && P <= kMaxP && (P & 1) == 0; }

}  // namespace

extern "C" {

int gymrl_es_pair_chunk(void) { return kChunk; }
size_t gymrl_es_noise_args_bytes(void) { return sizeof(gymrl_es_noise_args); }
size_t gymrl_es_perturb_args_bytes(void) { return sizeof(gymrl_es_perturb_args); }
size_t gymrl_es_shape_grad_args_bytes(void) { return sizeof(gymrl_es_shape_grad_args); }

int gymrl_es_noise(const gymrl_es_noise_args* args, void* stream) {
  if (!args) return -22;
  const gymrl_es_noise_args& a = *args;
  if (!a.out || ((uintptr_t)a.out & 3u)) return -22;
  if (a.n < 1 || a.K < 1 || a.k0 < 0 || a.k0 > kMaxP / 2 - a.K) return -22;      // pairs of a population: [0, 4096)
  const dim3 grid((((unsigned)a.n + 3u) / 4u + kThreads - 1) / kThreads, (unsigned)a.K), block(kThreads);
  hipLaunchKernelGGL(es_noise_kernel, grid, block, 0, (hipStream_t)stream, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_es_perturb(const gymrl_es_perturb_args* args, void* stream) {
  if (!args) return -22;
  const gymrl_es_perturb_args& a = *args;
  if (!a.theta || !a.params || ((uintptr_t)a.theta & 15u) || ((uintptr_t)a.params & 15u)) return -22;
  if (a.n < 1 || !population_ok(a.P) || !sigma_ok(a.sigma)) return -22;
  if (a.stride < a.n || (a.stride & 3) != 0) return -22;
  const dim3 grid((((unsigned)a.n + 3u) / 4u + kThreads - 1) / kThreads, (unsigned)(a.P / 2)), block(kThreads);
  hipLaunchKernelGGL(es_perturb_kernel, grid, block, 0, (hipStream_t)stream, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_es_shape_grad(const gymrl_es_shape_grad_args* args, void* stream) {
  if (!args) return -22;
  const gymrl_es_shape_grad_args& a = *args;
  if (!a.returns || !a.grad || !a.weights) return -22;
  if (((uintptr_t)a.returns & 3u) || ((uintptr_t)a.grad & 3u) || ((uintptr_t)a.weights & 3u)) return -22;
  if (a.n < 1 || a.E < 1 || !population_ok(a.P) || !sigma_ok(a.sigma)) return -22;
  const int n_chunks = (a.P / 2 + kChunk - 1) / kChunk;
  int cy_log2 = 0;
  while ((1 << cy_log2) < n_chunks) ++cy_log2;
  const unsigned QX = kGradThreads >> cy_log2, nq = ((unsigned)a.n + 3u) / 4u;
  const dim3 grid((nq + QX - 1) / QX), block(kGradThreads);
  if (a.P <= kFusedMaxP) {
    hipLaunchKernelGGL(es_grad_kernel<true>, grid, block, 0, (hipStream_t)stream, a, cy_log2);
  } else {
    hipLaunchKernelGGL(es_rank_kernel, dim3((unsigned)((a.P + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, a);
    GYMRL_CHECK_LAUNCH();
    hipLaunchKernelGGL(es_grad_kernel<false>, grid, block, 0, (hipStream_t)stream, a, cy_log2);
  }
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
