// es.hip — the small stages of the evolution-strategies learners around the one-launch population evaluators: OpenAI-ES
//  and separable NES (at the end of this file; it shares the noise, the ranks and the chunk layout).
//
//   gymrl_es_perturb     theta -> the population stack: row 2k = theta + sigma eps_k, row 2k + 1 = theta - sigma eps_k (mirrored
//                        sampling), one Philox call per four elements of a pair, float4 stores, nothing else touched
//   gymrl_es_shape_grad  returns -> fitness -> centred ranks (by counting, ties averaged) -> the search gradient
//                        -(1 / (P sigma)) sum_k (w_2k - w_2k+1) eps_k, the eps drawn again in registers
//   gymrl_es_noise       eps itself, for tests and tools
//   gymrl_snes_perturb   mu, sigma[n] -> the population stack, gymrl_es_perturb's body under a step size per element
//   gymrl_snes_tell      returns (float32 or float64) -> ranks -> sum_k u_k eps_k and sum_k s_k (eps_k^2 - 1) in the gradient's
//                        chunk layout, and mu and sigma stepped in place by the thread that closes an element's sums
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
// the step size of an element: OpenAI-ES has one for all, separable NES one each (f32[n], 16-byte aligned)
struct scalar_sigma {
  float s;
  __device__ __forceinline__ float4 quad(uint32_t) const { return make_float4(s, s, s, s); }
  __device__ __forceinline__ float at(size_t) const { return s; }
};
struct vector_sigma {
  const float* s;
  __device__ __forceinline__ float4 quad(uint32_t j) const { return *reinterpret_cast<const float4*>(s + 4u * (size_t)j); }
  __device__ __forceinline__ float at(size_t i) const { return s[i]; }
};

// rows 2k / 2k + 1 of params <- centre +- sigma * eps_k for the quad of elements this thread owns
template <typename Sigma>
__device__ __forceinline__ void perturb_quad(const float* centre, const Sigma sigma, int n, int64_t stride, uint64_t seed,
                                             uint64_t generation, float* params) {
  const uint32_t nq = ((uint32_t)n + 3u) >> 2;
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x, k = blockIdx.y;
  if (j >= nq) return;
  const es_quad q = es_eps4(seed, generation, k, j);
  const float* th = centre + 4u * (size_t)j;
  float* plus = params + (size_t)(2u * k) * (size_t)stride + 4u * (size_t)j;
  float* minus = plus + stride;
  const int left = n - (int)(4u * j);
  if (left >= 4) {                                           // the centre and the rows are 16-byte aligned, stride % 4 == 0
    const float4 t = *reinterpret_cast<const float4*>(th), sg = sigma.quad(j);
    const float s0 = sg.x * q.z[0], s1 = sg.y * q.z[1], s2 = sg.z * q.z[2], s3 = sg.w * q.z[3];
    *reinterpret_cast<float4*>(plus) = make_float4(t.x + s0, t.y + s1, t.z + s2, t.w + s3);
    *reinterpret_cast<float4*>(minus) = make_float4(t.x - s0, t.y - s1, t.z - s2, t.w - s3);
    return;
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    if (e >= left) break;
    const float t = th[e], s = sigma.at(4u * (size_t)j + (size_t)e) * q.z[e];
    plus[e] = t + s;
    minus[e] = t - s;
  }
}

__global__ void __launch_bounds__(kThreads) es_perturb_kernel(const gymrl_es_perturb_args a) {
  perturb_quad(a.theta, scalar_sigma{a.sigma}, a.n, a.stride, a.seed, a.generation, a.params);
}

// ------------------------------------------------------- fitness and ranks ---
// F[p] = the float64 sum of row p in ascending e, for every p, by the calling workgroup (R: float, each term widened, or double)
template <int T, typename R>
__device__ __forceinline__ void fitness_to_lds(const R* __restrict__ returns, int P, int E, double* F) {
  for (int p = threadIdx.x; p < P; p += T) {
    const R* row = returns + (size_t)p * (size_t)E;
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

template <typename R>
__global__ void __launch_bounds__(kThreads) es_rank_kernel(const R* __restrict__ returns, int P, int E, float* weights) {
  __shared__ double F[kMaxP];
  fitness_to_lds<kThreads>(returns, P, E, F);
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p < P) weights[p] = centred_rank(F, P, p);
}

// The fused start of a chunk-sum workgroup (P <= kFusedMaxP): every workgroup counts the ranks itself, thread p holds w_p,
// workgroup 0 writes them out.  -> w_p and w_p+1 (lanes 2k and 2k + 1 sit in one wave); threads p >= P hold zeros.
template <typename R>
__device__ __forceinline__ float fused_ranks(const R* __restrict__ returns, int P, int E, double* F, float* weights, float* w_next) {
  fitness_to_lds<kGradThreads>(returns, P, E, F);
  float w = 0.0f;
  if ((int)threadIdx.x < P) {
    w = centred_rank(F, P, threadIdx.x);
    if (blockIdx.x == 0) weights[threadIdx.x] = w;
  }
  *w_next = __shfl_down(w, 1, 64);
  return w;
}

// ----------------------------------------------------------- chunk layout ---
// CY chunk slots x (kGradThreads / CY) quads of elements per workgroup: thread (c, ql) sums chunk c of quad j; its W doubles
// per element go to part[] in slot() order; element t of the workgroup is then closed by one thread over the chunks in
// ascending order, total().  W: the sums kept per element (1: the search gradient; 2: separable NES's two moments).
struct chunk_layout {
  int pairs, n_chunks, QX, c, ql;
  uint32_t nq, j;
  __device__ __forceinline__ chunk_layout(int P, int n, int cy_log2)
      : pairs(P >> 1), n_chunks(((P >> 1) + kChunk - 1) / kChunk), QX(kGradThreads >> cy_log2),
        c((int)threadIdx.x & ((1 << cy_log2) - 1)), ql((int)threadIdx.x >> cy_log2), nq(((uint32_t)n + 3u) >> 2),
        j(blockIdx.x * (uint32_t)(kGradThreads >> cy_log2) + (uint32_t)((int)threadIdx.x >> cy_log2)) {}
  __device__ __forceinline__ bool active() const { return c < n_chunks && j < nq; }
  __device__ __forceinline__ int k_begin() const { return c * kChunk; }
  __device__ __forceinline__ int k_end() const { return min(pairs, (c + 1) * kChunk); }
  __device__ __forceinline__ int slot(int e) const { return (c * QX + ql) * 4 + e; }               // of this thread's element e
  __device__ __forceinline__ int elements() const { return QX * 4; }                               // of this workgroup
  __device__ __forceinline__ uint32_t element(int t) const { return 4u * (blockIdx.x * (uint32_t)QX) + (uint32_t)t; }
  __device__ __forceinline__ double total(const double* part, int t) const {
    double S = 0.0;
    for (int cc = 0; cc < n_chunks; ++cc) S = S + part[cc * QX * 4 + t];
    return S;
  }
};

// host: the grid of a chunk-sum kernel and its log2(CY)
dim3 chunk_grid(int P, int n, int* cy_log2) {
  const int n_chunks = (P / 2 + kChunk - 1) / kChunk;
  *cy_log2 = 0;
  while ((1 << *cy_log2) < n_chunks) ++*cy_log2;
  const unsigned QX = kGradThreads >> *cy_log2, nq = ((unsigned)n + 3u) / 4u;
  return dim3((nq + QX - 1) / QX);
}

// --------------------------------------------------------------- gradient ---
// kFused: the ranks are counted here (P <= kFusedMaxP), workgroup 0 writes them out; otherwise they are es_rank_kernel's in
// a.weights.
template <bool kFused>
__global__ void __launch_bounds__(kGradThreads) es_grad_kernel(const gymrl_es_shape_grad_args a, int cy_log2) {
  __shared__ double part[kGradThreads * 4];
  __shared__ double F[kFused ? kFusedMaxP : 1];
  __shared__ float u_lds[kFused ? kFusedMaxP / 2 : 1];
  if (kFused) {
    float w_odd;
    const float w = fused_ranks(a.returns, a.P, a.E, F, a.weights, &w_odd);
    if ((int)threadIdx.x < a.P && (threadIdx.x & 1u) == 0) u_lds[threadIdx.x >> 1] = w - w_odd;
    __syncthreads();
  }
  const chunk_layout L(a.P, a.n, cy_log2);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (L.active()) {
    const int k_end = L.k_end();
    for (int k = L.k_begin(); k < k_end; ++k) {
      const double u = (double)(kFused ? u_lds[k] : a.weights[2 * k] - a.weights[2 * k + 1]);
      const es_quad q = es_eps4(a.seed, a.generation, (uint32_t)k, L.j);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = acc[e] + u * (double)q.z[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) part[L.slot(e)] = acc[e];
  __syncthreads();
  const double coef = -(1.0 / ((double)a.P * (double)a.sigma));
  for (int t = threadIdx.x; t < L.elements(); t += kGradThreads) {
    const uint32_t i = L.element(t);
    if (i >= (uint32_t)a.n) break;
    a.grad[i] = (float)(coef * L.total(part, t));
  }
}

// ---------------------------------------------------------- separable NES ---
__global__ void __launch_bounds__(kThreads) snes_perturb_kernel(const gymrl_snes_perturb_args a) {
  perturb_quad(a.mu, vector_sigma{a.sigma}, a.n, a.stride, a.seed, a.generation, a.params);
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) {
  v = v < lo ? lo : v;
  return v > hi ? hi : v;
}

// es_grad_kernel's layout with two sums per element, and the step in the same launch: the thread that closes element i's
// chunk sums is the only one that reads or writes mu[i] and sigma[i], so both move in place.  R: the returns' type.
template <bool kFused, typename R>
__global__ void __launch_bounds__(kGradThreads) snes_tell_kernel(const gymrl_snes_tell_args a, const R* __restrict__ returns,
                                                                 int cy_log2) {
  __shared__ double part_mu[kGradThreads * 4], part_sg[kGradThreads * 4];         // 2 x 8 KB
  __shared__ double F[kFused ? kFusedMaxP : 1];                                    // 2 KB
  __shared__ float u_lds[kFused ? kFusedMaxP / 2 : 1], s_lds[kFused ? kFusedMaxP / 2 : 1];
  if (kFused) {
    float w_odd;
    const float w = fused_ranks(returns, a.P, a.E, F, a.weights, &w_odd);
    if ((int)threadIdx.x < a.P && (threadIdx.x & 1u) == 0) {
      u_lds[threadIdx.x >> 1] = w - w_odd;
      s_lds[threadIdx.x >> 1] = w + w_odd;
    }
    __syncthreads();
  }
  const chunk_layout L(a.P, a.n, cy_log2);
  double am[4] = {0.0, 0.0, 0.0, 0.0}, as[4] = {0.0, 0.0, 0.0, 0.0};
  if (L.active()) {
    const int k_end = L.k_end();
    for (int k = L.k_begin(); k < k_end; ++k) {
      const double u = (double)(kFused ? u_lds[k] : a.weights[2 * k] - a.weights[2 * k + 1]);
      const double s = (double)(kFused ? s_lds[k] : a.weights[2 * k] + a.weights[2 * k + 1]);
      const es_quad q = es_eps4(a.seed, a.generation, (uint32_t)k, L.j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double z = (double)q.z[e];
        am[e] = am[e] + u * z;
        as[e] = as[e] + s * (z * z - 1.0);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    part_mu[L.slot(e)] = am[e];
    part_sg[L.slot(e)] = as[e];
  }
  __syncthreads();
  const double c = 4.0 / (double)a.P;
  for (int t = threadIdx.x; t < L.elements(); t += kGradThreads) {
    const uint32_t i = L.element(t);
    if (i >= (uint32_t)a.n) break;
    const double Smu = L.total(part_mu, t), Ssg = L.total(part_sg, t);
    const float sigma = a.sigma[i];
    a.mu[i] = (float)((double)a.mu[i] + (double)a.eta_mu * ((double)sigma * (c * Smu)));
    a.sigma[i] = clampf(sigma * det_expf((float)(0.5 * (double)a.eta_sigma * (c * Ssg))), a.sigma_min, a.sigma_max);
  }
}

template <typename R>
int snes_tell_launch(const gymrl_snes_tell_args& a, const R* returns, hipStream_t stream) {
  int cy_log2;
  const dim3 grid = chunk_grid(a.P, a.n, &cy_log2), block(kGradThreads);
  if (a.P <= kFusedMaxP) {
    hipLaunchKernelGGL((snes_tell_kernel<true, R>), grid, block, 0, stream, a, returns, cy_log2);
  } else {
    hipLaunchKernelGGL(es_rank_kernel<R>, dim3((unsigned)((a.P + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, returns, a.P,
                       a.E, a.weights);
    GYMRL_CHECK_LAUNCH();
    hipLaunchKernelGGL((snes_tell_kernel<false, R>), grid, block, 0, stream, a, returns, cy_log2);
  }
  GYMRL_CHECK_LAUNCH();
  return 0;
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
  int cy_log2;
  const dim3 grid = chunk_grid(a.P, a.n, &cy_log2), block(kGradThreads);
  if (a.P <= kFusedMaxP) {
    hipLaunchKernelGGL(es_grad_kernel<true>, grid, block, 0, (hipStream_t)stream, a, cy_log2);
  } else {
    hipLaunchKernelGGL(es_rank_kernel<float>, dim3((unsigned)((a.P + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       a.returns, a.P, a.E, a.weights);
    GYMRL_CHECK_LAUNCH();
    hipLaunchKernelGGL(es_grad_kernel<false>, grid, block, 0, (hipStream_t)stream, a, cy_log2);
  }
  GYMRL_CHECK_LAUNCH();
  return 0;
}

size_t gymrl_snes_perturb_args_bytes(void) { return sizeof(gymrl_snes_perturb_args); }
size_t gymrl_snes_tell_args_bytes(void) { return sizeof(gymrl_snes_tell_args); }

int gymrl_snes_perturb(const gymrl_snes_perturb_args* args, void* stream) {
  if (!args) return -22;
  const gymrl_snes_perturb_args& a = *args;
  if (!a.mu || !a.sigma || !a.params) return -22;
  if (((uintptr_t)a.mu & 15u) || ((uintptr_t)a.sigma & 15u) || ((uintptr_t)a.params & 15u)) return -22;
  if (a.n < 1 || !population_ok(a.P)) return -22;
  if (a.stride < a.n || (a.stride & 3) != 0) return -22;
  const dim3 grid((((unsigned)a.n + 3u) / 4u + kThreads - 1) / kThreads, (unsigned)(a.P / 2)), block(kThreads);
  hipLaunchKernelGGL(snes_perturb_kernel, grid, block, 0, (hipStream_t)stream, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_snes_tell(const gymrl_snes_tell_args* args, void* stream) {
  if (!args) return -22;
  const gymrl_snes_tell_args& a = *args;
  if (!a.mu || !a.sigma || !a.weights || (a.returns != nullptr) == (a.returns64 != nullptr)) return -22;
  if (((uintptr_t)a.mu & 15u) || ((uintptr_t)a.sigma & 15u) || ((uintptr_t)a.weights & 3u)) return -22;
  if (((uintptr_t)a.returns & 3u) || ((uintptr_t)a.returns64 & 7u)) return -22;
  if (a.n < 1 || a.E < 1 || !population_ok(a.P)) return -22;
  if (!std::isfinite(a.eta_mu) || !std::isfinite(a.eta_sigma)) return -22;
  if (!sigma_ok(a.sigma_min) || !sigma_ok(a.sigma_max) || a.sigma_min > a.sigma_max) return -22;
  return a.returns ? snes_tell_launch(a, a.returns, (hipStream_t)stream) : snes_tell_launch(a, a.returns64, (hipStream_t)stream);
}

}  // extern "C"
