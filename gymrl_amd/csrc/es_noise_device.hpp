// es_noise_device.hpp — the perturbation of the evolution-strategies learner, stated once.
//
// eps(seed, generation, pair k, element i) is a standard normal float32 that nothing stores: gymrl_es_perturb draws it to build
// the population, gymrl_es_shape_grad draws it again to weigh it, gymrl_es_noise writes it out for tests and tools.  The map:
//
//   call      r = Philox4x32-10(key = seed; c0 = i >> 2, c1 = k, c2 = generation & 0xffffffff,
//                               c3 = RNG_ES | ((generation >> 32) & 0x0fffffff))
//   normals   z0 = rho(r.x) cos(2 pi u(r.y))   z1 = rho(r.x) sin(2 pi u(r.y))
//             z2 = rho(r.z) cos(2 pi u(r.w))   z3 = rho(r.z) sin(2 pi u(r.w))
//             rho(w) = sqrtf(-2 det_logf(((w >> 8) + 1) 2^-24)),  u(w) = (w >> 8) 2^-24, det_sincosf for the pair
//   element   eps = z[i & 3]
//
// so four consecutive elements of one pair share a call and all four words of it are used; generations below 2^60 are distinct
// counters (box_muller folds its counter the same way).  RNG_ES has the value csrc/tabular_device.hpp's RNG_TABULAR has: the
// tabular runs key c0 / c1 by their run id and c2 by the step, and no program draws from both.
#pragma once
#include "gymrl_device.hpp"

namespace gymrl {

struct es_quad { float z[4]; };

// the four normals of elements 4 * j .. 4 * j + 3 of pair k
__device__ __forceinline__ es_quad es_eps4(uint64_t seed, uint64_t generation, uint32_t k, uint32_t j) {
  const u32x4 r = philox4x32(seed, j, k, (uint32_t)generation, RNG_ES | (uint32_t)((generation >> 32) & 0x0FFFFFFFu));
  const float ra = sqrtf(-2.0f * det_logf(u01f_open0(r.x))), rb = sqrtf(-2.0f * det_logf(u01f_open0(r.z)));
  float sa, ca, sb, cb;
  det_sincosf(6.28318530717958647692f * u01f(r.y), &sa, &ca);
  det_sincosf(6.28318530717958647692f * u01f(r.w), &sb, &cb);
  return es_quad{{ra * ca, ra * sa, rb * cb, rb * sb}};
}

// one element; the kernels draw by quads, this is the definition they agree with
__device__ __forceinline__ float es_eps(uint64_t seed, uint64_t generation, uint32_t k, uint32_t i) {
  return es_eps4(seed, generation, k, i >> 2).z[i & 3u];
}

}  // namespace gymrl
