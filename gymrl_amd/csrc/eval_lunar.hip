// eval_lunar.hip — whole evaluation episodes of LunarLander-v3 under a PPO policy, P policies x E episodes in ONE launch.
//
// Replaces the eval() loops of ppo_lunarlander.py:368-399 and ppo_full_lunarlander.py (get_action(deterministic=True) ->
// env.step until the episode is over).  Stepped from the host every link of that chain costs the policy forward's launch, the
// pick, the env step, a select and a blocking read-back, up to 1001 times; here a workgroup carries 16 episodes of one policy
// from their reset to their end and never waits for another one.  The loop is eval_lunar_device.hpp's run_lunar_episodes; what
// is stated here is the policy forward of the two networks:
//
//   lunar_eval_kernel       PPO's Linear + Tanh network as gymrl_mlp_forward's stages (mlp_device.hpp forward_tile, the forward
//                           the persistent rollout acts on).  The critic is not on the way to an action: its stages are
//                           forward_tile's skip mask (deferrable_stages) and are never run.  Policy p reads every W and b
//                           p * policy_stride floats behind policy 0's: the workgroup shifts the stage table once, into LDS,
//                           and the forward reads it from there.  Weights are re-read from L2 every step.
//   lunar_eval_mhc_kernel   PPO-full's mHC network (mhc_policy_device.hpp policy_tile) in rollout_lunar_mhc_kernel's LDS layout,
//                           behind a __noinline__ call so that the tile's registers and the solver's are allocated separately.
//
// Every arithmetic piece is the device function the step-by-step path launches, so returns, lengths and terminal observations
// are the loop's bit for bit (tests/test_lunar_eval_gpu.py).
#include "eval_lunar_device.hpp"
#include "mhc_policy_device.hpp"

using namespace gymrl;
using namespace gymrl::lunar;
namespace M = gymrl::mlp;

namespace {

constexpr int kDynFloats = M::kBufs * M::kRows * M::kStride + M::kRows * M::kInStride + M::kRows * M::kHeadStride;
constexpr int kDynBytes = 64 * 1024;       // with the 29 KB of solver columns and parking: > 80 KB, one workgroup per CU
constexpr int kXStride = 16;               // the mHC tile's observation rows
constexpr int kDynBytesMhc = 40 * 1024;    // (its static LDS — policy tile, solver columns, parking — is 48 KB: > 80 KB in all)
static_assert(kDynFloats * 4 <= kDynBytes, "LDS carve-up");
static_assert((M::kRows * kXStride + M::kRows * M::kHeadStride) * 4 <= kDynBytesMhc, "LDS carve-up");

__global__ __launch_bounds__(kEvalThreads) void lunar_eval_kernel(const gymrl_lunar_eval_args a, const gymrl_mlp_desc d) {
  extern __shared__ __attribute__((aligned(16))) float dyn_lds[];
  __shared__ uint32_t lds_words[kLdsWords * kEnvBlock];            // the solver's per-lane columns (wave 0)
  __shared__ uint32_t lds_park[kParkWords * kEnvBlock];            // wave 0's worlds between the steps
  __shared__ gymrl_mlp_desc pd;                                    // the stage table of this workgroup's policy
  __shared__ int running;                                          // the loop's exit word
  float (*lds)[M::kRows * M::kStride] = reinterpret_cast<float (*)[M::kRows * M::kStride]>(dyn_lds);
  float* xin = dyn_lds + M::kBufs * M::kRows * M::kStride;
  float* head = xin + M::kRows * M::kInStride;
  const int tid = threadIdx.x;
  const EpisodeSlot slot(a.E);
  if (tid < d.n_stages) {                                          // (published by the loop's first barrier)
    gymrl_mlp_stage st = d.stage[tid];
    const size_t shift = (size_t)slot.p * (size_t)a.policy_stride;
    st.W += shift;
    if (st.b) st.b += shift;
    pd.stage[tid] = st;
  }
  if (tid == 0) pd.n_stages = d.n_stages;
  const uint32_t vdefer = M::deferrable_stages(d, kEvalActions);   // the critic's stages (0: the network has no such split)
  run_lunar_episodes<kEvalThreads>(a, lds_words, lds_park, running, xin, M::kInStride, slot.p, slot.e0,
                                   logits_policy(head, [&]() { M::forward_tile(pd, lds, xin, head, 0, M::kRows, tid, vdefer); }));
}

// its own function: the tile's ~170 registers and the solver's are allocated separately (as in rollout_lunar.hip)
__device__ __noinline__ void eval_policy_tile_call(const mhc::PolicyArgs& p, mhc::PolicyLds& L, const float* obs_row, float* head) {
  mhc::policy_tile(p, L, obs_row, head, M::kHeadStride, head + kEvalActions, M::kHeadStride, M::kRows);
}

__global__ __launch_bounds__(kEvalThreads) void lunar_eval_mhc_kernel(const gymrl_lunar_eval_args a, const mhc::PolicyArgs p) {
  extern __shared__ __attribute__((aligned(16))) float dyn_lds[];  // (its size keeps one workgroup per CU)
  __shared__ mhc::PolicyLds L;
  __shared__ uint32_t lds_words[kLdsWords * kEnvBlock];
  __shared__ uint32_t lds_park[kParkWords * kEnvBlock];
  __shared__ int running;
  float* xin = dyn_lds;                                            // [16][kXStride] observations
  float* head = xin + M::kRows * kXStride;                         // [16][kHeadStride]: logits 0..3, value 4
  const int tid = threadIdx.x;
  const int prow = 4 * (tid >> 6) + ((tid & 63) >> 4);             // the policy tile's view: this lane's row
  const EpisodeSlot slot(a.E);
  run_lunar_episodes<kEvalThreads>(a, lds_words, lds_park, running, xin, kXStride, slot.p, slot.e0, logits_policy(head, [&]() {
    eval_policy_tile_call(p, L, xin + prow * kXStride, head);
    __syncthreads();                                               // logits -> head[row][0..3]
  }));
}

// the policy must be a 2-output network on the LunarLander observation, logits [4] then value [1]: gymrl_rollout_lunar's rule
bool desc_ok(const gymrl_mlp_desc* policy) {
  int outs = 0, cols = 0;
  if (!policy || policy->n_stages <= 0 || policy->n_stages > GYMRL_MLP_MAX_STAGES) return false;
  for (int s = 0; s < policy->n_stages; ++s) {
    const gymrl_mlp_stage& st = policy->stage[s];
    if (!st.W || st.in_dim <= 0 || st.out_dim <= 0 || st.in_dim > GYMRL_MLP_MAX_WIDTH || st.src < -1 || st.src > 2 ||
        st.dst < -1 || st.dst > 2 || (st.dst >= 0 && (st.dst == st.src || st.out_dim > GYMRL_MLP_MAX_WIDTH)) ||
        (st.src < 0 && st.in_dim != kEvalObs) || st.act < GYMRL_ACT_NONE || st.act > GYMRL_ACT_RELU ||
        (reinterpret_cast<uintptr_t>(st.W) & 15))
      return false;
    if (st.dst < 0) {
      if ((outs == 0 && st.out_dim != kEvalActions) || (outs == 1 && st.out_dim != 1) || outs > 1) return false;
      ++outs; cols += st.out_dim;
    }
  }
  return outs == 2 && cols <= M::kHeadStride;
}

}  // namespace

extern "C" {

size_t gymrl_lunar_eval_args_bytes(void) { return sizeof(gymrl_lunar_eval_args); }

int gymrl_lunar_policy_eval(const gymrl_lunar_eval_args* a, const gymrl_mlp_desc* policy, void* stream) {
  if (!eval_args_ok(a) || !desc_ok(policy)) return -22;
  static bool attr_set = false;
  if (const int rc = set_max_lds_once(attr_set, {(const void*)lunar_eval_kernel}, kDynBytes)) return rc;
  const dim3 grid((unsigned)(a->P * ((a->E + 15) / 16)));
  hipLaunchKernelGGL(lunar_eval_kernel, grid, dim3(kEvalThreads), kDynBytes, (hipStream_t)stream, *a, *policy);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_lunar_mhc_eval(const gymrl_lunar_eval_args* a, const gymrl_mhc_policy* policy, void* stream) {
  if (!eval_args_ok(a) || a->P != 1) return -22;
  mhc::PolicyArgs p{};
  if (const int rc = mhc::policy_fill(p, policy)) return rc;
  if (p.obs_dim != kEvalObs || p.n_act != kEvalActions) return -22;       // LunarLander: 8 observations, 4 actions
  static bool attr_set = false;
  if (const int rc = set_max_lds_once(attr_set, {(const void*)lunar_eval_mhc_kernel}, kDynBytesMhc)) return rc;
  const dim3 grid((unsigned)((a->E + 15) / 16));
  hipLaunchKernelGGL(lunar_eval_mhc_kernel, grid, dim3(kEvalThreads), kDynBytesMhc, (hipStream_t)stream, *a, p);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
