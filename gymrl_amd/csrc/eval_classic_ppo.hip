// eval_classic_ppo.hip — whole evaluation episodes of CartPole-v1, MountainCar-v0 and Acrobot-v1 under a PPO actor-critic,
// P policies x E episodes in ONE launch: gymrl_lunar_policy_eval's contract (eval_lunar.hip) on the classic-control envs.
//
// Replaces the eval() loop of ppo_lunarlander.py:368-399 (get_action(deterministic=True) -> env.step until the episode is over) on
// these envs.  A workgroup carries 16 episodes of one policy from their in-kernel reset to their end and never waits for another
// one.  The loop is eval_episode_device.hpp's run_episodes — the env state, the float64 return and the length live in the
// registers of lanes 0..15 — writing its observations straight into the input tile of mlp_device.hpp's forward_tile, the forward
// the persistent rollout (rollout_classic.hip) acts on.  What is stated here is one step's forward and pick:
//
//   forward   PPO's Linear + Tanh network as gymrl_mlp_forward's stages, all four waves.  The critic is not on the way to an
//             action: its stages are forward_tile's skip mask (deferrable_stages) and are never run.  Policy p reads every W and b
//             p * policy_stride floats behind policy 0's: the workgroup shifts the stage table once, into LDS, and the forward
//             reads it from there.  Weights are re-read from L2 every step.
//   pick      the FIRST maximum of the logits (categorical_pick's deterministic scan, no draw); on Pendulum-v1
//             (gymrl_pendulum_ppo_eval) the actor's mean itself, gaussian_pick's deterministic branch: log_std is not read.
//
// Every arithmetic piece is the device function the step-by-step path launches, so returns, lengths, flags and final observations
// are the loop's bit for bit (tests/test_classic_ppo_eval_gpu.py).
#include <type_traits>
#include "classic_ppo_device.hpp"
#include "eval_episode_device.hpp"

using namespace gymrl;
namespace M = gymrl::mlp;

namespace {

constexpr int kThreads = M::kWaves * 64;
constexpr int kDynFloats = M::kBufs * M::kRows * M::kStride + M::kRows * M::kInStride + M::kRows * M::kHeadStride;
constexpr int kDynBytes = 96 * 1024;       // > 80 KB: one workgroup per CU (as rollout_classic_kernel)
static_assert(kDynFloats * 4 <= kDynBytes, "LDS carve-up");

template <int KIND, class Args>
__global__ __launch_bounds__(kThreads) void classic_ppo_eval_kernel(const Args a, const gymrl_mlp_desc d) {
  constexpr int kActions = ClassicEnv<KIND>::kActions;
  extern __shared__ __attribute__((aligned(16))) float dyn_lds[];
  __shared__ gymrl_mlp_desc pd;                                    // the stage table of this workgroup's policy
  __shared__ int running;                                          // the loop's exit word
  float (*lds)[M::kRows * M::kStride] = reinterpret_cast<float (*)[M::kRows * M::kStride]>(dyn_lds);
  float* xin = dyn_lds + M::kBufs * M::kRows * M::kStride;
  float* head = xin + M::kRows * M::kInStride;
  const int tid = threadIdx.x;
  const slab::EpisodeSlot slot(a.E);
  if (tid < d.n_stages) {                                          // (published by the loop's first barrier)
    gymrl_mlp_stage st = d.stage[tid];
    const size_t shift = (size_t)slot.p * (size_t)a.policy_stride;
    st.W += shift;
    if (st.b) st.b += shift;
    pd.stage[tid] = st;
  }
  if (tid == 0) pd.n_stages = d.n_stages;
  const uint32_t vdefer = M::deferrable_stages(d, kActions);       // the critic's stages (0: the network has no such split)
  slab::run_episodes<KIND>(
      a, xin, M::kInStride, running, slot.p, slot.e0, slot.nrows,
      [&]() { M::forward_tile(pd, lds, xin, head, 0, M::kRows, tid, vdefer); },
      [&](int t) {
        if constexpr (std::is_same<typename EpisodeEnv<KIND>::Action, float>::value) {
          return head[t * M::kHeadStride];                         // a = mu
        } else {
          float z[kActions], lp, H;
#pragma unroll
          for (int k = 0; k < kActions; ++k) z[k] = head[t * M::kHeadStride + k];
          return categorical_pick<kActions>(z, nullptr, 0ull, 0ull, 0ull, 1, lp, H);
        }
      });
}

// What the entry point refuses, before the first HIP call: the sizes, the stride, the streams, the outputs and their alignment
template <class Args>
bool eval_args_ok(const Args* a, int max_cap) {
  if (!a || !a->returns || !a->lengths || !a->terminated) return false;
  if (a->P < 1 || a->E < 1 || a->cap < 1 || a->cap > max_cap || a->stream_id0 < 0) return false;
  if ((int64_t)a->P * a->E > 0x7fffffffLL) return false;
  if (a->policy_stride < 0 || (a->policy_stride & 3) != 0 || (a->policy_stride == 0 && a->P != 1)) return false;
  // final_obs rows: whole float2 for the even widths, Pendulum-v1's 12-byte rows are scalar stores
  return slab::aligned(a->returns, 8) && slab::aligned(a->lengths, 4) &&
         slab::aligned(a->final_obs, std::is_same<Args, gymrl_pendulum_ppo_eval_args>::value ? 4 : 8);
}

template <int KIND, class Args>
int eval_launch(const Args* a, const gymrl_mlp_desc* policy, void* stream) {
  using Env = ClassicEnv<KIND>;
  if (!eval_args_ok(a, Env::kMaxSteps) || !ppo_desc_ok(policy, Env::kObs, Env::kActions)) return -22;
  static bool attr_set = false;
  if (const int rc = set_max_lds_once(attr_set, {(const void*)classic_ppo_eval_kernel<KIND, Args>}, kDynBytes)) return rc;
  const dim3 grid((unsigned)(a->P * ((a->E + 15) / 16)));
  hipLaunchKernelGGL((classic_ppo_eval_kernel<KIND, Args>), grid, dim3(kThreads), kDynBytes, (hipStream_t)stream, *a, *policy);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" {

size_t gymrl_classic_ppo_eval_args_bytes(void) { return sizeof(gymrl_classic_ppo_eval_args); }

int gymrl_classic_ppo_eval(const gymrl_classic_ppo_eval_args* a, const gymrl_mlp_desc* policy, void* stream) {
  if (!a) return -22;
  switch (a->env_kind) {
    case GYMRL_ENV_CARTPOLE: return eval_launch<GYMRL_ENV_CARTPOLE>(a, policy, stream);
    case GYMRL_ENV_MOUNTAINCAR: return eval_launch<GYMRL_ENV_MOUNTAINCAR>(a, policy, stream);
    case GYMRL_ENV_ACROBOT: return eval_launch<GYMRL_ENV_ACROBOT>(a, policy, stream);
    default: return -22;
  }
}

size_t gymrl_pendulum_ppo_eval_args_bytes(void) { return sizeof(gymrl_pendulum_ppo_eval_args); }

int gymrl_pendulum_ppo_eval(const gymrl_pendulum_ppo_eval_args* a, const gymrl_mlp_desc* policy, void* stream) {
  return eval_launch<GYMRL_ENV_PENDULUM>(a, policy, stream);
}

}  // extern "C"
