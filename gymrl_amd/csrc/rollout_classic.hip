// rollout_classic.hip — PPO's collect_rollout (ppo_lunarlander.py:198-231) for CartPole-v1, MountainCar-v0 and Acrobot-v1 as ONE
// persistent launch per chunk of vector steps: rollout_lunar.hip's scheme with the classic-control stepper in place of the Box2D one.
//
// Step by step, a classic-control vector step is the policy forward + the sample kernel + the env's step kernel: three launches
// of a few microseconds of work each, i.e. the launch floor.  Nothing couples two workgroups inside a rollout (frozen
// weights, independent envs), so a workgroup owns its 16 envs for `nsteps` steps: all four waves run the policy forward of
// the 16 observations (mlp_device.hpp: f32 MFMA, logits and value stay in LDS), then lanes 0..15 of wave 0 fold step
// t-1 into its GAE chunk map, draw the action (policy_device.hpp: the Philox keys / explicit noise of
// gymrl_categorical_sample), step their env (env_classic_device.hpp: the arithmetic of gymrl_env_step), write the slab
// rows and put the next observation into the forward's LDS input.  Every arithmetic piece is the device function the
// step-by-step path launches: the slab is bit-identical to collect_rollout() without this kernel
// (tests/test_hip_parity.py::test_persistent_rollout_cartpole_bit_identical_to_stepwise, tests/test_rollout_classic_gpu.py).
//
// The kernel is ONE template over classic_ppo_device.hpp's ClassicEnv<KIND>: the observation width, the action count, the state
// view, the step function and the vector an observation row is stored with are the env's, everything else is shared.
//
// Pendulum-v1 (gymrl_rollout_pendulum) is the fourth instance: its argument block is gymrl_rollout_pendulum_args, its action is
// the env's float torque and its pick is gauss_policy_device.hpp's gaussian_pick<1> on the actor's mean, the
// UNCLIPPED draw goes into the float action slab, and the stored reward is the env's times reward_scale (one float32 multiply).
#include <type_traits>
#include "classic_ppo_device.hpp"
#include "policy_device.hpp"
#include "gauss_policy_device.hpp"

using namespace gymrl;
namespace M = gymrl::mlp;

namespace {

constexpr int kThreads = M::kWaves * 64;
constexpr int kGaeChunk = 16;        // == gymrl_gae_chunk() (gae.hip kBlkTC)
constexpr int kDynFloats = M::kBufs * M::kRows * M::kStride + M::kRows * M::kInStride + M::kRows * M::kHeadStride;
constexpr int kDynBytes = 96 * 1024; // > 80 KB: one workgroup per CU (as mlp_forward_kernel)
static_assert(kDynFloats * 4 <= kDynBytes, "LDS carve-up");

template <int KIND, class Args>
__global__ __launch_bounds__(kThreads) void rollout_classic_kernel(Args a, gymrl_mlp_desc d) {
  using Env = ClassicEnv<KIND>;
  using ObsVec = typename Env::ObsVec;
  constexpr int kObs = Env::kObs, kActions = Env::kActions;
  constexpr int kObsVecs = kObs * (int)sizeof(float) / (int)sizeof(ObsVec);
  static_assert(kObsVecs * sizeof(ObsVec) == kObs * sizeof(float), "an observation row is whole store vectors");
  extern __shared__ __attribute__((aligned(16))) float dyn_lds[];
  float (*lds)[M::kRows * M::kStride] = reinterpret_cast<float (*)[M::kRows * M::kStride]>(dyn_lds);
  float* xin = dyn_lds + M::kBufs * M::kRows * M::kStride;
  float* head = xin + M::kRows * M::kInStride;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int N = a.n_envs, T = a.T;
  const int m0 = blockIdx.x * M::kRows;
  const int t_end = a.t0 + a.nsteps;
  const int row = lane, i = m0 + row;                              // wave 0's view: one lane per env (lanes 0..15)
  const bool valid = row < M::kRows && i < N;
  const typename Env::State st(a.env_state, N);
  const double gl = (double)(float)(a.gamma * a.lam);              // NEP-50 float32 decay (see gae.hip)

  for (int e = tid; e < M::kRows * M::kInStride; e += kThreads) xin[e] = 0.0f;
  __syncthreads();
  for (int e = tid; e < M::kRows * kObs; e += kThreads) {
    const int r = e / kObs, c = e - r * kObs;
    if (m0 + r < N) xin[r * M::kInStride + c] = a.obs[((size_t)a.t0 * N + m0 + r) * kObs + c];
  }
  for (int t = a.t0; t <= t_end; ++t) {
    const bool tail = t == t_end;                   // only the bootstrap value of the finished rollout is left
    if (tail && t_end != T) break;
    __syncthreads();                                // xin of step t is complete
    M::forward_tile(d, lds, xin, head, m0, N, tid, 0u);
    __syncthreads();                                // logits / value of the 16 rows are in `head`
    if (wave == 0) {
      ClassicStep<kObs> r;
      r.done = false; r.ret = 0.0; r.len = 0;
      if (valid) {
        const float v = head[row * M::kHeadStride + kActions];
        if (a.gae_running && t > 0) {               // V_t completes step t-1's delta
          const int tp = t - 1;
          const size_t o = (size_t)tp * N + i;
          double2* agg = reinterpret_cast<double2*>(a.gae_workspace) + (size_t)(tp / kGaeChunk) * N;
          gae_online_compose(a.rew[o], a.done[o], a.val[o], v, a.gamma, gl, (tp % kGaeChunk) == 0,
                             (tp % kGaeChunk) == kGaeChunk - 1 || tp == T - 1, a.gae_running, agg, N, i);
        }
        if (tail) a.next_value[i] = v;
        else {
          const size_t o = (size_t)t * N + i;
          a.val[o] = v;
          float z[kActions], lp, H;
#pragma unroll
          for (int k = 0; k < kActions; ++k) z[k] = head[row * M::kHeadStride + k];
          if constexpr (std::is_same<Args, gymrl_rollout_pendulum_args>::value) {   // N(mu, exp(log_std)): gymrl_gaussian_sample's bits
            float act[kActions];
            gaussian_pick<kActions>(z, a.log_std, a.noise_normal ? a.noise_normal + o * kActions : nullptr, a.seed,
                                    (uint64_t)(a.env_id0 + i), a.counter0 + (uint64_t)t, 0, act, lp, H);
            a.act[o] = act[0]; a.logp[o] = lp;
            Env::step(st, i, a.seed, a.env_id0, act[0], r);
            a.rew[o] = r.reward * a.reward_scale;
          } else {                                                                  // Categorical(logits): gymrl_categorical_sample's
            const int act = categorical_pick<kActions>(z, a.noise_exp ? a.noise_exp + o * kActions : nullptr, a.seed,
                                                       (uint64_t)(a.env_id0 + i), a.counter0 + (uint64_t)t, 0, lp, H);
            a.act[o] = act; a.logp[o] = lp;
            Env::step(st, i, a.seed, a.env_id0, act, r);
            a.rew[o] = r.reward;
          }
          a.done[o] = r.done;
          if (a.ep_ret && r.done) a.ep_ret[o] = (float)r.ret;
          float* on = a.obs + ((size_t)(t + 1) * N + i) * kObs;
          if constexpr (kObsVecs == 1 && sizeof(ObsVec) == 16) {
            reinterpret_cast<float4*>(on)[0] = make_float4(r.o_next[0], r.o_next[1], r.o_next[2], r.o_next[3]);
          } else if constexpr (sizeof(ObsVec) == 4) {
#pragma unroll
            for (int k = 0; k < kObsVecs; ++k) on[k] = r.o_next[k];
          } else {
#pragma unroll
            for (int k = 0; k < kObsVecs; ++k) reinterpret_cast<float2*>(on)[k] = make_float2(r.o_next[2 * k], r.o_next[2 * k + 1]);
          }
#pragma unroll
          for (int k = 0; k < kObs; ++k) xin[row * M::kInStride + k] = r.o_next[k];     // next policy input: the forward's LDS tile
        }
      }
      if (!tail) accumulate_ep_stats(a.ep_stats, r.done && valid, r.ret, r.len);
    }
    if (tail) break;
  }
}

// what every kind's entry refuses alike, before any launch: the slabs, the step window, the GAE pair, the row's alignment, the policy
template <int KIND, class Args>
bool rollout_args_ok(const Args* a, const gymrl_mlp_desc* policy) {
  using Env = ClassicEnv<KIND>;
  if (!a || !policy || !a->env_state || !a->obs || !a->act || !a->logp || !a->val || !a->rew || !a->done ||
      !a->next_value || a->n_envs <= 0 || a->T <= 0 || a->t0 < 0 || a->nsteps < 0 || a->t0 + a->nsteps > a->T)
    return false;
  if (a->gae_running && !a->gae_workspace) return false;
  if constexpr (std::is_same<Args, gymrl_rollout_pendulum_args>::value) {
    if (!a->log_std || !(a->reward_scale == a->reward_scale)) return false;
    if ((reinterpret_cast<uintptr_t>(a->act) | reinterpret_cast<uintptr_t>(a->log_std) | reinterpret_cast<uintptr_t>(a->noise_normal)) & 3) return false;
  }
  if (reinterpret_cast<uintptr_t>(a->obs) & (sizeof(typename Env::ObsVec) - 1)) return false;
  return ppo_desc_ok(policy, Env::kObs, Env::kActions);
}

template <int KIND, class Args>
int rollout_launch(const Args* a, const gymrl_mlp_desc* policy, void* stream) {
  if (!rollout_args_ok<KIND>(a, policy)) return -22;
  if (a->nsteps == 0 && a->t0 != a->T) return 0;
  static bool attr_set = false;
  if (const int rc = set_max_lds_once(attr_set, {(const void*)rollout_classic_kernel<KIND, Args>}, kDynBytes)) return rc;
  const int blocks = (a->n_envs + M::kRows - 1) / M::kRows;
  hipLaunchKernelGGL((rollout_classic_kernel<KIND, Args>), dim3(blocks), dim3(kThreads), kDynBytes, (hipStream_t)stream, *a, *policy);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" {

int gymrl_rollout_cartpole(const gymrl_rollout_lunar_args* a, const gymrl_mlp_desc* policy, void* stream) {
  return rollout_launch<GYMRL_ENV_CARTPOLE>(a, policy, stream);
}

int gymrl_rollout_classic(int env_kind, const gymrl_rollout_lunar_args* a, const gymrl_mlp_desc* policy, void* stream) {
  switch (env_kind) {
    case GYMRL_ENV_CARTPOLE: return rollout_launch<GYMRL_ENV_CARTPOLE>(a, policy, stream);
    case GYMRL_ENV_MOUNTAINCAR: return rollout_launch<GYMRL_ENV_MOUNTAINCAR>(a, policy, stream);
    case GYMRL_ENV_ACROBOT: return rollout_launch<GYMRL_ENV_ACROBOT>(a, policy, stream);
    default: return -22;
  }
}

size_t gymrl_rollout_pendulum_args_bytes(void) { return sizeof(gymrl_rollout_pendulum_args); }

int gymrl_rollout_pendulum(const gymrl_rollout_pendulum_args* a, const gymrl_mlp_desc* policy, void* stream) {
  return rollout_launch<GYMRL_ENV_PENDULUM>(a, policy, stream);
}

}  // extern "C"
