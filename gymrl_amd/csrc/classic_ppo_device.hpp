// classic_ppo_device.hpp — what PPO's one-launch kernels on the classic-control envs share: rollout_classic.hip (the persistent
// rollout) and eval_classic_ppo.hip (whole evaluation episodes) are templates over ClassicEnv<KIND>, and both entry points refuse
// the same policy descriptors.
//
//   ClassicEnv<KIND>   (env_classic_device.hpp, which the DQN-family act kernels read it from as well) CartPole-v1, MountainCar-v0,
//                      Acrobot-v1: the widths and the TimeLimit, the view of the env state buffer, ONE env's step with auto-reset, and
//                      the vector an observation row of the slab is stored with.
//   ppo_desc_ok        the policy is gymrl_mlp_forward's stage table on the env's observation: logits [A] then value [1] as its
//                      two dst == -1 stages.
#pragma once
#include "env_classic_device.hpp"
#include "mlp_device.hpp"

namespace gymrl {
namespace {

// the policy must be a 2-output network on the env's observation: logits [n_act] then value [1]
inline bool ppo_desc_ok(const gymrl_mlp_desc* policy, int n_obs, int n_act) {
  int outs = 0, cols = 0;
  if (!policy || policy->n_stages <= 0 || policy->n_stages > GYMRL_MLP_MAX_STAGES) return false;
  for (int s = 0; s < policy->n_stages; ++s) {
    const gymrl_mlp_stage& st = policy->stage[s];
    if (!st.W || st.in_dim <= 0 || st.out_dim <= 0 || st.in_dim > GYMRL_MLP_MAX_WIDTH || st.src < -1 || st.src > 2 ||
        st.dst < -1 || st.dst > 2 || (st.dst >= 0 && (st.dst == st.src || st.out_dim > GYMRL_MLP_MAX_WIDTH)) ||
        (st.src < 0 && st.in_dim != n_obs) || st.act < GYMRL_ACT_NONE || st.act > GYMRL_ACT_RELU ||
        (reinterpret_cast<uintptr_t>(st.W) & 15))
      return false;
    if (st.dst < 0) {
      if ((outs == 0 && st.out_dim != n_act) || (outs == 1 && st.out_dim != 1) || outs > 1) return false;
      ++outs; cols += st.out_dim;
    }
  }
  return outs == 2 && cols <= mlp::kHeadStride;
}

}  // namespace
}  // namespace gymrl
