/*
 * gymrl.h — C-ABI of libgymrl_hip.so: the MI355X (gfx950) vectorised-rollout +
 * PPO/DQN/SAC learner hot path that sits behind the Config / Trainer surface of
 * Starlight0798/gymRL's algorithms/<algo>_<env>.py scripts.
 *
 * The reference has no FFI of its own (pure Python); every entry point below
 * cites the reference function (file:line under the gymRL tree) whose arithmetic
 * it replaces.  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes; no torch / C++ types.
 *   - every data pointer is a DEVICE pointer (HBM) unless the name ends in _host.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - return 0 on success, -EINVAL (-22) on a bad argument, -(hipError_t) - 1000
 *     when a launch fails.  Nothing allocates, nothing synchronises, nothing
 *     copies to the host: the caller owns every buffer.  Safe to capture in a
 *     hipGraph.
 *   - layouts are time-major SoA slabs: x[T][N] (t outer, env inner) so that a
 *     wavefront's 64 lanes (= 64 env instances) touch 64 consecutive words.
 */
#ifndef GYMRL_H
#define GYMRL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GYMRL_ABI_VERSION 4   /* 2: round-2 signature changes (adam_step, per_*, replay_append, nstep_push, gae_decoupled, rollout descriptors); gymrl_gemm_config left the product library
                               * 3: gymrl_rollout_lunar_args grew `gae_carry` (round 6), gymrl_gae variant 3
                               * 4: the entry point that ran a SAC vector step as ONE launch was removed (five launches are the only form) */

/* ---------------------------------------------------------------- misc --- */
int gymrl_abi_version(void);
/* 1 when a gfx950 device is visible to the HIP runtime, else 0. */
int gymrl_device_ok(void);

/* ------------------------------------------------------------- env kinds -- */
enum {
  GYMRL_ENV_CARTPOLE    = 0, /* CartPole-v1   obs 4, 2 discrete actions   */
  GYMRL_ENV_PENDULUM    = 1, /* Pendulum-v1   obs 3, 1 continuous in [-2,2] */
  GYMRL_ENV_LUNARLANDER = 2, /* LunarLander-v3 obs 8, 4 discrete actions  */
  GYMRL_ENV_MOUNTAINCAR = 3, /* MountainCar-v0 obs 2, 3 discrete actions (the steppers, gymrl_mountaincar_rule_eval and
                              * gymrl_mountaincar_net_eval only: the fused acting, ring and rollout kernels and the other
                              * policy-episode entry points refuse it with -EINVAL) */
  /* 4 is left free for MountainCar's continuous sibling (MountainCarContinuous-v0, not built): every entry point refuses it */
  GYMRL_ENV_ACROBOT     = 5  /* Acrobot-v1 obs 6, 3 discrete actions (the steppers and gymrl_acrobot_net_eval only, like kind 3) */
};
#define GYMRL_ACROBOT_WRAP_TRIPS 8   /* Acrobot-v1: trips of each angle-wrapping loop (the rule below) */

/*
 * Batched env stepper.  Replaces gym.make / env.reset / env.step as used by
 * ppo_lunarlander.py:160,200,211,222  dqn_cartpole.py:94,176,181
 * rainbow_dqn_cartpole.py:270,369,373  sac_pendulum.py:154,275,281
 * utils/runner.py:53,111,123  mountaincar_baseline.py:29,53,60.
 * One env instance per lane; state is a caller-owned SoA byte buffer of
 * gymrl_env_state_bytes(kind, n_envs) bytes (256-B aligned base required).
 * Classic envs: consecutive fields [n_envs], each field's byte size rounded up to a multiple of 256 —
 *   CartPole-v1  f64 x, f64 x_dot, f64 theta, f64 theta_dot, f64 ep_ret, i32 ep_len, u32 episode
 *   Pendulum-v1  f64 theta, f64 theta_dot, f64 ep_ret, i32 ep_len, u32 episode
 *   MountainCar-v0  f64 position, f64 velocity, f64 ep_ret, i32 ep_len, u32 episode
 *   Acrobot-v1   f64 theta1, f64 theta2, f64 dtheta1, f64 dtheta2, f64 ep_ret, i32 ep_len, u32 episode
 * (float64 like gymnasium's own state; tests/test_classic_micro_gpu.py writes states through this layout, and a
 * checkpoint of a running vector is a copy of the buffer).  LunarLander: 144 dwords per env, word-major.
 */

/*
 * Acrobot-v1, the rule (gymnasium is no dependency of this library: what follows is the specification, after gymnasium's published
 * AcrobotEnv in its "book" variant with torque_noise_max = 0).  Everything is IEEE float64, no operation is contracted into an
 * fma, sin / cos are csrc/gymrl_device.hpp's det_sincos, and an expression is evaluated left to right in exactly the grouping
 * written here, so that a host restatement (tests/acrobot_ref.py) reproduces every bit.
 *   state   y = (th1, th2, dth1, dth2);  torque a = (double)(action - 1), action in {0, 1, 2}
 *   f(y; a) (m1 = m2 = l1 = I1 = I2 = 1, lc1 = lc2 = 0.5, g = 9.8 multiplied out; 14.7 stands for the double 1.5 * 9.8):
 *     s2 = sin(th2), c2 = cos(th2), c12 = cos((th1 + th2) - pi / 2), c1 = cos(th1 - pi / 2)
 *     d1    = ((0.25 + (1.25 + c2)) + 1.0) + 1.0
 *     d2    = (0.25 + 0.5 * c2) + 1.0
 *     phi2  = 4.9 * c12
 *     phi1  = ((((-0.5 * (dth2 * dth2)) * s2) - ((dth2 * dth1) * s2)) + 14.7 * c1) + phi2
 *     ddth2 = (((a + (d2 / d1) * phi1) - ((0.5 * (dth1 * dth1)) * s2)) - phi2) / (1.25 - (d2 * d2) / d1)
 *     ddth1 = (-(d2 * ddth2 + phi1)) / d1
 *     f     = (dth1, dth2, ddth1, ddth2)
 *   step    one classical RK4 step over dt = 0.2, per component:
 *     k1 = f(y), k2 = f(y + 0.1 * k1), k3 = f(y + 0.1 * k2), k4 = f(y + 0.2 * k3)
 *     y' = y + (0.2 / 6.0) * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)
 *   then    th1, th2: GYMRL_ACROBOT_WRAP_TRIPS times `x = x > pi ? x - 2.0 * pi : x`, then as many times
 *           `x = x < -pi ? x + 2.0 * pi : x` — gymnasium's two while loops with a fixed trip count: from a state inside the
 *           velocity box an angle moves by less than 9 pi in a step (at the box's corners), so five trips do
 *           (tests/test_acrobot_ref.py); an angle handed in through `start` more than 16 pi outside stays outside.  dth1 is clamped to +-4.0 * pi, dth2 to
 *           +-9.0 * pi (x < lo ? lo : x > hi ? hi : x).
 *   end     terminated = ((-cos(th1)) - cos(th2 + th1)) > 1.0 on the new state; reward -1, and 0 on the terminating step;
 *           TimeLimit 500 (truncated = length >= 500).
 *   obs     the float32 casts of (cos th1, sin th1, cos th2, sin th2, dth1, dth2)
 *   reset   y[k] = -0.1 + 0.2 * u_k, the four u_k taken from the Philox words exactly as CartPole-v1's reset takes them (two
 *           calls, RNG_ENV_RESET | 0 and | 1).  gymnasium rounds the reset state to float32; like CartPole-v1's, that rounding
 *           is deliberately not modelled.
 */
int    gymrl_env_obs_dim(int kind);
int    gymrl_env_act_dim(int kind);     /* #discrete actions, or continuous dim */
int    gymrl_env_is_discrete(int kind);
int    gymrl_env_max_steps(int kind);   /* TimeLimit: 500 / 200 / 1000 / 200 / (kind 5) 500 */
size_t gymrl_env_state_bytes(int kind, int n_envs);

/* (Re)initialise every env: episode counter := 0, draws from the counter-based
 * Philox stream keyed by (seed, env_id0 + lane, episode).  obs_out [N, obs_dim]. */
int gymrl_env_reset(int kind, void* state, int n_envs, uint64_t seed,
                    int64_t env_id0, float* obs_out, void* stream);

/* One vector step with auto-reset.
 *   action        i32[N] (discrete) or f32[N, act_dim] (continuous)
 *   obs_out       f32[N, obs]  observation the policy sees next (post-reset
 *                 where done — ppo_lunarlander.py:220-223)
 *   term_obs_out  f32[N, obs] or NULL: pre-reset observation (what off-policy
 *                 buffers store as next_state — dqn_cartpole.py:183)
 *   rew_out       f32[N]
 *   terminated_out / truncated_out  u8[N]  (rainbow_dqn_cartpole.py:376 needs both)
 *   done_out      u8[N] or NULL  = terminated | truncated (ppo_lunarlander.py:212)
 *   ep_ret_out    f32[N] or NULL: finished episode's return where done, else unchanged
 *   ep_len_out    i32[N] or NULL: finished episode's length where done
 *   ep_stats      f64[3] or NULL: += (#finished episodes, sum of returns, sum of lengths)
 */
int gymrl_env_step(int kind, void* state, int n_envs, uint64_t seed, int64_t env_id0,
                   const void* action, float* obs_out, float* term_obs_out,
                   float* rew_out, uint8_t* terminated_out, uint8_t* truncated_out,
                   uint8_t* done_out, float* ep_ret_out, int32_t* ep_len_out,
                   double* ep_stats, void* stream);

/* Episodes a trainer abandons at its own step cap below the env's TimeLimit — `for step in range(cfg.max_steps)`
 * of dqn_cartpole.py:178, sac_pendulum.py:278 (no done flag is stored; the next loop turn calls env.reset()).
 * Call after gymrl_env_step: every env whose running episode has reached `cap` steps starts its next episode;
 * obs_inout [N, obs] rows of those envs become the reset observation, flag_inout u8[N] (or NULL) is OR-ed with 1
 * for them, ep_ret_out / ep_len_out / ep_stats receive the abandoned episode as gymrl_env_step would for a
 * finished one.  CartPole-v1, Pendulum-v1, MountainCar-v0 and Acrobot-v1 (no reference off-policy script runs LunarLander: -EINVAL). */
int gymrl_env_abandon(int kind, void* state, int n_envs, uint64_t seed, int64_t env_id0, int cap,
                      float* obs_inout, uint8_t* flag_inout, float* ep_ret_out, int32_t* ep_len_out,
                      double* ep_stats, void* stream);

/* Optional latency hiding for expensive resets (LunarLander's reset() ends with a full
 * physics step): prepares, for every env that lacks one, the post-reset world of its NEXT
 * episode in a spare slot of `state`; gymrl_env_step then swaps it in when the episode ends
 * instead of running the reset inside the step.  Results are bit-identical with or without
 * it.  Intended for a side stream (it may overlap later gymrl_env_step calls on the same
 * state); a no-op for CartPole / Pendulum / MountainCar / Acrobot. */
int gymrl_env_refill(int kind, void* state, int n_envs, uint64_t seed, int64_t env_id0,
                     void* stream);

/* -------------------------------------------------- categorical policy ---- */
/*
 * Categorical(logits).sample()/log_prob/entropy — ppo_lunarlander.py:92-104.
 * sample == argmax_k(softmax(z)_k / q_k), q ~ Exp(1)  (torch.multinomial's CPU
 * path).  noise_exp f32[N,A] supplies q explicitly (parity
 * mode); when NULL q is drawn in-kernel from Philox(seed, counter, env).
 * deterministic != 0 -> action = argmax(z) (ppo_lunarlander.py:98-99).
 * value_in f32[N] (may be NULL) is copied to value_out so the rollout slab row
 * is written by one kernel.  A <= 8.
 */
/* Optional producer-side fusion of GAE's chunk reduction (see gymrl_gae variant 2): while
 * sampling step t the kernel also composes step t-1 — whose delta needs V_t = value_in —
 * into the affine map of its time chunk.  All pointers are rows of the rollout slab. */
typedef struct {
  const float* rew_prev;      /* f32[N] rewards of step t-1                         */
  const uint8_t* done_prev;   /* u8[N]  done flags of step t-1                      */
  const float* val_prev;      /* f32[N] values of step t-1                          */
  double* running;            /* f64[2][N] map of the chunk being composed (scratch) */
  void* gae_workspace;        /* the workspace later handed to gymrl_gae(variant 2)  */
  int t_prev;                 /* t-1, 0-based                                        */
  int T;                      /* rollout length                                      */
  double gamma, lam;
  double lam2;                /* > 0 with running2 != NULL: decoupled-lambda mode (G3) — `lam` is lam_actor,   */
  double* running2;           /* `lam2` lam_critic; both decay factors are the float64 products gamma * lam;   */
                              /* the critic's chunk maps follow the actor's in the workspace of                */
                              /* gymrl_gae_decoupled(variant 2); running2 f64[2][N] scratch                    */
} gymrl_gae_online;

int gymrl_categorical_sample(const float* logits, const float* value_in,
                             const float* noise_exp, uint64_t seed, uint64_t counter,
                             int64_t env_id0, int n, int n_actions, int deterministic,
                             int32_t* act_out, float* logp_out, float* ent_out,
                             float* value_out, const gymrl_gae_online* online, void* stream);
/*
 * Gaussian policy — the diagonal-Gaussian head PPO uses on a continuous action (gymrl_amd/ppo_pendulum.py).  The reference tree
 * has no continuous-action PPO script: this rule is the project's own, restated on the host in tests/gauss_policy_ref.py
 * (float32 throughout, no contraction into fma, the grouping as written, every sum over k ascending from 0.0f).
 *   network   ActorCritic(state_dim, A): the actor's last layer is the mean mu[A], not squashed; log_std f32[A] is a
 *             state-independent parameter vector in device memory; the critic is the categorical head's.
 *   draw      eps_k ~ N(0, 1): Philox4x32-10 keyed as gymrl_categorical_sample keys its words — key = seed, counter words
 *             (env id low, env id high, counter low, RNG_POLICY | (counter high & 0x3FFFFF) << 2 | block) — with block = k / 2;
 *             words (x, y) give eps_{2 block}, (z, w) give eps_{2 block + 1}, each by Box-Muller:
 *             u1 = ((w0 >> 8) + 1) * 2^-24, u2 = (w1 >> 8) * 2^-24, eps = sqrtf(-2.0f * det_logf(u1)) * det_cosf(6.2831855f * u2).
 *             noise_normal f32[...][A] replaces the draw when given (parity mode, as noise_exp is for the categorical).
 *             a_k = mu_k + det_expf(log_std_k) * eps_k.  deterministic != 0: a = mu, eps = 0.
 *             The action is NOT clipped: the slab holds the draw, the env clips the torque it applies.
 *   logp      at the draw: sum_k ((-0.5f * (eps_k * eps_k) - log_std_k) - 0.918938533f)
 *             at the update, for a stored action a: the same with z_k = (a_k - mu_k) * det_expf(-log_std_k) in place of eps_k
 *   entropy   sum_k (1.418938533f + log_std_k)
 *   loss      gymrl_ppo_loss_fwd_bwd's terms, clip / dual-clip and tie rules, metrics and gymrl_ppo_cfg with this logp / entropy;
 *             with g_lp = dL/dlogp and g_H = -entropy_coef / B of a row:
 *             dmu_k = g_lp * (z_k * det_expf(-log_std_k)),  dvalue as L1,
 *             dlog_std_k = sum over rows of (g_lp * (z_k * z_k - 1.0f) + g_H), each row's float32 term added in float64.
 *   update    the two MLPs through torch autograd around gymrl_ppo_gauss_loss_fwd_bwd, or the hand-scheduled minibatch of
 *             ppo_net.FusedGaussianUpdate with the heads, this loss and dlog_std as ONE pass over the pre-activations:
 *             gymrl_gauss_heads_loss_fwd_bwd below (A == 1, gated by gymrl_ppo_gauss_update_shape_ok); the same row arithmetic.
 *
 * gymrl_gaussian_sample: mu f32[N, A], log_std f32[A], value_in f32[N] or NULL (copied to value_out), noise_normal f32[N, A] or
 * NULL -> act_out f32[N, A], logp_out f32[N], ent_out f32[N] or NULL.  `online`: gymrl_categorical_sample's producer side of GAE
 * (the same composition; the decoupled-lambda pair running2 / lam2 is refused).  1 <= A <= 8.
 */
int gymrl_gaussian_sample(const float* mu, const float* log_std, const float* value_in,
                          const float* noise_normal, uint64_t seed, uint64_t counter,
                          int64_t env_id0, int n, int act_dim, int deterministic,
                          float* act_out, float* logp_out, float* ent_out,
                          float* value_out, const gymrl_gae_online* online, void* stream);
/* Last step of a rollout: composes step T-1 with val_cur = the bootstrap value V_T. */
int gymrl_gae_online_flush(const gymrl_gae_online* online, const float* val_cur, int N,
                           void* stream);
int gymrl_gae_chunk(void);   /* time-chunk length of the blocked GAE (16) */

/* ------------------------------------------------------------------ GAE --- */
/*
 * G1: PPOTrainer.compute_gae — ppo_lunarlander.py:179-196.
 *   delta_t = r_t + g*V_{t+1}*(1-d_t) - V_t ; A_t = delta_t + g*l*(1-d_t)*A_{t+1}
 *   V_T = next_val ; ret = A + V.   float64 recursion, float32 storage.
 * rew,val f32[T][N]; done u8[T][N]; next_val f32[N]; adv_out, ret_out f32[T][N].
 * moments_out f64[3] or NULL: = (count, sum A, sum A^2) over the float64
 * advantages (feeds the whole-rollout normalisation of ppo_lunarlander.py:236);
 * reduced in a fixed order (no float atomics) so training is reproducible.
 * variant 0 = one lane walks one env sequentially (reference operation order);
 * variant 1 = time-blocked affine scan (roofline variant; needs N % 4 == 0 and
 *             16-B aligned rows, else it falls back to variant 0);
 * variant 2 = variant 1 without its first pass: the per-chunk maps were composed during
 *             the rollout (gymrl_gae_online in gymrl_categorical_sample + _flush), so the
 *             launch reads r, v, d once (17 -> ~19 HBM bytes per transition instead of 29).
 * variant 3 = variant 2 without its carry launch: the persistent rollout ran the carry pass for its own envs
 *             at its tail (gymrl_rollout_lunar_args.gae_carry) — the apply launch (+ the moments' fold) alone;
 *             the carries, and so every advantage, have variant 2's bits.
 * workspace: gymrl_gae_workspace_bytes(T, N) bytes, 256-B aligned; required for
 * variant 1 or when moments_out != NULL.
 */
size_t gymrl_gae_workspace_bytes(int T, int N);
int gymrl_gae(const float* rew, const float* val, const uint8_t* done,
              const float* next_val, int T, int N, double gamma, double lam,
              float* adv_out, float* ret_out, double* moments_out,
              int variant, void* workspace, void* stream);

/* G2: ReplayBuffer_on_policy.compute_advantage — utils/buffer.py:21-35
 * (== ppo_rnn_lunarlander.py:187-204): stored next values, separate dw
 * (terminated) and done masks, float32 recursion.  All arrays [T][N]. */
int gymrl_gae_dw(const float* rew, const float* val, const float* next_val,
                 const uint8_t* done, const uint8_t* dw, int T, int N,
                 double gamma, double lam, float* adv_out, float* vtarget_out,
                 double* moments_out, void* workspace, void* stream);

/* G3: ppo_full compute_advantages — ppo_full_lunarlander.py:507-535: two scans
 * sharing delta (lam_actor, lam_critic); ret = adv_critic + V; adv_actor raw.
 * variant 0 = one lane walks one env sequentially (the reference's operation order);
 * variant 1 = time-blocked affine scan with two (A, b) maps per chunk (same layout rules as gymrl_gae variant 1,
 *             falls back to variant 0 when they do not hold);
 * variant 2 = variant 1 without its first pass: both chunk maps were composed during the rollout
 *             (gymrl_gae_online with lam2 / running2).
 * workspace: gymrl_gae_decoupled_workspace_bytes(T, N) bytes, 256-B aligned (variants 1, 2; NULL: variant 0). */
size_t gymrl_gae_decoupled_workspace_bytes(int T, int N);
int gymrl_gae_decoupled(const float* rew, const float* val, const uint8_t* done,
                        const float* next_val, int T, int N, double gamma,
                        double lam_actor, double lam_critic, float* adv_actor_out,
                        float* ret_out, int variant, void* workspace, void* stream);

/* Whole-rollout advantage normalisation — ppo_lunarlander.py:236 (ddof 0) and
 * utils/buffer.py:33 (ddof 1).  moments f64[3] = (count, sum, sumsq) on device.
 * x <- (x - mean) / (std + eps), f64 arithmetic, f32 storage. */
size_t gymrl_reduce_workspace_bytes(void);
int gymrl_moments(const float* x, int64_t n, double* moments_out, void* workspace,
                  void* stream);
int gymrl_normalize(float* x, int64_t n, const double* moments, int ddof,
                    double eps, void* stream);

/* ------------------------------------------------------------- PPO loss --- */
typedef struct {
  float clip_eps;     /* ppo_lunarlander.py:41  (0.2)  */
  float dual_clip;    /* :42 (3.0)                     */
  float value_coef;   /* :44 (0.5)                     */
  float entropy_coef; /* :43 (0.01)                    */
} gymrl_ppo_cfg;

/*
 * L1+L2: evaluate_actions + clipped/dual-clip surrogate + value + entropy loss,
 * forward AND backward w.r.t. logits/value, plus the five metrics —
 * ppo_lunarlander.py:110-117, 278-300, 309-322.
 *   logits f32[B,A], value f32[B]: network outputs for minibatch rows 0..B-1
 *   idx    i32[B] or NULL: row b reads act/logp_old/adv/ret at idx[b] of the
 *          rollout slab (fused minibatch gather, ppo_lunarlander.py:268-272)
 *   act i32[*], logp_old f32[*], adv f32[*], ret f32[*]
 *   adv_moments f64[3] or NULL: when given, adv is normalised on the fly with
 *          (mean, population std + 1e-8) — ppo_lunarlander.py:236
 *   dlogits_out f32[B,A], dvalue_out f32[B]: d(loss)/d(logits|value), loss =
 *          mean over the B rows (torch autograd tie rules)
 *   metrics_sum f64[5] or NULL: += (sum -obj, vf*sum (v-ret)^2, sum H, #clipped,
 *          sum (logp_old - logp)).  The caller keeps one zeroed row per minibatch
 *          and divides by B on the host after the whole update (one D2H copy
 *          instead of ppo_lunarlander.py:309-322's five .item() per minibatch).
 *          Reduced block partials -> fixed-order sum through `workspace`
 *          (>= gymrl_reduce_workspace_bytes(), required when metrics_sum != NULL).
 *          With metrics_sum == NULL and workspace != NULL the kernel only writes its
 *          block partials f64[gymrl_loss_blocks(B)][5] to `workspace`: give every minibatch
 *          its own slice of one table and reduce the whole update with ONE
 *          gymrl_reduce_rows launch (what the trainers do).
 */
int gymrl_ppo_loss_fwd_bwd(const float* logits, const float* value, const int32_t* idx,
                           const int32_t* act, const float* logp_old, const float* adv,
                           const float* ret, const double* adv_moments, int B, int A,
                           const gymrl_ppo_cfg* cfg_host, float* dlogits_out,
                           float* dvalue_out, double* metrics_sum, void* workspace,
                           void* stream);
/*
 * L1 under the Gaussian policy above: gymrl_ppo_loss_fwd_bwd's interface (idx, adv_moments, metrics_sum and `workspace` mean what
 * they mean there) with mu f32[B, A] in place of the logits, log_std f32[A], act f32[*, A] the stored actions ->
 * dmu_out f32[B, A], dvalue_out f32[B], dlog_std_out f32[A] (written, not accumulated).  One row per lane, one launch plus the
 * finalising pass(es); no host synchronisation, no float atomics, capturable in a hipGraph.
 * dlog_std is a fixed-order reduction whose order depends on B alone: rows [256 j, 256 j + 256) are segment j, a segment's terms
 * are added in float64 (a wave's lanes by shuffle, the four waves in order) into dls_workspace f64[ceil(B / 256)][A]
 * (gymrl_ppo_gauss_loss_workspace_bytes(B, A) bytes, 8-byte aligned, required), and the finalising pass adds the segments — the
 * same bits from run to run and for every grid.  grid_blocks: 0 = min(ceil(B / 256), 1024) workgroups (gymrl_loss_blocks(B), the
 * rows of the metric partials); a smaller positive value narrows the grid (tests; refused where `workspace` is a caller's
 * partials table, i.e. without metrics_sum).  1 <= A <= 8.  A NaN advantage yields NaN metrics and gradients.
 */
size_t gymrl_ppo_gauss_loss_workspace_bytes(int B, int A);
int gymrl_ppo_gauss_loss_fwd_bwd(const float* mu, const float* log_std, const float* value, const int32_t* idx,
                                 const float* act, const float* logp_old, const float* adv,
                                 const float* ret, const double* adv_moments, int B, int A,
                                 const gymrl_ppo_cfg* cfg_host, float* dmu_out, float* dvalue_out,
                                 float* dlog_std_out, double* metrics_sum, void* workspace,
                                 void* dls_workspace, int grid_blocks, void* stream);

int gymrl_loss_blocks(int B);
/* out[r][k] = sum over b < blocks_per_row of partials[r][b][k]  (f64, fixed order) */
int gymrl_reduce_rows(const double* partials, int rows, int blocks_per_row, int K,
                      double* out, void* stream);

typedef struct {
  float clip_eps_min;  /* ppo_full_lunarlander.py:34 (0.2)  */
  float clip_eps_max;  /* :35 (0.28)                        */
  float dual_clip;     /* :36 (3.0) ratio clamp upper bound */
  float erc_beta_low;  /* :39 (0.06)                        */
  float erc_beta_high; /* :40 (0.06)                        */
  float entropy_coef;  /* current (annealed) value, :662-666 */
  const float* entropy_coef_dev;   /* the same from device memory (a hipGraph replayed across updates: the coefficient is
                                    * annealed after every update) or NULL */
} gymrl_ppo_full_cfg;

/* L3: ppo_full update_model minibatch loss — ppo_full_lunarlander.py:575-652.
 * ent_old f32[*] = behaviour-policy entropy stored at collection (:488).
 * corr_mul f32[B] or NULL: per-row multiplier of the entropy-ratio mask — the covariance clip :611-616
 * (clip_cov_ratio > 0; dead under the reference default :44): the caller picks the rows (covs window, random
 * subset of clip_cov_ratio of them) and passes 0 for those, 1 elsewhere.
 * metrics_sum f64[9]: += (sum policy term, sum 0.5*corr*(v-ret)^2, sum H*corr,
 * sum clipped*corr, sum (logp_old-logp), #erc-masked, sum logp, sum adv,
 * sum logp*adv) — the last three give covs.mean() (:594-596) per minibatch. */
int gymrl_ppo_full_loss_fwd_bwd(const float* logits, const float* value, const int32_t* idx,
                                const int32_t* act, const float* logp_old,
                                const float* ent_old, const float* adv, const float* ret,
                                int B, int A, const gymrl_ppo_full_cfg* cfg_host, const float* corr_mul,
                                float* dlogits_out, float* dvalue_out,
                                double* metrics_sum, void* workspace, void* stream);

/* L4: recurrent-PPO minibatch loss — ppo_lstm_lunarlander.py:716-776.  The L3 terms with
 * (a) every mean a masked mean over the entropy-ratio mask `corr`: sum(x*corr)/sum(corr), 0 when the mask is
 * empty (masked_mean :646-655), and (b) the clipped value loss :763-770
 *   0.5 * masked_mean(max((v - ret)^2, (v_old + clamp(v - v_old, -clip_eps_min, +clip_eps_max) - ret)^2)).
 * val_old f32[*] = values stored at collection.  The RND loss (:775) is a plain mean of squares and stays with
 * the network's autograd.  metrics_sum f64[10]: the nine L3 sums (index 1 = sum 0.5*corr*max(...)) followed by
 * sum(corr); the caller divides sums 0..3 by metrics_sum[9] (or reports 0 when it is 0).
 * corr_mul as in gymrl_ppo_full_loss_fwd_bwd (:747-753).
 * workspace >= gymrl_reduce_workspace_bytes(). */
int gymrl_ppo_rnn_loss_fwd_bwd(const float* logits, const float* value, const int32_t* idx,
                               const int32_t* act, const float* logp_old, const float* ent_old,
                               const float* val_old, const float* adv, const float* ret, int B, int A,
                               const gymrl_ppo_full_cfg* cfg_host, const float* corr_mul, float* dlogits_out,
                               float* dvalue_out, double* metrics_sum, void* workspace, void* stream);

/* Pointwise half of torch.nn.GRU's cell as used by URNN — ppo_lstm_lunarlander.py:449-491 (nn.GRU,
 * batch_first, one layer).  gi = x W_ih^T + b_ih, gh = h W_hh^T + b_hh, both f32[B,3H] in PyTorch's gate
 * order (r, z, n); h f32[B,H]:
 *   r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r*gh_n), h_out = (1 - z)*n + z*h.
 * _bwd recomputes the gates from (gi, gh) and writes dgi, dgh f32[B,3H] and the direct dh f32[B,H]
 * (dh_out * z; the path through gh is the caller's GEMM).  H % 4 == 0, 16-byte aligned pointers. */
int gymrl_gru_cell_fwd(const float* gi, const float* gh, const float* h, int B, int H, float* h_out,
                       void* stream);
int gymrl_gru_cell_bwd(const float* gi, const float* gh, const float* h, const float* dh_out, int B, int H,
                       float* dgi, float* dgh, float* dh, void* stream);

/* RND intrinsic reward — ppo_lstm_lunarlander.py:588-590: rnd[b] = mean_e (predict[b,e] - target[b,e])^2
 * (float32, as numpy's mean of a float32 array), rew_inout[b] += rnd[b] when given, rnd_out[b] = rnd[b]
 * when given.  One wave per row: lane l adds columns l, l+64, ... in order, then a shfl_down tree. */
int gymrl_rnd_reward(const float* predict, const float* target, int B, int E, float* rew_inout,
                     float* rnd_out, void* stream);

/* The GRU over whole episodes — ppg_rnn_lunarlander.py:125-140 (MLPRNN: nn.GRU(256, 64) fed one unbatched [T, 256]
 * episode per call, hidden state reset per episode :335, :377) and the same in ppo_rnn_lunarlander.py.  B episodes in
 * one time-major batch: gi f32[T,B,3H] = x W_ih^T + b_ih (one library GEMM), W_hh f32[3H,H], b_hh f32[3H], h0 f32[B,H]
 * or NULL (zeros), len i32[B] a HOST array with 0 <= len[b] <= T.  Gate order and cell arithmetic are
 * gymrl_gru_cell_fwd's.  _fwd writes h_seq f32[T,B,H] (zero for t >= len[b]) and h_last f32[B,H] = h_{len[b]-1}
 * (h0 when len[b] == 0).  _bwd runs the reverse recurrence from the stored h_seq: d_hseq f32[T,B,H] and d_hlast f32[B,H]
 * are the incoming gradients (either may be NULL = zeros); it writes dgi, dgh f32[T,B,3H] (zero for t >= len[b]) and
 * dh0 f32[B,H] (may be NULL).  dW_hh = sum_t dgh_t^T h_{t-1}, db_hh, dW_ih and dx are the caller's GEMMs over the
 * flattened rows.  One launch per 768 episodes, all T steps inside; H in {16, 32, 48, 64}; W_hh, h0, h_seq 16-byte
 * aligned.  With T == 0 or B == 0 the [T,B,*] arrays have no element and may be NULL (h_last too when B == 0); T == 0
 * still writes h_last = h0 and dh0 = d_hlast.  -22 on anything else, before any HIP call. */
int gymrl_gru_seq_fwd(const float* gi, const float* W_hh, const float* b_hh, const float* h0, const int32_t* len,
                      int T, int B, int H, float* h_seq, float* h_last, void* stream);
int gymrl_gru_seq_bwd(const float* gi, const float* W_hh, const float* b_hh, const float* h0, const float* h_seq,
                      const float* d_hseq, const float* d_hlast, const int32_t* len, int T, int B, int H, float* dgi,
                      float* dgh, float* dh0, void* stream);

/* torch.nn.LSTM's cell — ppo_lstm_lunarlander.py:449-491 (URNN with layer=nn.LSTM, hidden state cat(h, c)).  The
 * pointwise half on gi = x W_ih^T + b_ih and gh = h W_hh^T + b_hh, both f32[B,4H] in PyTorch's gate order (i, f, g, o);
 * c f32[B,H]:  a = gi + gh, i = s(a_i), f = s(a_f), g = tanh(a_g), o = s(a_o), c_out = f*c + i*g, h_out = o*tanh(c_out).
 * _bwd recomputes the gates from (gi, gh, c); dh_out, dc_out f32[B,H] are dL/dh_out and dL/dc_out (dc_out may be NULL =
 * zeros).  It writes dgates f32[B,4H], which is both dgi and dgh, and dc f32[B,H] = dL/dc through the cell state (the
 * path through h is the caller's dgates . W_hh).  H % 4 == 0, 16-byte aligned pointers; -22 otherwise, before any HIP
 * call. */
int gymrl_lstm_cell_fwd(const float* gi, const float* gh, const float* c, int B, int H, float* h_out, float* c_out,
                        void* stream);
int gymrl_lstm_cell_bwd(const float* gi, const float* gh, const float* c, const float* dh_out, const float* dc_out, int B,
                        int H, float* dgates, float* dc, void* stream);

/* The LSTM recurrence in one launch per direction; the contract is gymrl_gru_seq_*'s.  B rows in one time-major batch:
 * gi f32[T,B,4H] = x W_ih^T + b_ih (one library GEMM), W_hh f32[4H,H], b_hh f32[4H], h0, c0 f32[B,H] or NULL (zeros),
 * len i32[B] a HOST array with 0 <= len[b] <= T.  Gate order and cell arithmetic are gymrl_lstm_cell_fwd's.  _fwd writes
 * h_seq, c_seq f32[T,B,H] (zero for t >= len[b]) and h_last, c_last f32[B,H] = (h, c)_{len[b]-1} ((h0, c0) when
 * len[b] == 0; either may be NULL).  _bwd runs the reverse recurrence from the stored h_seq, c_seq: d_hseq f32[T,B,H],
 * d_hlast and d_clast f32[B,H] are the incoming gradients (each may be NULL = zeros); it writes dgates f32[T,B,4H] (both
 * dgi and dgh; zero for t >= len[b]) and dh0, dc0 f32[B,H] (each may be NULL).  dW_hh = sum_t dgates_t^T h_{t-1}, db_hh,
 * dW_ih and dx are the caller's GEMMs over the flattened rows.  One launch per 768 rows, all T steps inside;
 * H in {16, 32, 48, 64}; W_hh, h0, h_seq 16-byte aligned.  -22 on anything else, before any HIP call. */
int gymrl_lstm_seq_fwd(const float* gi, const float* W_hh, const float* b_hh, const float* h0, const float* c0,
                       const int32_t* len, int T, int B, int H, float* h_seq, float* c_seq, float* h_last, float* c_last,
                       void* stream);
int gymrl_lstm_seq_bwd(const float* gi, const float* W_hh, const float* b_hh, const float* h0, const float* c0,
                       const float* h_seq, const float* c_seq, const float* d_hseq, const float* d_hlast,
                       const float* d_clast, const int32_t* len, int T, int B, int H, float* dgates, float* dh0, float* dc0,
                       void* stream);

/* EpisodeBuffer.compute_advantage — ppg_rnn_lunarlander.py:198-215 (== ppo_rnn_lunarlander.py), per episode, E
 * episodes stored back to back: episode e is rows [offsets[e], offsets[e+1]) of the flat f32 / u8 arrays; offsets
 * i64[E+1] a HOST array, offsets[0] == 0, no empty episode.  G2's arithmetic (gymrl_gae_dw): f32 td-error
 * (rew + gamma*next_val*(1-dw)) - val, the f32 recursion gae = (gamma*lam)*gae*(1-done) + delta; v_target = adv + val;
 * adv_norm = (adv - mean) / (std + 1e-8) with the episode's mean and unbiased std taken in f64 (a length-1 episode has
 * std NaN and normalises to NaN, as it does in torch).  adv_raw f32 (may be NULL) = the unnormalised adv;
 * ep_moments f64[E][2] (may be NULL) = (mean, std).  One workgroup per episode, 255 episodes per launch. */
int gymrl_episode_gae(const float* rew, const float* val, const float* next_val, const uint8_t* done,
                      const uint8_t* dw, const int64_t* offsets, int E, double gamma, double lam, float* adv_raw,
                      float* adv_norm, float* v_target, double* ep_moments, void* stream);

/* L5: PPG / PPO-RNN policy phase — ppg_rnn_lunarlander.py:330-370 over G episodes (offsets as gymrl_episode_gae).
 * logits f32[M,A] (2 <= A <= 8) of probs = softmax(logits); Categorical(probs) semantics: p / sum p, every log
 * log(clamp(p, FLT_EPSILON, 1 - FLT_EPSILON)).  Per episode: clip_loss = -mean(where(adv < 0, max(min(r*adv,
 * clamp(r, 1-clip, 1+clip)*adv), dual_clip*adv), min(...))), value_loss = mean((v_target - value)^2), entropy_loss =
 * -mean(H); loss = mean over episodes of clip_loss + val_coef*value_loss + ent_coef*entropy_loss.  Writes dlogits
 * f32[M,A], dvalue f32[M], metrics_ep f64[G][5] = (loss, clip_loss, value_loss, entropy_loss, adv mean) of each
 * episode, and metrics_sum f64[5] (may be NULL) += their mean over the G episodes.  act must lie in [0, A): an action
 * outside makes its log-prob NaN, and with it that episode's loss, metrics and gradients (L6 alike). */
int gymrl_ppg_policy_loss_fwd_bwd(const float* logits, const float* value, const int32_t* act,
                                  const float* old_logp, const float* adv, const float* v_target,
                                  const int64_t* offsets, int G, int A, float clip, float dual_clip, float val_coef,
                                  float ent_coef, float* dlogits, float* dvalue, double* metrics_ep,
                                  double* metrics_sum, void* stream);

/* L6: PPG aux phase — ppg_rnn_lunarlander.py:372-393.  Per episode mse(v_target, aux_value) + beta *
 * mse(log pi(a), old_logp) with L5's clamped log; loss = mean over episodes.  Writes dlogits, d_aux, metrics_ep
 * f64[G][3] = (aux_value_loss, clone_loss, joint) and metrics_sum f64[3] (may be NULL) += their mean. */
int gymrl_ppg_aux_loss_fwd_bwd(const float* logits, const float* aux_value, const int32_t* act,
                               const float* old_logp, const float* v_target, const int64_t* offsets, int G, int A,
                               float beta, float* dlogits, float* d_aux, double* metrics_ep, double* metrics_sum,
                               void* stream);

/* The acting step of the PPG / PPO-RNN trainers — ppg_rnn_lunarlander.py:311-328 (choose_action / evaluate_action) over
 * ActorCriticPPG.forward :165-176 for N envs in ONE launch: PSCN(D, 256) (:92-122: four Linear -> PReLU layers 256, 128,
 * 64, 32 wide, each layer's first half kept, its second half fed on), MLPRNN(256, 256) (:125-140: cat(rnn_linear(x), one
 * nn.GRU(256, 64) step)), actor_fc MLP([256, 64, A]) and critic_fc MLP([256, 32, 1]) (:156-157; one PReLU slope per MLP),
 * probs = softmax(logits).  Every pointer of gymrl_mlprnn_params is the nn.Module parameter in its torch layout (Linear
 * weights [out, in] row-major, PReLU slopes f32[1], GRU weights in gate order r, z, n); the weights marked (16) are read
 * with 16-byte loads and must be 16-byte aligned.  Exact f32 throughout (MFMA f32 products, no reduced precision).
 *   x f32[N,D] (1 <= D <= 16), h_in f32[N,64]; h_out f32[N,64] (may be h_in) = the GRU cell of gymrl_gru_cell_fwd on
 *   the step's gi, gh; value f32[N]; probs f32[N,A] (may be NULL) = softmax; act i32[N]: with deterministic, the first
 *   maximum of probs (evaluate_action); otherwise Categorical(probs).sample() = argmax_k p_k / q_k over p / sum p with
 *   q ~ Exp(1) from noise_exp f32[N,A] (may be NULL) or Philox keyed (seed, counter, env_id0 + row) as in
 *   gymrl_categorical_sample; logp f32[N] = log(clamp(p_a / sum p, FLT_EPSILON, 1 - FLT_EPSILON)), the expression of
 *   L5 / L6.  live u8[N] (may be NULL = all): rows with live == 0 write nothing.  2 <= A <= 8, 0 <= N <= 2^24; -22 on
 *   anything else (NULL required pointers, misaligned weights) before any HIP call.  One workgroup per 16 envs. */
typedef struct gymrl_mlprnn_params {
  const float* pscn_w[4];   /* fc_head.layers.i.mlp.0.weight: [256,D], [128,128] (16), [64,64] (16), [32,32] (16) */
  const float* pscn_b[4];
  const float* pscn_a[4];   /* fc_head.layers.i.mlp.1.weight (PReLU) */
  const float* lin_w;       /* rnn.rnn_linear.mlp.0.weight [192,256] (16) */
  const float* lin_b;
  const float* w_ih;        /* rnn.rnn.weight_ih_l0 [192,256] (16) */
  const float* b_ih;
  const float* w_hh;        /* rnn.rnn.weight_hh_l0 [192,64] (16) */
  const float* b_hh;
  const float* actor_w1;    /* actor_fc.mlp.0.weight [64,256] (16) */
  const float* actor_b1;
  const float* actor_a;     /* actor_fc.mlp.1.weight */
  const float* actor_w2;    /* actor_fc.mlp.2.weight [A,64] */
  const float* actor_b2;
  const float* critic_w1;   /* critic_fc.mlp.0.weight [32,256] (16) */
  const float* critic_b1;
  const float* critic_a;
  const float* critic_w2;   /* critic_fc.mlp.2.weight [1,32] */
  const float* critic_b2;
} gymrl_mlprnn_params;
size_t gymrl_mlprnn_params_bytes(void);   /* sizeof(gymrl_mlprnn_params): a binding checks its mirror */
int gymrl_mlprnn_act(const float* x, const float* h_in, const gymrl_mlprnn_params* params, int N, int D, int A,
                     const uint8_t* live, const float* noise_exp, uint64_t seed, uint64_t counter, int64_t env_id0,
                     int deterministic, float* h_out, int32_t* act, float* logp, float* value, float* probs,
                     void* stream);

/*
 * P6/P7: minibatch staging — ppo_lunarlander.py:238-272 (lists -> tensors, shuffled
 * index slices).  gymrl_pack_rollout writes one 64-B record per transition
 *   packed[i] = { obs[i][0..D) (zero padded to 12) | act bits | logp_old | adv | ret }
 * once per rollout; gymrl_gather_minibatch then fetches ONE random cache line per
 * sample (idx i32[B] = a slice of the epoch's permutation) into contiguous rows
 * obs_out f32[B,D], act_out i32[B], logp_out/adv_out/ret_out f32[B].  D <= 12.
 */
/* P6: the epoch shuffle — ppo_lunarlander.py:262 `np.random.shuffle(indices)`.  perm_out i32[M] = a keyed
 * bijection of [0, M) evaluated per element (gymrl_device.hpp keyed_permute): for M <= 16 a Fisher-Yates draw
 * over a 4-bit table in one register (uniform over the M! orders to 2^-24 relative); above, alternating Feistel
 * rounds on ceil(log2 M) bits with a Philox4x32-10 round function keyed by (seed, counter), cycle-walked into
 * range — 12 rounds below 10 bits (M <= 512), 6 from there up (M >= 513).  tests/test_rng_distributions.py holds the position x value,
 * ordered-pair and minibatch co-membership laws to the uniform permutation's.  One streaming write of 4M bytes
 * instead of torch.randperm's key sort (3.3 ms per epoch at M = 2^23).  Deterministic in (seed, counter, M);
 * parity runs pass the reference's own order instead. */
int gymrl_permutation(uint64_t seed, uint64_t counter, int64_t M, int32_t* perm_out, void* stream);
int gymrl_pack_rollout(const float* obs, const int32_t* act, const float* logp,
                       const float* adv, const float* ret, int64_t M, int obs_dim,
                       float* packed, void* stream);
int gymrl_gather_minibatch(const float* packed, const int32_t* idx, int B, int obs_dim,
                           float* obs_out, int32_t* act_out, float* logp_out,
                           float* adv_out, float* ret_out, void* stream);
/* out [B, row_floats] = src[idx[b], :] — a minibatch of rows by index (ppo_full_lunarlander.py:574 `states[mb_idx]`);
 * row_floats a multiple of 4, src and out 16-byte aligned. */
int gymrl_gather_rows(const float* src, const int32_t* idx, int B, int row_floats, float* out, void* stream);

/* ------------------------------------------------------------ optimiser --- */
/*
 * O1 / D4 / R4: clip_grad_norm_ + Adam on ONE flat fp32 parameter buffer —
 * ppo_lunarlander.py:169,302-307; dqn_cartpole.py:163-166 (clamp_abs = 1);
 * rainbow_dqn_cartpole.py:343-345; sac_pendulum.py:244-255.
 *   gymrl_sqnorm:    sqnorm_out f64[1] (device) = sum (g*grad_scale)^2, fixed-order
 *                    reduction; workspace >= gymrl_reduce_workspace_bytes().  The order is part of the
 *                    contract (oracle/gymrl_oracle.c orc_sqnorm restates it; the optimiser step is pinned bit for
 *                    bit): nb = clamp(ceil(n/4096), 1, 1024) workgroups of 256; thread t of workgroup b adds the
 *                    float4 groups b*256+t, +nb*256, ... as ((a^2+b^2)+c^2)+d^2 in f64; the n%4 tail goes to
 *                    threads 0..2 of workgroup 0; waves fold by halves (32, 16, .. 1), the 4 wave sums add in
 *                    order; the final pass gives thread t partials t, t+256, ... and folds 256 sums by halves.
 *   gymrl_adam_step: scale = max_grad_norm>0 ? min(1, max_norm/(sqrt(sqnorm)+1e-6)) : 1
 *                    g' = g*grad_scale*scale, then clamped to +-clamp_abs when clamp_abs>0
 *                    A gradient that is not finite does what torch does: a NaN norm gives scale = NaN (every
 *                    parameter goes NaN), an infinite one scale = 0 (NaN at the infinite element only), and the
 *                    clamp keeps a NaN element NaN.
 *                    m,v,p updated as torch.optim.Adam (no amsgrad, no decay);
 *                    g is zeroed (zero_grad fused) when zero_grad != 0.
 *   lr_dev f32[1] or NULL (then lr_host is used): device-resident lr lets LR
 *   annealing change the rate without re-capturing a graph.
 *   grad_scale multiplies g first (1/world_size after an all-reduce SUM).
 *   bias_dev f32[4] or NULL: device-resident {lr/(1-b1^t), 1/(1-b1^t), sqrt(1-b2^t), 0} — the only
 *   step-dependent scalars of the update.  With it (and `step` ignored) a hipGraph captured around the
 *   optimiser step replays unchanged; the host refreshes the block before each replay with
 *   gymrl_adam_bias (host arithmetic, identical to the eager path's) + gymrl_store_scalars.
 *   polyak_target f32[n] or NULL: theta' <- tau*theta + (1-tau)*theta' (gymrl_soft_update's expression) on the
 *   parameters this launch has just written — optimiser step + soft target update in one pass.
 *   gymrl_store_scalars: copies nbytes <= 3840 (multiple of 4) of host scalars into device memory as ONE
 *   launch whose payload is the kernel argument (stream-ordered, nothing to fence, not capturable state).
 *
 * Per-step scalars on the device.  Entry points whose arguments change every vector step — ring cursors, Philox
 * draw counters, the PER exponent — take a trailing `*_dev` / `dev` pointer (NULL on the plain path): when given,
 * the kernel reads those values from DEVICE memory instead of its host arguments, so the launch can be recorded
 * into a hipGraph and replayed with new values that the host stages beforehand with ONE gymrl_store_scalars for a
 * whole chunk of vector steps (gymrl_amd/graphs.py StepChunk: acting, env step, ring append, index draw and update
 * of 16 vector steps = one scalar store + one graph launch).  Layouts (8-byte aligned):
 *   gymrl_replay_append   cursor_dev     int64[1]  {cursor}
 *   gymrl_uniform_indices dev            {uint64 counter; int64 size}
 *   gymrl_nstep_push      dev            int64[2]  {pushes, cursor}   (the return value follows the HOST pushes)
 *   gymrl_per_update      idx_start_dev  int64[1]  {idx_start}        (idx == NULL only)
 *   gymrl_per_sample      dev            {uint64 counter; int64 size; double beta}
 *   gymrl_noisy_noise     counter_dev    uint64[1] {counter}
 */
int gymrl_sqnorm(const float* g, int64_t n, float grad_scale, double* sqnorm_out,
                 void* workspace, void* stream);
int gymrl_adam_step(float* p, float* g, float* m, float* v, int64_t n,
                    double lr_host, const float* lr_dev, double beta1, double beta2,
                    double eps, int64_t step, const float* bias_dev, float grad_scale,
                    float max_grad_norm, const double* sqnorm, float clamp_abs, int zero_grad,
                    float* polyak_target, double tau, void* stream);
/*
 * clip_grad_norm_ + Adam as TWO launches instead of gymrl_sqnorm's two + gymrl_adam_step's one: the squared norm's first level,
 * then the Adam kernel, every workgroup of which folds the block partials itself exactly as gymrl_sqnorm's second launch does.
 * Same sums in the same order, same bits (tests/test_hip_parity.py).  max_grad_norm > 0; sqnorm_out f64[1] or NULL (the squared
 * norm, for logging); workspace: gymrl_reduce_workspace_bytes().  Other arguments as gymrl_adam_step.
 */
int gymrl_clip_adam_step(float* p, float* g, float* m, float* v, int64_t n, double lr_host, const float* lr_dev, double beta1,
                         double beta2, double eps, int64_t step, const float* bias_dev, float grad_scale, float max_grad_norm,
                         double* sqnorm_out, float clamp_abs, int zero_grad, float* polyak_target, double tau, void* workspace,
                         void* stream);

int gymrl_adam_bias(double lr, double beta1, double beta2, int64_t step, float* out_host4);
int gymrl_store_scalars(void* dst_dev, const void* src_host, int nbytes, void* stream);

/* R4 / A4: theta' <- tau*theta + (1-tau)*theta' on flat buffers —
 * rainbow_dqn_cartpole.py:347-352, sac_pendulum.py:194-199. */
int gymrl_soft_update(float* target, const float* source, int64_t n, double tau,
                      void* stream);

/* ============================================================ MLP forward == */
/*
 * P1 / D1 / A1 inference path: ActorCritic.forward ppo_lunarlander.py:86-90 (as called by
 * get_action :92-104 and get_value :106-108 once per env step), QNetwork.forward
 * dqn_cartpole.py:62-65 and Actor.forward sac_pendulum.py:66-74 in select_action.  The
 * reference runs one torch Linear + activation call per layer on a B = 1 batch; here the
 * whole chain of Linear(+Tanh|ReLU) layers runs in ONE launch on [n_rows, in_dim] rows, 16
 * rows per workgroup, activations in LDS, f32 MFMA (v_mfma_f32_16x16x4_f32: exact f32).
 *
 * A network is a list of <= GYMRL_MLP_MAX_STAGES stages  y = act(x W^T + b):
 *   W = the PACKED image of the f32[out_dim, in_dim] row-major weight (torch
 *   nn.Linear.weight) that gymrl_mlp_pack writes — gymrl_mlp_packed_floats(out_dim, in_dim)
 *   floats, P[tile][kblock][lane][c] = W[16 tile + (lane & 15)][16 kblock + 4 (lane >> 4) + c],
 *   zero padded to 16-row tiles and to K rounded up to 64; repack after every parameter
 *   update (one tiny launch per layer).  b f32[out_dim] or NULL (read in place);
 *   src = -1 reads the network input x, 0..2 reads LDS buffer `src` (written by an earlier
 *   stage); dst = 0..2 writes LDS buffer `dst` (out_dim <= GYMRL_MLP_MAX_WIDTH), dst = -1
 *   writes out[row*out_stride + col] in HBM.  in_dim <= GYMRL_MLP_MAX_WIDTH (network input
 *   <= GYMRL_MLP_MAX_INPUT).  Two heads on one trunk are two stages reading the same src.
 * Summation order (bit-reproducible on the CPU, see csrc/mlp.hip): per output element
 *   acc = 0; for kb in 0,16,.. < roundup(in_dim,64): for j in 0..3: for q in 0..3:
 *     acc = fmaf(x[kb+4q+j], W[n][kb+4q+j], acc)   (k >= in_dim contribute fmaf(0,0,acc));
 *   y = act(acc + b[n]); tanh = the deterministic
 *   polynomial/exp kernel of csrc/gymrl_device.hpp.
 */
#define GYMRL_MLP_MAX_STAGES 8
#define GYMRL_MLP_MAX_WIDTH 256
#define GYMRL_MLP_MAX_INPUT 64
enum { GYMRL_ACT_NONE = 0, GYMRL_ACT_TANH = 1, GYMRL_ACT_RELU = 2, GYMRL_ACT_CLAMP = 3, GYMRL_ACT_DUELING = 4, GYMRL_ACT_SILU = 5 /* 3-5: gymrl_lin_* only; 4, 5: forward only */ };
typedef struct {
  const float* W;
  const float* b;
  float* out;       /* dst == -1 only */
  int in_dim, out_dim, act, src, dst, out_stride;
} gymrl_mlp_stage;
typedef struct {
  int n_stages;
  gymrl_mlp_stage stage[GYMRL_MLP_MAX_STAGES];
} gymrl_mlp_desc;
size_t gymrl_mlp_packed_floats(int out_dim, int in_dim);
int gymrl_mlp_pack(const float* W, int out_dim, int in_dim, float* packed, void* stream);
int gymrl_mlp_forward(const float* x, int n_rows, int in_dim, const gymrl_mlp_desc* desc,
                      void* stream);

/* ======================================================= MLP policy stacks == */
/*
 * gymrl_mlp_pack for a POPULATION: P flat parameter vectors x n_layers layers into the packed layout, with the biases, in ONE
 * launch (csrc/pack_stack.hip) — what the one-launch evaluators read as a stack of policies (gymrl_lunar_policy_eval with
 * policy_stride = packed_stride and a gymrl_mlp_desc whose W / b point into row 0 at w_at / b_at).
 *   Weights   for every policy p and layer k the gymrl_mlp_packed_floats(out_dim, in_dim) floats from
 *             packed + p * packed_stride + w_at are exactly what gymrl_mlp_pack writes for the weight
 *             params + p * params_stride + w_off (f32[out_dim][in_dim] row-major):
 *             P[tile][kblock][lane][c] = W[16 tile + (lane & 15)][16 kblock + 4 (lane >> 4) + c], zeros beyond out_dim and
 *             beyond in_dim, K rounded up to 64.
 *   Biases    the out_dim floats from b_at are params[p][b_off ..]; the floats up to the next multiple of four are 0.0f.
 *   Untouched no float of a packed row outside these 2 n_layers ranges is written: a caller's padding and the tail of a reused
 *             buffer survive.
 *   Copy only every float written is a copy or a zero, no arithmetic: the bits of n_layers gymrl_mlp_pack launches and bias
 *             copies per policy (tests/test_pack_stack_gpu.py).
 * Kernel: one thread per output float4, gridDim.y = P, gridDim.x covers a row's float4s, the layer table by value in the kernel
 * arguments; no LDS, no atomics, no workgroup waits for another; one coalesced 16-byte store per lane; the weight reads are
 * strided by in_dim across lanes as gymrl_mlp_pack's are (not staged through LDS).
 * -EINVAL before any launch: NULL args, params or packed; P < 1 or P > 65535; n_layers outside 1..GYMRL_MLP_MAX_STAGES; an
 * out_dim or in_dim < 1 or > GYMRL_MLP_MAX_WIDTH (what gymrl_mlp_forward takes between stages); a negative offset;
 * w_off + out_dim * in_dim or b_off + out_dim beyond params_stride; w_at, b_at or packed_stride not a multiple of 4; a packed
 * range that ends beyond packed_stride; two packed ranges of a row that overlap; packed not 16-byte aligned; params not 4-byte.
 */
typedef struct {
  int out_dim, in_dim;
  int64_t w_off, b_off;                    /* floats into a params row: W f32[out_dim][in_dim] row-major, b f32[out_dim] */
  int64_t w_at, b_at;                      /* floats into a packed row, each % 4 == 0 */
} gymrl_mlp_pack_layer;
typedef struct {
  int P;                                   /* policies, 1..65535 */
  int n_layers;                            /* 1..GYMRL_MLP_MAX_STAGES */
  const float* params;                     /* f32[P][params_stride]: row p = policy p's flat parameter vector */
  int64_t params_stride;                   /* floats between rows */
  float* packed;                           /* f32[P][packed_stride] out, 16-byte aligned */
  int64_t packed_stride;                   /* floats between rows, % 4 == 0 */
  gymrl_mlp_pack_layer layer[GYMRL_MLP_MAX_STAGES];
} gymrl_mlp_pack_stack_args;
size_t gymrl_mlp_pack_stack_args_bytes(void);  /* sizeof(gymrl_mlp_pack_stack_args) */
int gymrl_mlp_pack_stack(const gymrl_mlp_pack_stack_args* args, void* stream);

/* ======================================================== persistent rollout */
/*
 * P4: PPOTrainer.collect_rollout — ppo_lunarlander.py:198-231 — for LunarLander-v3 as one launch per
 * chunk of vector steps: policy forward (gymrl_mlp_forward's stages, logits [4] then value [1] as the two
 * dst == -1 stages; their `out` pointers are ignored), categorical draw, GAE chunk-map composition, env
 * step with reset-on-done, slab writes.  A workgroup owns 16 envs for all `nsteps` steps and never waits
 * for another workgroup, so a step costs the mean per-wavefront solver time instead of the slowest
 * wavefront's.  Bit-identical to the step-by-step sequence gymrl_mlp_forward -> gymrl_categorical_sample
 * (same seed / counter0 + t / env ids, or the same explicit noise) -> gymrl_env_step.
 *   obs f32[T+1][N][8] (row t0 must hold the current observations), act i32[T][N], logp/val/rew f32[T][N],
 *   done u8[T][N], ep_ret f32[T][N] or NULL (written where done), next_value f32[N] (written by the
 *   launch that reaches t0 + nsteps == T: V(obs[T]), the bootstrap of :225-229), noise_exp f32[T][N][4] or
 *   NULL, gae_running f64[2][N] + gae_workspace (gymrl_gae_workspace_bytes(T, N)) or NULL for no online
 *   composition (then gymrl_gae variant 1), ep_stats f64[3] or NULL, wg_ticks: optional load-balance probe.
 */
typedef struct {
  void* env_state;            /* gymrl_env_state_bytes(GYMRL_ENV_LUNARLANDER, n_envs)          */
  int n_envs;
  uint64_t seed;
  int64_t env_id0;
  uint64_t counter0;          /* Philox counter of step 0 of this rollout (step t uses counter0 + t) */
  float* obs;
  int32_t* act;
  float* logp;
  float* val;
  float* rew;
  uint8_t* done;
  float* ep_ret;
  float* next_value;
  const float* noise_exp;
  double* gae_running;
  void* gae_workspace;
  double gamma, lam;
  double* ep_stats;
  unsigned long long* wg_ticks; /* NULL, or u64[2][ceil(N/16)]: start / end of every workgroup in 100 MHz ticks */
  int T, t0, nsteps;
  /* gymrl_rollout_lunar_mhc only (gymrl_rollout_lunar ignores them): */
  float* ent;                 /* f32[T][N] or NULL: entropy of the behaviour policy at every step             */
  double lam2;                /* decoupled-lambda GAE (G3): the critic's lambda, with gae_running2             */
  double* gae_running2;       /* f64[2][N] or NULL; with it gae_workspace is gymrl_gae_decoupled_workspace_bytes(T, N) */
  /* both kernels: */
  int refill;                 /* != 0: while wave 0 steps the envs, wave 1 of the workgroup keeps every env's NEXT episode
                               * prepared in the state buffer's spare world (reset() ends with a full physics step; built inline
                               * it stalls the 15 other envs of the wave on every step an episode ends).  A spare is a pure
                               * function of (seed, env id, episode): the slab is bit-identical either way.             */
  /* gymrl_rollout_lunar only (ABI 3): */
  int gae_carry;              /* != 0 (with gae_running): the launch that reaches T also runs the blocked scan's carry pass for its
                               * own envs into the workspace (gymrl_gae_blk_carry's arithmetic, operation for operation), so
                               * gymrl_gae may be called with variant 3 — the apply launch alone; the same bits as variant 2 */
} gymrl_rollout_lunar_args;
int gymrl_rollout_lunar(const gymrl_rollout_lunar_args* args, const gymrl_mlp_desc* policy, void* stream);
/* The same rollout for PPO on CartPole-v1 (PPOTrainer with env_name "CartPole-v1": the reference's collect_rollout is
 * env-agnostic, ppo_lunarlander.py:198-231): obs f32[T+1][N][4], the policy's two dst == -1 stages are logits [2] then
 * value [1], env_state is gymrl_env_state_bytes(GYMRL_ENV_CARTPOLE, n_envs); `ent`, `lam2`, `gae_running2`, `refill` and
 * `wg_ticks` are ignored.  A step by step CartPole vector step is three launches at the launch floor; here a workgroup
 * keeps its 16 envs for the whole chunk.  Bit-identical to gymrl_mlp_forward -> gymrl_categorical_sample -> gymrl_env_step. */
int gymrl_rollout_cartpole(const gymrl_rollout_lunar_args* args, const gymrl_mlp_desc* policy, void* stream);
/* The same rollout for PPO on any of the discrete classic-control envs (csrc/rollout_classic.hip: one kernel template, one
 * instantiation per env): env_kind is GYMRL_ENV_CARTPOLE (D = 4 observations, A = 2 actions), GYMRL_ENV_MOUNTAINCAR (2, 3) or
 * GYMRL_ENV_ACROBOT (6, 3).  The argument block is gymrl_rollout_cartpole's, with the same ignored fields: obs f32[T+1][N][D],
 * noise_exp f32[T][N][A] or NULL, env_state is gymrl_env_state_bytes(env_kind, n_envs); the policy's two dst == -1 stages are
 * logits [A] then value [1].  With GYMRL_ENV_CARTPOLE it is gymrl_rollout_cartpole's launch.  Bit-identical to gymrl_mlp_forward
 * -> gymrl_categorical_sample -> gymrl_env_step.  -EINVAL before any launch: everything gymrl_rollout_cartpole refuses, any other
 * kind, a descriptor whose input width is not D or whose logit width is not A, and an `obs` that is not aligned to the store of
 * an observation row: 16 bytes (CartPole-v1: one float4) or 8 bytes (the other two: one and three float2). */
int gymrl_rollout_classic(int env_kind, const gymrl_rollout_lunar_args* args, const gymrl_mlp_desc* policy, void* stream);
/* The same rollout for PPO on Pendulum-v1 under the Gaussian policy (gymrl_gaussian_sample above; csrc/rollout_classic.hip, the
 * fourth instance of its kernel template): obs f32[T+1][N][3], act f32[T][N] the UNCLIPPED draw (the stepper clips the torque to
 * +-2), the policy's two dst == -1 stages are the mean [1] then the value [1], log_std f32[1], noise_normal f32[T][N][1] or NULL,
 * env_state is gymrl_env_state_bytes(GYMRL_ENV_PENDULUM, n_envs).  rew holds the env's reward times reward_scale (one float32
 * multiply); ep_ret and ep_stats stay unscaled.  The other members are gymrl_rollout_lunar_args'.  Bit-identical to
 * gymrl_mlp_forward -> gymrl_gaussian_sample -> gymrl_env_step (-> rew * reward_scale).  An observation row is 12 bytes: it is
 * stored as three floats, and `obs`, `act`, `log_std` and `noise_normal` are 4-byte aligned.  -EINVAL before any launch: a NULL
 * block, policy, env_state, slab, next_value or log_std, n_envs <= 0, T <= 0, a window outside [0, T], gae_running without
 * gae_workspace, a NaN reward_scale, a misaligned pointer, and a descriptor that is not (3 -> ... -> 1, 1). */
typedef struct {
  void* env_state;
  int n_envs;
  uint64_t seed;
  int64_t env_id0;
  uint64_t counter0;
  float* obs;
  float* act;
  float* logp;
  float* val;
  float* rew;
  uint8_t* done;
  float* ep_ret;
  float* next_value;
  const float* log_std;
  const float* noise_normal;
  float reward_scale;
  double* gae_running;
  void* gae_workspace;
  double gamma, lam;
  double* ep_stats;
  int T, t0, nsteps;
} gymrl_rollout_pendulum_args;
size_t gymrl_rollout_pendulum_args_bytes(void);  /* sizeof(gymrl_rollout_pendulum_args) */
int gymrl_rollout_pendulum(const gymrl_rollout_pendulum_args* args, const gymrl_mlp_desc* policy, void* stream);
/* The same persistent rollout for PPO-full (ppo_full_lunarlander.py collect_experience :440-505): the policy is the mHC network
 * (gymrl_mhc_policy, declared with gymrl_mhc_policy_forward below; obs_dim 8, n_act 4), `ent` receives the behaviour policy's
 * entropy, and with gae_running2 / lam2 both decoupled-lambda chunk maps are composed (the actor's with `lam`, then the critic's).
 * Bit-identical to the step-by-step sequence gymrl_mhc_policy_forward -> gymrl_categorical_sample(online) -> gymrl_env_step. */
struct gymrl_mhc_policy_s;
int gymrl_rollout_lunar_mhc(const gymrl_rollout_lunar_args* args, const struct gymrl_mhc_policy_s* policy, void* stream);

/* ------------------------------ LunarLander-v3 PPO policies: whole episodes in one launch ---- */
/*
 * Replaces the eval() loops of ppo_lunarlander.py:368-399 and ppo_full_lunarlander.py (get_action(deterministic=True) -> env.step
 * until the episode is over, up to the TimeLimit of 1000 steps) for P policies x E episodes at a time (csrc/eval_lunar.hip; the
 * episode loop is stated once in csrc/eval_lunar_device.hpp).  ONE workgroup of 256 threads carries 16 episodes of one policy from
 * reset to their end, laid out like gymrl_rollout_lunar's: all four waves run the policy forward of the 16 observations, wave 0
 * takes the FIRST maximum of the four logits (gymrl_categorical_sample's deterministic branch) and steps the envs four lanes per
 * env.  The grid is P * ceil(E / 16) workgroups.  The worlds are built in the kernel (gymrl_env_reset's arithmetic) and stay in
 * LDS: there is no env_state buffer.  A finished episode's lanes idle; the workgroup leaves when all 16 are finished (at `cap` at
 * the latest) on one LDS word behind a barrier every thread reaches.  No atomics, nothing waits for another workgroup, no random
 * draw, and global memory is only written where an episode ends.
 *
 * Episode i = p * E + e is the first episode of env stream_id0 + e under `seed` — the SAME starts for every policy, env e of a
 * gymrl_env_reset with env_id0 = stream_id0.  It ends with terminated = 1 when the env says so, with terminated = 0 when its length
 * reaches `cap`.
 *
 * Outputs, each [P * E], written once when the episode ends: returns (float64: the sum of the float32 rewards in step order),
 * lengths, terminated, terminal_obs [P * E][8] (optional) the observation after the last step.
 *
 * gymrl_lunar_policy_eval: the policy is gymrl_rollout_lunar's descriptor, logits [4] then value [1] as the two dst == -1 stages
 * (their `out` pointers are ignored); stages that only feed the value are not run.  Policy p reads every stage's W and b
 * p * policy_stride floats behind policy 0's (0: P == 1), the rule of gymrl_classic_policy_eval further down.  Bit-identical to the step-by-step
 * sequence gymrl_mlp_forward -> gymrl_categorical_sample(deterministic) -> gymrl_env_step.
 * gymrl_lunar_mhc_eval: the policy is the mHC network (gymrl_mhc_policy; obs_dim 8, n_act 4), P == 1.  Bit-identical to
 * gymrl_mhc_policy_forward -> gymrl_categorical_sample(deterministic) -> gymrl_env_step.
 * -EINVAL before any launch: NULL args / policy / returns / lengths / terminated, P < 1, E < 1, cap outside 1..1000, a negative
 * policy_stride or one that is not a multiple of 4, policy_stride == 0 with P > 1, P > 1 on the mHC entry, P * E above INT32_MAX,
 * stream_id0 < 0, a pointer that is not aligned (returns: 8 bytes; lengths: 4; terminal_obs: 16), and every descriptor
 * gymrl_rollout_lunar / gymrl_rollout_lunar_mhc refuse.
 */
typedef struct {
  int P, E, cap;
  uint64_t seed; int64_t stream_id0;
  int64_t policy_stride;                   /* floats between consecutive policies' tensors; 0 with P == 1 */
  double* returns; int32_t* lengths; uint8_t* terminated;
  float* terminal_obs;                     /* f32[P * E][8] or NULL */
} gymrl_lunar_eval_args;
size_t gymrl_lunar_eval_args_bytes(void);  /* sizeof(gymrl_lunar_eval_args) */
int gymrl_lunar_policy_eval(const gymrl_lunar_eval_args* args, const gymrl_mlp_desc* policy, void* stream);
int gymrl_lunar_mhc_eval(const gymrl_lunar_eval_args* args, const struct gymrl_mhc_policy_s* policy, void* stream);
/*
 * gymrl_lunar_mlprnn_eval: the same episodes under the recurrent PPG / PPO-RNN network (gymrl_mlprnn_params, D = 8, A = 4) —
 * the eval() loop of ppg_rnn_lunarlander.py:501-524 (csrc/eval_lunar_rnn.hip).  Every episode starts from the hidden state 0,
 * which stays on chip for the whole episode; the action is gymrl_mlprnn_act's deterministic branch, the FIRST maximum of the
 * probabilities (not of the logits).  Policy p reads every pointer of `policy` p * policy_stride floats behind policy 0's.
 *   norm_stats f64 [2 + 3 * 8] per policy in RunningMeanStd.stats layout (may be NULL: the network reads raw observations):
 *     the network reads gymrl_running_norm_masked(update = 0) of every observation; policy p's stats start
 *     p * norm_stride doubles behind policy 0's (0: one set shared by all, otherwise >= 26).  terminal_obs stays raw.
 *   h_final f32 [P * E][64] (may be NULL): the hidden state after the last forward of each episode.
 * Bit-identical in actions, lengths, flags, terminal observations and h_final to the step-by-step sequence gymrl_mlprnn_act
 * (deterministic, live) -> gymrl_env_step -> gymrl_running_norm_masked(update = 0); returns are the float64 sum of the float32
 * rewards in step order.  -EINVAL before any launch: everything above that concerns `args`, a NULL policy or member, a weight
 * gymrl_mlprnn_act reads 16 bytes at a time that is not 16-byte aligned, a negative norm_stride or one in 1..25, norm_stats not
 * 8-byte or h_final not 16-byte aligned.
 */
int gymrl_lunar_mlprnn_eval(const gymrl_lunar_eval_args* args, const gymrl_mlprnn_params* policy,
                            const double* norm_stats, int64_t norm_stride, float* h_final, void* stream);
/*
 * gymrl_lunar_mlprnn_collect: one collection round of the PPG-RNN / PPO-RNN trainers (collect_round() of
 * ppg_rnn_lunarlander.py) as ONE launch of ONE workgroup (csrc/collect_lunar_rnn.hip): N <= 16 LunarLander-v3 episodes (envs
 * env_id0 + i under `seed`, episode 0, gymrl_env_reset's arithmetic) from their reset until every episode has ended or `cap`
 * steps have passed, the worlds and the GRU states (from 0) on chip throughout.  Per step t, in the loop's order: gymrl_env_step
 * under act[t] for the envs live at t; done[t] = terminated | truncated (the env's own 1000-step limit; a `cap` below it ends
 * the round without a done flag), dw[t] = terminated; ep_ret += reward in float32; gymrl_running_norm_masked(update = 1) over
 * the step's (possibly terminal) observations, live rows in env order -> states[t + 1]; gymrl_reward_scaling_masked (no done
 * flags: R is not zeroed where an episode ends) -> rew[t]; gymrl_mlprnn_act's sampling branch with counter counter0 + t + 1,
 * masked by live at t (an env whose episode just ended gets one more forward, on its terminal state: value[t + 1] is its stored
 * next value) -> act / logp / value[t + 1]; live[t + 1] = live[t] & !done[t].  Row 0 is the reset: states[0] the normalised
 * first observations, act / logp / value[0] the draw with counter0.  There is no explicit-noise input.
 *   slabs, time-major with N columns: states f32[cap + 1][N][8], act i32 / logp f32 / value f32 / live u8 [cap + 1][N],
 *   rew f32 / done u8 / dw u8 [cap][N]; a row (t, i) is written only while env i is live (live: 1 or 0 for every t reached).
 *   ep_ret f32[N] the raw return, lengths i32[N] the steps each env took.
 *   norm_stats f64[2 + 3 * 8], reward_stats f64[2 + 3] (RunningMeanStd.stats) and R f64[N] are read and updated in place.
 * Bit-identical to the step-by-step sequence above in every output.  The two statistics consume their rows one after the other
 * in env order, which one workgroup reproduces and several cannot: N <= 16 is the limit.  The workgroup leaves on one LDS word
 * behind a barrier every thread reaches, after at most cap + 1 iterations; no atomics, nothing waits for another workgroup.
 * -EINVAL before any launch: NULL args, policy, member of either or output, N outside 1..16, cap outside 1..1000, env_id0 < 0,
 * states not 16-byte, a float64 buffer not 8-byte or a 4-byte slab not 4-byte aligned, a weight gymrl_mlprnn_act reads 16 bytes
 * at a time that is not 16-byte aligned.
 */
typedef struct {
  int N, cap;
  uint64_t seed; int64_t env_id0; uint64_t counter0;
  double gamma;
  double* norm_stats; double* reward_stats; double* R;
  float* states; int32_t* act; float* logp; float* value;
  float* rew; uint8_t* done; uint8_t* dw; uint8_t* live;
  float* ep_ret; int32_t* lengths;
} gymrl_lunar_collect_args;
int gymrl_lunar_mlprnn_collect(const gymrl_lunar_collect_args* args, const gymrl_mlprnn_params* policy, void* stream);
size_t gymrl_lunar_collect_args_bytes(void);  /* sizeof(gymrl_lunar_collect_args) */

/* ------------------------------ classic-control PPO policies: whole episodes in one launch ---- */
/*
 * gymrl_lunar_policy_eval's contract for PPOTrainer on CartPole-v1, MountainCar-v0 and Acrobot-v1 (csrc/eval_classic_ppo.hip):
 * P policies x E deterministic episodes in ONE launch, the grid is P * ceil(E / 16) workgroups of 256 threads.  A workgroup
 * carries 16 episodes of one policy from the in-kernel reset to their end: lanes 0..15 of wave 0 keep the float64 env state, the
 * float64 return and the length in registers (the episode loop of gymrl_classic_policy_eval further down), all four waves run the
 * policy forward (gymrl_mlp_forward's stages; stages that only feed the value are not run), the action is the FIRST maximum of the
 * logits (gymrl_categorical_sample's deterministic branch).  No atomics, nothing waits for another workgroup, no random draw;
 * global memory is written once, when the workgroup's episodes have ended.
 *
 * env_kind is GYMRL_ENV_CARTPOLE, GYMRL_ENV_MOUNTAINCAR or GYMRL_ENV_ACROBOT; the policy is gymrl_rollout_classic's descriptor for
 * that kind (their `out` pointers are ignored).  Policy p reads every stage's W and b p * policy_stride floats behind policy 0's
 * (0: P == 1).  Episode i = p * E + e is the first episode of env stream_id0 + e under `seed` — the SAME starts for every policy,
 * env e of a gymrl_env_reset with env_id0 = stream_id0.  It ends with terminated = 1 when the env says so, with terminated = 0
 * when its length reaches `cap`.
 *
 * Outputs, each [P * E]: returns (float64: the sum of the float32 rewards in step order), lengths, terminated, final_obs
 * [P * E][D] (optional) the observation after the last step (the terminal one, not the next episode's first).  Bit-identical to
 * the step-by-step sequence gymrl_mlp_forward -> gymrl_categorical_sample(deterministic) -> gymrl_env_step.
 * -EINVAL before any launch: NULL args / policy / returns / lengths / terminated, P < 1, E < 1, P * E above INT32_MAX, cap < 1 or
 * above the kind's TimeLimit (500 / 200 / 500), stream_id0 < 0, a negative policy_stride or one that is not a multiple of 4,
 * policy_stride == 0 with P > 1, a pointer that is not aligned (returns: 8 bytes; lengths: 4; final_obs: 8), any other kind, and
 * every descriptor gymrl_rollout_classic refuses for the kind.
 */
typedef struct {
  int P, E, cap;
  int env_kind;                            /* GYMRL_ENV_CARTPOLE | GYMRL_ENV_MOUNTAINCAR | GYMRL_ENV_ACROBOT */
  uint64_t seed; int64_t stream_id0;
  int64_t policy_stride;                   /* floats between consecutive policies' tensors; 0 with P == 1 */
  double* returns; int32_t* lengths; uint8_t* terminated;
  float* final_obs;                        /* f32[P * E][D] or NULL */
} gymrl_classic_ppo_eval_args;
size_t gymrl_classic_ppo_eval_args_bytes(void);  /* sizeof(gymrl_classic_ppo_eval_args) */
int gymrl_classic_ppo_eval(const gymrl_classic_ppo_eval_args* args, const gymrl_mlp_desc* policy, void* stream);
/* gymrl_classic_ppo_eval's contract and kernel for Pendulum-v1 under the Gaussian policy: the policy is gymrl_rollout_pendulum's
 * descriptor, the action is the actor's mean (a = mu: no draw, log_std is not read), an episode ends with terminated = 0 when its
 * length reaches cap <= 200.  final_obs f32[P * E][3] (4-byte aligned).  Bit-identical to gymrl_mlp_forward ->
 * gymrl_gaussian_sample(deterministic) -> gymrl_env_step; the return is the float64 sum the stepper keeps (ep_ret). */
typedef struct {
  int P, E, cap;
  uint64_t seed; int64_t stream_id0;
  int64_t policy_stride;                   /* floats between consecutive policies' tensors; 0 with P == 1 */
  double* returns; int32_t* lengths; uint8_t* terminated;
  float* final_obs;                        /* f32[P * E][3] or NULL */
} gymrl_pendulum_ppo_eval_args;
size_t gymrl_pendulum_ppo_eval_args_bytes(void);  /* sizeof(gymrl_pendulum_ppo_eval_args) */
int gymrl_pendulum_ppo_eval(const gymrl_pendulum_ppo_eval_args* args, const gymrl_mlp_desc* policy, void* stream);

/* ================================================ low-latency Linear layers == */
/*
 * D2 / A2 / T1 update path and the vectorised acting forward of the off-policy trainers: every
 * nn.Linear (+ ReLU / Tanh / clamp) of QNetwork dqn_cartpole.py:56-65, DuelingNoisyNetwork
 * rainbow_dqn_cartpole.py:97-113, Actor / Critic sac_pendulum.py:49-125, td3_pendulum.py:49-83,
 * ddpg_pendulum.py:37-48, sac_cartpole.py:47-70 — forward as called in update() / select_action(), and the
 * backward loss.backward() runs through it.  The reference issues a GEMM, a bias add, an activation, and in
 * backward an activation-gradient, two GEMMs and a bias reduction per layer; here a layer is ONE launch per
 * direction (csrc/lin.hip: one wavefront per 16-row output tile, v_mfma_f32_16x16x4_f32, operands from L2),
 * for batches up to a few thousand rows.  Up to GYMRL_LIN_MAX_ITEMS layers of one shape share a launch
 * (twin critics, mean / log_std heads, online + target network); the activation is per item.
 *
 *   fwd         y  = act(cat(x, x2) w^T + b)       x [B, K1] (row stride ldx), x2 [B, K - K1] (ldx2; K1 == K: unused),
 *                                                  w [N, K] row-major = nn.Linear.weight, b [N] or NULL, y [B, N] (ldy)
 *   bwd_input   (dx | dx2) (+)= (dy * act'(y)) w   dy, y [B, N] (ldy); dx [B, K1] (lddx), dx2 [B, K - K1] (lddx2);
 *                                                  a NULL dx / dx2 skips that part (at least one is required);
 *                                                  sum_items != 0: ONE result, the sum over the items (layers fed by the
 *                                                  same input), written to item 0's dx / dx2
 *   bwd_weight  dw (+)= (dy * act'(y))^T cat(x, x2),  db (+)= column sums of dy * act'(y)   (db NULL: skipped)
 *
 * act' is taken from the saved OUTPUT y: ReLU y > 0; Tanh 1 - y^2 (tanh = 1 - 2/(exp(2z)+1) on the exp2/rcp
 * units, as in gymrl_linear_fwd); clamp(lo, hi) lo < y < hi (torch passes the gradient AT the bounds as well — a
 * measure-zero difference).  accumulate != 0 adds to the destination (torch's .grad +=).  Sums are f32 fma chains
 * in the order given at the top of csrc/lin.hip; bwd_weight cuts B > 512 into <= 16 row slices whose partial
 * results are added in slice order by a second launch (workspace: gymrl_lin_workspace_bytes, else NULL).
 * Compared with torch float64 at 1e-5 relative (tests/test_lin_gpu.py), not bit for bit.
 */
#define GYMRL_LIN_MAX_ITEMS 4
typedef struct {
  const float* x;
  const float* x2;
  const float* w;
  const float* b;
  float* y;           /* fwd: output; bwd: the saved output (NULL allowed when act == GYMRL_ACT_NONE) */
  const float* dy;
  float* dx;
  float* dx2;
  float* dw;
  float* db;
  int act;            /* GYMRL_ACT_*; clamp bounds in lo / hi */
  float lo, hi;
  int32_t* argmax;    /* fwd with GYMRL_ACT_DUELING only: NULL, or i32[B] = first index of the row maximum of q (the greedy
                         action, torch.argmax's tie rule) */
} gymrl_lin_item;
size_t gymrl_lin_workspace_bytes(int B, int N, int K, int n_items);
int gymrl_lin_fwd(const gymrl_lin_item* items, int n_items, int B, int K, int K1, int N, int ldx, int ldx2, int ldy,
                  void* stream);
int gymrl_lin_bwd_input(const gymrl_lin_item* items, int n_items, int B, int N, int K, int K1, int ldy, int lddx,
                        int lddx2, int accumulate, int sum_items, void* stream);
int gymrl_lin_bwd_weight(const gymrl_lin_item* items, int n_items, int B, int N, int K, int K1, int ldy, int ldx,
                         int ldx2, int accumulate, void* workspace, void* stream);

/*
 * gymrl_lin_fwd with act == GYMRL_ACT_DUELING (N = A + 1 <= 16 stacked rows: A advantage rows, then the value row)
 * writes q [B, A] = value + advantage - mean(advantage) — DuelingNoisyNetwork.forward rainbow_dqn_cartpole.py:108-113 —
 * instead of the N raw columns; gymrl_dueling_bwd maps dq [B, A] back to the stacked dS [B, A + 1].
 *
 * NoisyLinear (rainbow_dqn_cartpole.py:60-95): gymrl_noisy_combine stacks the effective parameters of up to
 * GYMRL_NOISY_MAX_LAYERS layers that share K — W[row] = w_mu + w_sigma * w_eps, b likewise (training == 0: mu only) —
 * into W_out [sum n_out, K] / b_out [sum n_out] and copies the noise through to w_eps_copy / b_eps_copy (the
 * module's weight_epsilon / bias_epsilon buffers) when given; gymrl_noisy_split sends the stacked gradient back:
 * d mu (+)= dW, d sigma (+)= dW * eps (zeros when training == 0; NULL d*_sigma: skipped).
 */
#define GYMRL_NOISY_MAX_LAYERS 8
typedef struct {
  const float* w_mu; const float* w_sigma; const float* w_eps;      /* [n_out, K] */
  const float* b_mu; const float* b_sigma; const float* b_eps;      /* [n_out] */
  float* w_eps_copy; float* b_eps_copy;                             /* combine only, NULL: no copy */
  float* dw_mu; float* dw_sigma; float* db_mu; float* db_sigma;     /* split only */
  uint64_t seed, counter;                                           /* combine with draw != 0 */
  const uint64_t* counter_dev;                                      /* NULL, or the counter in device memory (graphs) */
  int draw;            /* combine: draw this layer's noise in the launch itself — bit for bit gymrl_noisy_noise(seed,
                          counter) — instead of reading w_eps / b_eps; it is written to w_eps_copy / b_eps_copy when given */
  int eval;            /* combine: this layer contributes its mu only even when training != 0 (a target network's layer
                          stacked beside training-mode ones) */
  int n_out;
} gymrl_noisy_layer;
int gymrl_noisy_combine(const gymrl_noisy_layer* layers, int n_layers, int K, int training, float* W_out, float* b_out,
                        void* stream);
int gymrl_noisy_split(const gymrl_noisy_layer* layers, int n_layers, int K, int training, const float* dW, const float* db,
                      int accumulate, void* stream);
/* MFMA-operand images of a square Linear weight W [H][H] (H % 16 == 0), csrc/lin_device.hpp: the forward operand (lane (r, q) of
 * (tile t, step c) holds W[16t + r][16c + 4q .. + 3]) and the input-gradient operand (W[16c + 4q .. + 3][16t + r]), one contiguous
 * 1 KiB block per wave-wide load — what a slab kernel streams 2-3x faster than nn.Linear's rows.  Either output may be NULL. */
typedef struct { const float* W; int H; float* img_fwd; float* img_bwd; } gymrl_weight_image;
#define GYMRL_NOISY_MAX_IMAGES 4
/* gymrl_noisy_combine and, on extra workgroups of the SAME launch, n_images (<= GYMRL_NOISY_MAX_IMAGES) weight images rebuilt from
 * the parameters as they are: Rainbow's vector step has this launch between the optimiser step and the acting forward anyway. */
int gymrl_noisy_combine_images(const gymrl_noisy_layer* layers, int n_layers, int K, int training, float* W_out, float* b_out,
                               const gymrl_weight_image* images, int n_images, void* stream);
int gymrl_dueling_bwd(const float* dq, int B, int A, float* dS_out, void* stream);

/* ================================================ mHC backbone ============== */
/*
 * F1: ManifoldHyperConnectionFuse.gates + MHCBlock._sub + RMSNorm of PPO-full's network — ppo_full_lunarlander.py:106-194
 * (gates :125-147, sub-block :160-165), RMSNorm :96-104, MHCBackbone.forward :178-183 — as called from get_action :395-407 /
 * get_value once per env step and from the minibatch passes of update_model :537-660.  The reference issues ~95 torch launches per
 * hyper-connection; here a sub-block's forward is gymrl_mhc_gates + gymrl_lin_fwd + gymrl_mhc_combine.
 *   gymrl_mhc_gates: h [B, n, D] (n = 2 or 4 branches) -> pre [B, n] = sigmoid(r H[:n] a0 + beta), post [B, n] =
 *     2 sigmoid(r H[n:2n] a1 + beta), mix [B, n, n] = u A v with A = exp(r H[2n:] a2 + beta) and u, v from sk_it
 *     Sinkhorn-Knopp sweeps, where H = (norm_w * flat) w, r = 1 / (|flat| / sqrt(nD) + 1e-6); read [B, D] = sum_i pre_i h_i.
 *     norm_w [nD] = fuse.norm.weight, w [nD, n*n + 2n], alpha [3], beta [n*n + 2n].  stats_out (nullable; n = 2 and
 *     n*D = 256 or 512 only): f32[B, 9] = the row's eight read-out sums H and |flat|^2, the input of gymrl_mhc_gates_bwd.
 *   gymrl_mhc_combine: h_out[b, i, :] = post[b, i] o[b, :] + sum_j mix[b, i, j] h[b, j, :], o = out (act = GYMRL_ACT_NONE) or
 *     SiLU(out) (GYMRL_ACT_SILU: `out` is the Linear's raw output, the training pass keeps it for the backward).
 *   gymrl_rmsnorm: y [B, D] = s rsqrt(mean(s^2) + eps) w, s = the sum of the row's n_sum consecutive [D] blocks
 *     (n_sum = n: final_norm(h.sum(1)); 1: the MLPs' RMSNorm), through SiLU first when act = GYMRL_ACT_SILU
 *     (the MLPs' Linear -> SiLU -> RMSNorm :371-402).
 * Floating point, compared with the torch modules at 1e-5 (tests/test_mhc_fused_gpu.py).
 */
int gymrl_mhc_gates(const float* h, const float* norm_w, const float* w, const float* alpha, const float* beta, int B, int n,
                    int D, int sk_it, float* pre_out, float* post_out, float* mix_out, float* read_out, float* stats_out,
                    void* stream);
int gymrl_mhc_combine(const float* post, const float* mix, const float* out, const float* h, int B, int n, int D, int act,
                      float* h_out, void* stream);
int gymrl_rmsnorm(const float* x, const float* w, int B, int D, int n_sum, float eps, int act, float* y, void* stream);
/* Backward of gymrl_rmsnorm (n_sum = 1, D <= 512): g = dL/dy -> d_x [B, D] (dL/dx, through SiLU' when act = GYMRL_ACT_SILU)
 * and d_w [D] (overwritten; per-workgroup partial sums in `workspace`, gymrl_rmsnorm_bwd_workspace_bytes, added in a fixed
 * order — no atomics). */
size_t gymrl_rmsnorm_bwd_workspace_bytes(int D);
int gymrl_rmsnorm_bwd(const float* g, const float* x, const float* w, int B, int D, float eps, int act, float* d_x, float* d_w,
                      void* workspace, void* stream);
/* The same for the norm of a branch sum (final_norm(h.sum(dim=1)), MHCBackbone.forward :243): x [B, n_sum, D], d_x [B, D] is
 * the gradient of EVERY block (the sum hands each the same one — the caller broadcasts it, nothing is materialised). */
int gymrl_rmsnorm_sum_bwd(const float* g, const float* x, const float* w, int B, int D, int n_sum, float eps, int act, float* d_x,
                          float* d_w, void* workspace, void* stream);
/* A head's tail in one launch each way: out [B, n_out] = RMSNorm(SiLU(x)) W2^T + b2 for x [B, D], D <= 256, n_out <= 8
 * (MLP([128, 256, n_out]) :371-402: the actor's and the critic's Linear -> SiLU -> RMSNorm -> Linear; b2 may be NULL), and its
 * backward from d_out [B, n_out]: d_x [B, D], d_norm_w [D], d_W2 [n_out, D], d_b2 [n_out] (overwritten; per-workgroup partial
 * sums in `workspace`, added in a fixed order).  The normalised activations and their gradient never touch HBM.
 * The kernel (one row or four rows per wave, i.e. the summation order) is chosen by (D, n_out) ALONE: at D = 256 x, norm_w, W2
 * (and d_x, n_out = 1) must be 16-byte aligned — -22 otherwise; a result's bits never depend on where a buffer starts. */
int gymrl_norm_proj_fwd(const float* x, const float* norm_w, const float* W2, const float* b2, int B, int D, int n_out, float eps,
                        float* out, void* stream);
size_t gymrl_norm_proj_bwd_workspace_bytes(int D, int n_out);
int gymrl_norm_proj_bwd(const float* d_out, const float* x, const float* norm_w, const float* W2, int B, int D, int n_out, float eps,
                        float* d_x, float* d_norm_w, float* d_W2, float* d_b2, void* workspace, void* stream);
/* The Sinkhorn-Knopp sweeps alone (:141-146; constants of the backward pass in the reference): A f32[B, n, n] > 0 ->
 * u [B, n], v [B, n] after sk_it sweeps u = 1/(A v + 1e-8), v = 1/(A^T u + 1e-8) from u = v = 1 — for gate shapes
 * gymrl_mhc_gates_bwd does not cover, whose other gate operations stay with autograd. */
int gymrl_sinkhorn(const float* A, int B, int n, int sk_it, float* u_out, float* v_out, void* stream);
/* Training pass of MHCBlock._sub (:160-165): the branch products' backward (autograd wraps them:
 * gymrl_amd/ppo_full_lunarlander.py _MhcSub; _MhcRead / _MhcCombine for the shapes it does not cover).
 *   read_fwd:     read [B, D] = sum_i pre[b, i] h[b, i, :]
 *   read_bwd:     d_pre [B, n] = sum_d g[b, d] h[b, i, d];  d_h [B, n, D] (+)= pre[b, i] g[b, d]   (d_h NULL: d_pre only)
 *   combine_bwd (forward = gymrl_mhc_combine with the same act), g = dL/dh' [B, n, D]:
 *                 d_post [B, n], d_mix [B, n, n], d_out [B, D] (act = GYMRL_ACT_SILU: `out` is the raw Linear output z and
 *                 d_out is dL/dz), d_h [B, n, D] = mix^T g (overwritten; NULL: left to gymrl_mhc_gates_bwd's g_out term) */
/* Backward of the gates (n = 2, n*D = 256 or 512; forward = gymrl_mhc_gates with stats_out): given dL/d pre, post, mix — u, v of
 * the Sinkhorn sweeps are constants, as in the reference — writes d_h [B, n, D] (overwritten) and the parameter gradients
 * d_norm_w [nD], d_w [nD, n*n + 2n], d_alpha [3], d_beta [n*n + 2n] (overwritten; sums over rows in a fixed order:
 * per-workgroup partial vectors in `workspace`, gymrl_mhc_gates_bwd_workspace_bytes, added ascending — no atomics).
 * d_read (nullable, [B, D]) and g_out (nullable, [B, n, D]) fold the sub-block's other two paths into d_h in the same pass:
 * d_h[b, j] += pre[b, j] d_read[b] (the read's backward) + sum_i mix[b, i, j] g_out[b, i] (the combine's), so that the three
 * consumers of h produce ONE gradient tensor and autograd adds nothing. */
size_t gymrl_mhc_gates_bwd_workspace_bytes(int n, int D);
int gymrl_mhc_gates_bwd(const float* h, const float* norm_w, const float* w, const float* alpha, const float* pre, const float* post,
                        const float* mix, const float* stats, const float* d_pre, const float* d_post, const float* d_mix,
                        const float* d_read, const float* g_out, int B, int n, int D, float* d_h, float* d_norm_w, float* d_w,
                        float* d_alpha, float* d_beta, void* workspace, void* stream);
int gymrl_mhc_read_fwd(const float* pre, const float* h, int B, int n, int D, float* read_out, void* stream);
int gymrl_mhc_read_bwd(const float* g, const float* pre, const float* h, int B, int n, int D, float* d_pre, float* d_h,
                       int accumulate, void* stream);
int gymrl_mhc_combine_bwd(const float* g, const float* post, const float* mix, const float* out, const float* h, int B, int n, int D,
                          int act, float* d_post, float* d_mix, float* d_out, float* d_h, void* stream);

/* Training pass: the forward of one hyper-connection sub-block (MHCBlock._sub :160-165 with the gates :125-147) in ONE launch for
 * n = 2 branches of D = 128: h [B, 2, 128] -> h_out = post (x) SiLU(z) + mix h with z = read lin_w^T + lin_b, read = sum_i pre_i h_i,
 * and everything the backward takes: pre_out [B, 2], post_out [B, 2], mix_out [B, 2, 2], stats_out [B, 9] (as gymrl_mhc_gates),
 * read_out [B, 128], z_out [B, 128].  h_broadcast != 0: h is [B, 128], the same row for both branches (the first sub-block's
 * input is the input projection repeated, MHCBackbone.forward :239: no [B, 2, 128] copy is made of it).  The same values as gymrl_mhc_gates + gymrl_lin_fwd + gymrl_mhc_combine(GYMRL_ACT_SILU) up to
 * the order of the Linear's sums; 16-row tiles per wave, the weights staged in LDS once per workgroup. */
int gymrl_mhc_sub_forward(const float* h, int h_broadcast, const float* norm_w, const float* w, const float* alpha, const float* beta,
                          const float* lin_w, const float* lin_b, int B, int n, int D, int sk_it, float* pre_out, float* post_out,
                          float* mix_out, float* stats_out, float* read_out, float* z_out, float* h_out, void* stream);
/* Training pass: the backward of the same sub-block in ONE launch (+ the fixed-order reduction of the parameter partials).
 * Inputs: the upstream gradient g [B, 2, 128] (g_broadcast != 0: [B, 128], the same row for both branches — the final norm's
 * d x), the saved h [B, 2, 128] (h_broadcast != 0: [B, 128], the repeated input of the first sub-block), z, pre, post, mix, stats.
 * Outputs: d_z [B, 128] = dL/dz (what gymrl_lin_bwd_weight takes with `read` for the Linear's d W, d b), d_h [B, 2, 128] — the
 * gates', the read's and the combine's paths into h added (sum_branches != 0: [B, 128], the two branches' gradients added:
 * the gradient of a repeated row), d_norm_w [256], d_w [256, 8], d_alpha [3], d_beta [8].  d_z and d_h must have room for
 * ceil(B / 16) * 16 rows: the kernel writes whole 16-row tiles (rows past B hold unspecified values).  workspace:
 * gymrl_mhc_gates_bwd_workspace_bytes(2, 128).  The values of gymrl_mhc_combine_bwd + gymrl_linear_bwd_input +
 * gymrl_mhc_read_bwd + gymrl_mhc_gates_bwd up to the order of the sums (float64 autograd at 3e-5: tests/test_mhc_fused_gpu.py);
 * g and h cross HBM once instead of three times. */
int gymrl_mhc_sub_backward(const float* g, int g_broadcast, const float* h, int h_broadcast, const float* z, const float* pre,
                           const float* post, const float* mix, const float* stats, const float* norm_w, const float* w,
                           const float* alpha, const float* lin_w, int B, int n, int D, float* d_z, float* d_h, int sum_branches,
                           float* d_norm_w, float* d_w, float* d_alpha, float* d_beta, void* workspace, void* stream);
/* The whole rollout forward of PPO-full's network (ActorCritic.forward :377-407 as called by get_action / get_value) in ONE
 * launch, for the reference's default shape: n = 2 branches of D = 128 (mhc_rate, mhc_dim), 256-wide heads
 * (MLP([128, 256, n_out]) :371-402), obs_dim <= 16, n_act <= 8, n_sub = 2 * mhc_layers <= 8 sub-blocks.  Rows are
 * independent, so 16 of them travel through every layer inside one workgroup (branch stack in registers, the Linears on
 * v_mfma_f32_16x16x4_f32).  Pointers are the modules' own parameters (nn.Linear layout [out, in]); logits_out [B, n_act],
 * value_out [B].  Same values as the per-layer entry points above to 1e-5 (tests/test_mhc_fused_gpu.py). */
typedef struct {
  const float* norm_w;   /* fuse.norm.weight [256] */
  const float* w;        /* fuse.w [256, 8] */
  const float* alpha;    /* [3] */
  const float* beta;     /* [8] */
  const float* lin_w;    /* the sub-block's Linear [128, 128] */
  const float* lin_b;    /* [128] */
} gymrl_mhc_sub;
typedef struct {
  const float* w1;       /* mlp.0.weight [256, 128] */
  const float* b1;       /* [256] */
  const float* norm_w;   /* mlp.2.weight [256] */
  float norm_eps;
  const float* w2;       /* mlp.3.weight [n_out, 256] (n_out = n_act for head 0, 1 for head 1) */
  const float* b2;       /* [n_out] */
} gymrl_mhc_head;
typedef struct gymrl_mhc_policy_s {
  int obs_dim, n_sub, n_act, sk_it;
  const float* in_w;     /* input_proj.weight [128, obs_dim] */
  const float* in_b;     /* [128] */
  gymrl_mhc_sub sub[8];
  const float* final_norm_w;   /* [128] */
  float final_norm_eps;
  gymrl_mhc_head head[2];      /* 0 = actor, 1 = critic */
  const float* image;          /* NULL: every weight is read in place.  Else gymrl_mhc_policy_pack's output (16-byte aligned,
                                * gymrl_mhc_policy_image_floats(n_sub) floats): the sub-blocks' Linears and gate weights and the heads'
                                * first Linears in the order the kernel's lanes read them — one contiguous KiB per wave-wide load
                                * instead of a 64-byte piece of sixteen rows; repack after the parameters change.  Same values. */
} gymrl_mhc_policy;
size_t gymrl_mhc_policy_image_floats(int n_sub);
int gymrl_mhc_policy_pack(const gymrl_mhc_policy* p, float* image, void* stream);      /* p->image is ignored */
int gymrl_mhc_policy_forward(const gymrl_mhc_policy* p, const float* obs, int B, float* logits_out, float* value_out, void* stream);

/* ===================================================== MLP update path ===== */
/*
 * The HBM-bound passes of one ActorCritic minibatch update around the library GEMMs —
 * ppo_lunarlander.py:274-307: evaluate_actions' forward :110-117 (shared/actor/critic
 * Sequentials :67-84) and loss.backward() :303.  Activations are row-major f32 [B, C],
 * C a power of two in 16..256.  workspace: gymrl_mlp_train_workspace_bytes(C, D, A) bytes.
 * Column reductions are deterministic (fixed-order f64 finalize over per-workgroup partials).
 *
 *   linear_tanh_smallk : out = tanh(x W^T + b), x [B, D], W [C, D], D in {2,3,4,6,8}
 *                        (shared.0: Linear(obs, hidden) + Tanh)
 *   tanh_inplace       : z <- tanh(z + bias[col]) on n floats = rows of C columns (bias NULL: none) after a
 *                        library GEMM; the bias rides on this pass, the GEMM runs without an epilogue
 *   tanh_bwd_colsum    : dH <- dH * (1 - H^2) in place; colsum_out[c] = sum_r dH[r][c]
 *                        (Tanh backward + the bias gradient of the Linear below it)
 *   linear_smallk_bwd  : dZ = dH * (1 - H^2) (never stored); dW [C, D] = dZ^T x; db [C] = colsum dZ.
 *                        W, b non-NULL (the layer's own weight [C, D] / bias): H is not read (may be NULL) —
 *                        H = tanh(x W^T + b) is recomputed exactly as linear_tanh_smallk computed it
 *   heads_fwd_tanh     : Zac [B, 2C] = pre-activations of actor.0 | critic.0 (one N = 2C GEMM; their biases
 *                        bac [2C] are added here, NULL if the GEMM already did) -> Hac = tanh(Zac + bac) in place AND logits [B, A] = Ha Wa2^T + ba2,
 *                        value [B] = Hc Wc2^T + bc2 from the tanh values still in registers
 *                        (actor.0/critic.0's Tanh + actor.2 + critic.2 forward in one pass).
 *                        store_h == 0: Zac is NOT rewritten (it keeps the pre-activations; 2 KB/row less HBM
 *                        traffic) — then call heads_bwd with pre_activation = 1, which recomputes the same tanh
 *   heads_bwd          : Hac [B, 2C] = [Ha | Hc], the Tanh outputs of actor.0 / critic.0;
 *                        dlogits [B, A] (A in {2,4}), dv [B] from gymrl_ppo_loss_fwd_bwd;
 *                        Wa2 [A, C] = actor.2.weight, Wc2 [1, C] = critic.2.weight.  Writes
 *                        dZac [B, 2C] = [(dlogits Wa2)(1 - Ha^2) | (dv Wc2)(1 - Hc^2)],
 *                        dbac [2C] = colsum dZac, dWa2 = dlogits^T Ha, dba2 = colsum dlogits,
 *                        dWc2 = dv^T Hc, dbc2 = sum dv — one pass over Hac instead of four
 *                        skinny GEMMs, two tanh' passes and four reductions.
 *                        pre_activation != 0: `Hac` holds the pre-activations instead and the kernel applies
 *                        tanh(. + bac[col]) (bac NULL: no bias) first — bit for bit the forward's values
 * tanh here (and in gymrl_linear_fwd's epilogue) is 1 - 2/(exp(2x)+1) on the hardware exp2/rcp units:
 * device-deterministic, absolute error < 2e-7, exact +-1 limits; compared with torch at 1e-5, not bit for bit.
 * linear_smallk_bwd with H == NULL and W == NULL takes dH as dZ itself (the tanh' factor was applied upstream,
 * gymrl_linear_bwd_input).
 */
size_t gymrl_mlp_train_workspace_bytes(int C, int D, int A);
int gymrl_linear_tanh_smallk(const float* x, const float* W, const float* b, int64_t B, int D, int C,
                             float* out, void* stream);
/* The same launch without the tanh: out [B, C] = x [B, D] W[C, D]^T + b (D in {2, 3, 4, 6, 8}, C a power of two >= 4), one fmaf chain
 * per output in ascending d — PPO-full's input projection (ppo_full_lunarlander.py:236: Linear(obs, 128)) at 524 288-row
 * micro-batches, where the 16 x 16-tile layer kernel writes its 268 MB in 64-byte pieces (152 us; this one: 16-byte stores). */
int gymrl_linear_smallk(const float* x, const float* W, const float* b, int64_t B, int D, int C, float* out, void* stream);
int gymrl_tanh_inplace(float* z, int64_t n, const float* bias, int C, void* stream);
int gymrl_tanh_bwd_colsum(float* dH, const float* H, int64_t B, int C, float* colsum_out,
                          void* workspace, void* stream);
int gymrl_linear_smallk_bwd(const float* dH, const float* H, const float* x, int64_t B, int D, int C,
                            float* dW, float* db, const float* W, const float* b, void* workspace,
                            void* stream);
int gymrl_heads_fwd_tanh(float* Zac, int64_t B, int C, int A, const float* bac, const float* Wa2,
                         const float* ba2, const float* Wc2, const float* bc2, float* logits, float* value,
                         int store_h, void* stream);
int gymrl_heads_bwd(const float* Hac, const float* dlogits, const float* dv, int64_t B, int C, int A,
                    const float* Wa2, const float* Wc2, float* dZac, float* dbac, float* dWa2,
                    float* dba2, float* dWc2, float* dbc2, int pre_activation, const float* bac,
                    void* workspace, void* stream);

/*
 * heads_loss_fwd_bwd : gymrl_heads_fwd_tanh + gymrl_ppo_loss_fwd_bwd + gymrl_heads_bwd as ONE pass over
 *   Zac [B, 2C] (C in {64, 128, 256}, A in {2, 3, 4}): per row tanh(Zac + bac), logits / value from the two heads, the clipped-surrogate loss of
 *   ppo_lunarlander.py:278-300 (advantage normalised on load from adv_moments as in gymrl_ppo_loss_fwd_bwd; act /
 *   logp_old / adv / ret are the minibatch's rows in order, i.e. already gathered), and the heads' backward: dZac
 *   overwrites Zac in place; dbac [2C], dWa2 [A, C], dba2 [A], dWc2 [C], dbc2 [1] as gymrl_heads_bwd.
 *   metric_parts: f64[gymrl_heads_loss_blocks(B, C)][5] block partials of (policy loss, value loss, entropy,
 *   clip fraction, approx KL) sums — reduce with gymrl_reduce_rows.  Same arithmetic per row as the three
 *   separate passes (one shared device function each), so gradients and metrics are bit-identical to them.
 */
/* (gradient outputs: all five non-NULL, or all five NULL = "block partials only": they stay in `workspace` for
 *  gymrl_update_finalize below; gymrl_linear_smallk_bwd takes dW = db = NULL and gymrl_linear_bwd_weight dW = NULL the same way) */
int gymrl_heads_loss_blocks(int64_t B, int C);
/* 1 where the fused PPO update (ppo_net.FusedActorCriticUpdate) covers an ActorCritic of hidden width C, observation width D
 * and A actions: C in {64, 128, 256}, D in {2, 3, 4, 6, 8}, A in {2, 3, 4}; 0 otherwise.  Host only.  (A = 3 takes
 * gymrl_heads_loss_fwd_bwd at every width: gymrl_heads_bwd stays A in {2, 4}.) */
int gymrl_ppo_update_shape_ok(int C, int D, int A);
int gymrl_heads_loss_fwd_bwd(float* Zac, int64_t B, int C, int A, const float* bac, const float* Wa2,
                             const float* ba2, const float* Wc2, const float* bc2, const int32_t* act,
                             const float* logp_old, const float* adv, const float* ret,
                             const double* adv_moments, const gymrl_ppo_cfg* cfg, float* dbac, float* dWa2,
                             float* dba2, float* dWc2, float* dbc2, double* metric_parts, void* workspace,
                             void* stream);
/*
 * The same ONE pass under the Gaussian policy ("Gaussian policy" above; ppo_net.FusedGaussianUpdate): the actor head's A sums
 * plus ba2 are the mean mu[A], log_std f32[A] is read from device memory, act f32[B, A] holds the minibatch's stored actions in
 * order, and a row's loss and gradients are gymrl_ppo_gauss_loss_fwd_bwd's, bit for bit (one shared device function).  Layout,
 * the advantage normalisation from adv_moments, dZac in place, the five head gradients, `workspace`
 * (gymrl_mlp_train_workspace_bytes(C, D, A)) and metric_parts f64[gymrl_heads_loss_blocks(B, C)][5] are
 * gymrl_heads_loss_fwd_bwd's.  The five head gradients and dlog_std_out f32[A] are all required (written, not accumulated):
 * there is no "block partials only" mode, gymrl_update_finalize stays the categorical head's.  No host synchronisation, no
 * float atomics, capturable in a hipGraph.
 * dlog_std is a fixed-order reduction whose order depends on B and C alone.  With rpw = 256 / C rows per wave-load, rows
 * [8 rpw j, 8 rpw j + 8 rpw) are batch j (32 / 16 / 8 rows at C = 64 / 128 / 256) and row 8 rpw j + l sits in lane l of the wave
 * that walks the batch.  A row's float32 term (g_lp * (z_k * z_k - 1.0f) + g_H) is widened to float64; lanes without a row hold
 * 0.0; the wave's 64 lanes are added by the halving tree v[l] += v[l + off], off = 32, 16, .. 1, and lane 0's sum is stored to
 * dls_workspace f64[ceil(B / (8 rpw))][A] (gymrl_gauss_heads_loss_workspace_bytes(B, C, A) bytes, 8-byte aligned) at row j —
 * by the batch's number, whichever wave of whichever workgroup walked it.  A second launch of ONE workgroup then adds the
 * batches: thread t of 256 adds batches t, t + 256, t + 512, .. in ascending order, a wave's 64 threads are added by the same
 * halving tree, the four waves' sums are added in order 0, 1, 2, 3, and the result is rounded to float32 once.
 * grid_blocks: 0 = gymrl_heads_loss_blocks(B, C) workgroups; a smaller positive value narrows the grid (tests; a larger one is
 * the default).  The batches are dealt to gymrl_heads_loss_blocks(B, C) virtual workgroups whatever the grid, and a workgroup of
 * a narrower grid runs several of them one after the other, each to its own partial row and metric row: dZac, the six
 * gradients and every row of metric_parts carry the same bits under every grid.
 * -22 before any launch: C not in {64, 128, 256}, A != 1, B <= 0, grid_blocks < 0, Zac (or a given bac) off 16 bytes,
 * metric_parts or dls_workspace off 8 bytes, or a NULL among Zac, Wa2, Wc2, log_std, act, logp_old, adv, ret, cfg, the six
 * gradient outputs, metric_parts, workspace, dls_workspace (bac, ba2, bc2 and adv_moments may be NULL).
 * gymrl_ppo_gauss_update_shape_ok: 1 where that update covers a GaussianActorCritic of hidden width C, observation width D and
 * A action components: C in {64, 128, 256}, D in {2, 3, 4, 6, 8}, A == 1; 0 otherwise.  Host only.  gymrl_ppo_update_shape_ok and
 * the categorical entry points answer A = 1 as they always did.
 */
int gymrl_ppo_gauss_update_shape_ok(int C, int D, int A);
size_t gymrl_gauss_heads_loss_workspace_bytes(int64_t B, int C, int A);
int gymrl_gauss_heads_loss_fwd_bwd(float* Zac, int64_t B, int C, int A, const float* bac, const float* Wa2,
                                   const float* ba2, const float* Wc2, const float* bc2, const float* log_std,
                                   const float* act, const float* logp_old, const float* adv, const float* ret,
                                   const double* adv_moments, const gymrl_ppo_cfg* cfg, float* dbac, float* dWa2,
                                   float* dba2, float* dWc2, float* dbc2, float* dlog_std_out, double* metric_parts,
                                   void* workspace, void* dls_workspace, int grid_blocks, void* stream);

/* ===================================================== update-path GEMMs === */
/*
 * The 256-wide contractions of one ActorCritic minibatch update — ppo_lunarlander.py:274-307:
 * shared.2 / actor.0 / critic.0 of evaluate_actions' forward (:67-84, :110-117) and their
 * input / weight gradients under loss.backward() (:303) — as hand-written exact-f32 MFMA kernels
 * (v_mfma_f32_32x32x2_f32: f32 in, f32 accumulate, bit for bit an fmaf chain; the reference computes
 * in f32 and gfx950 has no TF32) with the layer's elementwise work in the epilogue.  Row-major f32,
 * K = 256 (hidden_dim), B rows.  workspace: gymrl_gemm_workspace_bytes() bytes, 16-B aligned.
 *
 *   linear_fwd         Y [B, N] = act(X [B, K] W[N, K]^T + b[N]);  N in {256, 512}; act 0 none, 1 tanh
 *                      (b NULL: no bias).  Linear + Tanh of shared.2 (N = 256) and of actor.0 | critic.0
 *                      as one N = 512 layer over their adjacent weights.
 *   linear_bwd_input   dX [B, K] = (dY [B, N] W[N, K]) * (1 - H^2), H [B, K] = the tanh output of the layer
 *                      BELOW (H NULL: no factor).  N in {256, 512}.  (The bias gradient of the layer below —
 *                      the column sums of dX — comes out of that layer's linear_bwd_weight as `db`.)
 *   linear_bwd_weight  dW [N, K] = dY [B, N]^T X [B, K];  N in {256, 512}.
 *
 * Accumulation order (part of the contract — oracle/gymrl_oracle.c restates it and tests compare bit for
 * bit).  fwd / bwd_input: one fmaf chain per output from +0 over the reduction index r in chunks of 8
 * ascending, inside a chunk in the order 0, 4, 1, 5, 2, 6, 3, 7; bias / factor applied after the chain in
 * f32 ((acc + b), acc * (1 - h*h)).  bwd_weight: the rows are cut into `slices` slices of
 * `rows_per_slice` rows (gymrl_linear_bwd_weight_geometry); inside a slice one fmaf chain from +0 over
 * the rows ascending; dW = ((g0 + g1) + g2) + g3 in f64, g_j = the f64 sum of the slice results s = j
 * (mod 4) ascending, rounded once to f32.  act = tanh uses the same hardware-exp2 form as the passes above.  bwd_weight's db [N]
 * (NULL: skipped) = column sums of dY — the bias gradient of the same layer: per slice the even- and the odd-offset
 * rows are summed sequentially in f32 and added, slices combine like the weight tiles (bit for bit in the oracle).
 * gymrl_gemm_config(key, value) exists ONLY in the probe build (make -C gymrl_amd/csrc prof -> libgymrl_hip_prof.so,
 * -DGYMRL_PROF_BUILD): it selects timing-only ablation variants of the kernels for tools/abl_gemm.py (4: bwd_weight,
 * 5: fwd; 0 = the product kernel).  The product library exports no such switch and keeps no mutable global state.
 */
size_t gymrl_gemm_workspace_bytes(void);
#ifdef GYMRL_PROF_BUILD
int gymrl_gemm_config(int key, int value);
#endif
int gymrl_linear_fwd(const float* X, const float* W, const float* b, int64_t B, int K, int N, int act,
                     float* Y, void* stream);
int gymrl_linear_bwd_input(const float* dY, const float* W, const float* H, int64_t B, int N, int K,
                           float* dX, void* stream);
/* dX [B, K] = G + dY W for the (N, K) = (256, 128) layer: the input gradient of a SECOND Linear on the same input added to the
 * first one's in the GEMM's epilogue (PPO-full's actor and critic heads both read the backbone's output: the separate add was a
 * 0.8 GB pass per 524 288-row micro-batch).  Same sums as gymrl_linear_bwd_input followed by G + . ; G may not alias dX. */
int gymrl_linear_bwd_input_add(const float* dY, const float* W, const float* G, int64_t B, int N, int K, float* dX, void* stream);
/* How the row-streaming kernels behind linear_fwd (kind 0), linear_bwd_input (1) and linear_bwd_input_add (2) cut B rows, for
 * the kernel the entry picks at (K, N) — host only, nothing is launched.  The launch has `row_groups` row groups of four waves;
 * a wave owns rows_per_round / 4 rows at a time, and row group g's loop iteration j covers the rows from
 * (g + j * row_groups) * rows_per_round on.  So one call runs ceil(ceil(B / rows_per_round) / row_groups) iterations per wave;
 * tests use this to reach (or to stay out of) the iterations after the first.  -22: B <= 0 or a shape the entry refuses. */
int gymrl_linear_geometry(int kind, int64_t B, int K, int N, int* row_groups, int* rows_per_round);
int gymrl_linear_bwd_weight_geometry(int64_t B, int N, int* slices, int64_t* rows_per_slice);
int gymrl_linear_bwd_weight(const float* dY, const float* X, int64_t B, int N, int K, float* dW,
                            float* db, void* workspace, void* stream);
/*
 * The second halves of the five batch reductions that close one ActorCritic minibatch backward (ppo_lunarlander.py:303) as ONE
 * launch: the slice partials of dWac = d[actor.0 | critic.0].weight (gymrl_linear_bwd_weight, N = 2C, called with dW = NULL)
 * and of dW2 / db2 = d shared.2 (N = C, dW = NULL, db != NULL), the block partials of the heads' gradients
 * (gymrl_heads_loss_fwd_bwd with its five outputs NULL) and of the first layer's (gymrl_linear_smallk_bwd, dW = db = NULL) —
 * each left in the workspace handed to that call (FOUR DIFFERENT workspaces: a deferred reduction's partials must survive
 * until this launch).  Every block runs the body of the kernel it replaces: same loads, same float64 sums in the same order,
 * outputs bit-identical to the five separate launches (tests/test_update_path_gpu.py).  C = 256, A in {2, 3, 4}, D in {2, 3, 4, 6, 8}.
 */
int gymrl_update_finalize(int64_t B, int C, int A, int D, const void* ws_dw_ac, float* dWac, const void* ws_dw_2, float* dW2,
                          float* db2, const void* ws_heads, float* dbac, float* dWa2, float* dba2, float* dWc2, float* dbc2,
                          const void* ws_smallk, float* dW1, float* db1, void* stream);

/* ========================================================= off-policy ===== */
/*
 * D2 / A3 / S2: device-resident replay ring, SoA rows [cap]:
 *   state f32[cap,D], action u32[cap,AW] (raw 4-byte words: i32 discrete action or
 *   f32 continuous components), reward f32[cap], next_state f32[cap,D], flag u8[cap]
 *   (done for DQN/SAC — dqn_cartpole.py:183, sac_pendulum.py:283; terminal for
 *   Rainbow — rainbow_dqn_cartpole.py:376-380).
 * Replaces ReplayBuffer.push/sample (dqn_cartpole.py:68-88, sac_pendulum.py:128-148)
 * and utils/buffer.py:105-135.  append writes rows (cursor + i) % cap, i < n.
 */
int gymrl_replay_append(float* state, uint32_t* action, float* reward, float* next_state,
                        uint8_t* flag, int64_t cap, int64_t cursor, int D, int AW, int n,
                        const float* src_state, const void* src_action, const float* src_reward,
                        const float* src_next_state, const uint8_t* src_flag, const int64_t* cursor_dev,
                        void* stream);
/* rows idx[b] -> contiguous batch (torch.tensor(np.array(...)) of dqn_cartpole.py:143-155) */
int gymrl_replay_gather(const float* state, const uint32_t* action, const float* reward,
                        const float* next_state, const uint8_t* flag, const int32_t* idx, int B,
                        int D, int AW, float* state_out, void* action_out, float* reward_out,
                        float* next_state_out, float* flag_out, void* stream);
/* random.sample(buffer, B) (dqn_cartpole.py:76) / np.random.choice(size, B, replace=False)
 * (utils/buffer.py:127): B DISTINCT rows — idx[b] = the b-th element of a keyed permutation of [0, size) (the
 * bijection of gymrl_permutation, keyed by (seed, counter)), so the ordered B-tuple follows the law of a uniform
 * sample without replacement (tests/test_rng_distributions.py); B <= size. */
int gymrl_uniform_indices(uint64_t seed, uint64_t counter, int64_t size, int B,
                          int32_t* idx_out, const void* dev, void* stream);

/*
 * S2: PrioritizedNStepBuffer.store_transition + _get_n_step_transition —
 * rainbow_dqn_cartpole.py:179-218 — for N envs at once.  Each env keeps its own
 * n-deep window (never cleared at episode end, :163) in caller-owned SoA arrays
 *   w_state f32[n,N,D], w_action i32[n,N], w_reward f32[n,N], w_next f32[n,N,D],
 *   w_terminal u8[n,N], w_done u8[n,N];
 * `pushes` = number of calls so far (slot = pushes % n).  When pushes + 1 >= n every env
 * emits one n-step row into the replay ring at (cursor + env) % cap:
 *   R = sum via R = r_i + gamma*(1-d_i)*R (float64, newest to oldest, :212-214),
 *   (next_state, terminal) from the newest entry unless some d_i, then from the
 *   EARLIEST done (:215-216).  Returns 1 if rows were emitted, 0 if still filling, <0 error.
 * terminal NULL: the flag is formed here as the reference's loop does (:376): done[e] && ep_len[e] != max_episode_steps
 * (ep_len i32[N] = the env's step index inside its episode, as gymrl_env_step reports it).
 */
int gymrl_nstep_push(float* w_state, int32_t* w_action, float* w_reward, float* w_next,
                     uint8_t* w_terminal, uint8_t* w_done, int n_steps, int64_t pushes,
                     int N, int D, double gamma,
                     const float* obs, const int32_t* action, const float* reward,
                     const float* next_obs, const uint8_t* terminal, const uint8_t* done,
                     float* r_state, uint32_t* r_action, float* r_reward, float* r_next,
                     uint8_t* r_flag, int64_t cap, int64_t cursor, const int64_t* dev, const int32_t* ep_len,
                     int max_episode_steps, void* stream);

/*
 * S1 / S1': SumTree — rainbow_dqn_cartpole.py:116-152 (variant A) and
 * ddqn_per_cartpole.py:67-104 (variant B).  tree f64[2*cap-1], leaf i at i+cap-1;
 * cap need not be a power of two (the array rule is followed literally).
 *   gymrl_per_update: the reference's `for idx, p in zip(...): tree.update(idx, p)`
 *     (:258-261 / :146-147): leaf := p, every ancestor += (p - old leaf), applied in
 *     batch order — duplicates resolve last-writer-wins and every node receives its
 *     additions in the reference's order, so the float64 array matches bit for bit.
 *     idx NULL -> the N-ROW VECTOR STORE: consecutive rows (idx_start + b) % cap (the store path :201-205), B <= cap.
 *       The reference stores one row per env step, so the order in which the N changes of a vector step reach an
 *       ancestor is defined HERE (and restated by the oracle's tree_store_chunk): change_b = p_b - old leaf, leaf := p_b;
 *       a complete binary tree over the batch index, seg[P + b] = change_b (+0.0 beyond B, P = the power of two >= B),
 *       seg[k] = seg[2k] + seg[2k + 1]; a node's elements (ascending b) form maximal runs of consecutive b; a run [a, e)
 *       is summed from the canonical blocks (l = a + P, r = e + P; while l < r: l odd -> sl += seg[l++]; r odd ->
 *       sr += seg[--r]; halve both; run = sl + sr); S = +0.0 + run_1 + run_2 ...; node := node + S — ONE addition per
 *       node, no chain longer than log2(P) + 4 float64 adds.  B > 8192: sub-stores of 8192 rows in order.  At B = 1 this
 *       is the reference's `tree[parent] += change` (:122-128) bit for bit; the strictly ordered per-node sums above
 *       remain for explicit index batches (update_priorities, whose order the reference does define).
 *     idx_is_tree != 0 -> idx are tree indices (variant B, :75-80).
 *     prio f64[B], or prio NULL and prio_scalar for all (store: 1.0 or priority_max).
 *     workspace >= gymrl_per_workspace_bytes(B).
 *   gymrl_per_max_leaf: priority_max (:151-152) = max over all leaves -> out f64[1].
 *   gymrl_per_priorities: p = min(|td| + eps, clip)^alpha in float64 (:259 eps 0.01,
 *     clip inf; ddqn_per_cartpole.py:142-145 eps 1e-4, clip 1.0).
 *   gymrl_per_sample: stratified draw (:228-239): segment = total/B,
 *     v = seg*b + seg*u[b] (u f64[B] in [0,1), or NULL -> Philox(seed, counter, b)),
 *     get_index descent (:130-144); idx_out data (A) or tree (B) indices, prio_out f64,
 *     w_out f32[B] = (size * p/total)^(-beta) / max — float32 normalisation for
 *     variant A (:226,:239,:241), float64 for variant B (ddqn_per_cartpole.py:135-138).
 */
size_t gymrl_per_workspace_bytes(int B);
int gymrl_per_update(double* tree, int64_t cap, const int32_t* idx, int64_t idx_start,
                     int idx_is_tree, const double* prio, const double* prio_scalar_dev,
                     double prio_scalar, int B, const int64_t* idx_start_dev, void* workspace, void* stream);
int gymrl_per_max_leaf(const double* tree, int64_t cap, double* out, void* workspace,
                       void* stream);
int gymrl_per_priorities(const float* td, int B, double alpha, double eps, double clip,
                         double* prio_out, void* stream);
/* update_priorities of a sampled batch (rainbow_dqn_cartpole.py:258-261) in two launches: gymrl_per_priorities' transform of
 * td inside gymrl_per_update's leaf pass (data indices idx i32[B], B <= 512, cap < 2^30), and — max_out != NULL — the maximum
 * over the leaves AFTER the update (gymrl_per_max_leaf: what the next store gives its new rows) computed by extra workgroups
 * of the ancestor launch; `ticket` u32[1] must be zero before the first call and is left zero.  The tree and max_out hold the
 * bits of gymrl_per_priorities -> gymrl_per_update -> gymrl_per_max_leaf. */
int gymrl_per_update_td(double* tree, int64_t cap, const int32_t* idx, const float* td, int B, double alpha, double eps,
                        double clip, double* max_out, unsigned int* ticket, void* workspace, void* stream);
int gymrl_per_sample(const double* tree, int64_t cap, const double* u, uint64_t seed,
                     uint64_t counter, int B, int64_t size, double beta, int variant_b,
                     int32_t* idx_out, double* prio_out, float* w_out, const void* dev, void* workspace,
                     void* stream);

/* R1: NoisyLinear.scale_noise + reset_noise — rainbow_dqn_cartpole.py:77-87.
 * f(x) = sign(x)*sqrt(|x|); w_eps[out,in] = outer(f(eps_out), f(eps_in)); b_eps = f(eps_out).
 * eps_in/eps_out raw N(0,1) f32 (parity mode) or NULL -> Box-Muller on Philox(seed, counter). */
int gymrl_noisy_noise(const float* eps_in_raw, const float* eps_out_raw, uint64_t seed,
                      uint64_t counter, int in_features, int out_features, float* w_eps_out,
                      float* b_eps_out, const uint64_t* counter_dev, void* stream);

/* D3: epsilon-greedy action selection for N envs — dqn_cartpole.py:117-133.
 * u f32[N,2] uniforms (or NULL -> Philox): u[.,0] < eps -> action = floor(u[.,1]*A) else argmax q. */
int gymrl_epsilon_greedy(const float* q, const float* u, uint64_t seed, uint64_t counter,
                         int64_t env_id0, int n, int A, float epsilon, int32_t* act_out,
                         void* stream);

/*
 * D4 / R4: TD target + loss forward/backward on the Q heads —
 * dqn_cartpole.py:157-161 (q_next_online NULL: max_a' Q_tgt), rainbow_dqn_cartpole.py:319-338
 * and ddqn_per_cartpole.py:224-233 (double DQN: a* = argmax q_next_online, weights w).
 *   y = r + gamma_n * q_tgt(s', a*) * (1 - flag);  td = q(s,a) - y
 *   loss = mean(td^2 * w) (w NULL -> 1, i.e. F.mse_loss);  dq[b,a] = 2*td*w/B
 * td_out f32[B] (feeds update_priorities), dq_out f32[B,A], loss_sum f64[1] += sum td^2*w.
 */
int gymrl_dqn_td_loss(const float* q, const float* q_next_online, const float* q_next_target,
                      const int32_t* act, const float* rew, const float* flag, const float* w,
                      int B, int A, double gamma_n, float* td_out, float* dq_out,
                      double* loss_sum, void* workspace, void* stream);

/*
 * C51: the categorical value head (Bellemare et al. 2017) — csrc/c51.hip, arithmetic in csrc/c51_device.hpp.
 * logits f32[B][A][M]: a Linear(H, A * M) head, atom j of action a at a * M + j.  Support z_j = vmin + j * dz,
 * dz = (vmax - vmin) / (M - 1), float32.  Shapes: 1 <= A <= 8, 2 <= M <= 64 (one atom per lane of a wave64), vmax > vmin with
 * a finite dz > 0, B >= 0; anything else is -22 before any HIP call, B == 0 returns 0 without a launch.
 *   softmax   e_j = det_expf(x_j - max_j x_j),  s = sum_j e_j,  p_j = e_j / s
 * Sums over a row's atoms (s, q, the cross-entropy) run as the halving tree over 64 slots (slots >= M hold +0):
 * v[0:off] + v[off:2 off] for off = 32 ... 1.  No order depends on B or the grid.
 *
 * gymrl_c51_q: q_out f32[B][A] = sum_j p_j z_j per (row, action); argmax_out i32[B] (may be NULL) = the FIRST maximum over the
 * actions (torch.argmax's tie rule).  Acting: q_out feeds gymrl_epsilon_greedy.
 *
 * gymrl_c51_loss, per row b (next_online, next_target f32[B][A][M]; act i32[B]; rew, flag f32[B]; w f32[B] or NULL = 1):
 *   1. a* = first maximum over a of the expected value of next_online[b] (double-Q; NULL: of next_target[b])
 *   2. p* = softmax(next_target[b, a*, :])
 *   3. Tz_j = clamp(rew + gamma_n (1 - flag) z_j, vmin, vmax),  b_j = (Tz_j - vmin) / dz,
 *      m_i = sum_j p*_j max(0, 1 - |b_j - i|), j ascending from +0: the gather form of the floor / ceil scatter — no atomics,
 *      and a b_j that lands on an atom gives that atom weight 1 (the textbook scatter's l == u case)
 *   4. logp_i = (x_i - max) - det_logf(s) on x = logits[b, act_b, :];  row_loss_out[b] = -sum_i m_i logp_i (unweighted: the
 *      priority error of a PER trainer)
 *   5. dlogits_out[b, act_b, i] = (w_b * (1 / B)) * (p_i - m_i); every other action's atoms are written 0, so the caller
 *      needs no memset.  An act_b outside [0, A) touches nothing out of range: row_loss_out[b] = NaN, the row's gradient 0
 *   6. loss_sum f64[1] (may be NULL) += sum_b (double)(row_loss_b * w_b) in gymrl_dqn_td_loss's reduction (one workgroup of
 *      four rows adds to loss_sum itself, more go through workspace >= gymrl_reduce_workspace_bytes(), required with loss_sum,
 *      and a finalize launch)
 */
int gymrl_c51_q(const float* logits, int B, int A, int M, float vmin, float vmax, float* q_out,
                int32_t* argmax_out, void* stream);
int gymrl_c51_loss(const float* logits, const float* next_online, const float* next_target,
                   const int32_t* act, const float* rew, const float* flag, const float* w, int B, int A,
                   int M, float vmin, float vmax, double gamma_n, float* row_loss_out,
                   float* dlogits_out, double* loss_sum, void* workspace, void* stream);

/*
 * QR-DQN: the quantile-regression value head (Dabney et al. 2018) — csrc/qrdqn.hip, arithmetic in csrc/qrdqn_device.hpp.
 * quant f32[B][A][N]: a Linear(H, A * N) head, quantile i of action a at a * N + i, for the fixed midpoints
 * tau_i = (2 i + 1) / (2 N).  There is no support, no projection and no clamp.  Shapes: 1 <= A <= 8, 1 <= N <= 64 (one quantile
 * per lane of a wave64), B >= 0, kappa finite and > 0; anything else, a NULL required pointer, or loss_sum without workspace is
 * -22 before any HIP call, B == 0 returns 0 without a launch.  float32 throughout, +, -, *, / and comparisons only.
 * Sums over a row's quantiles (the mean, the row's loss) run as the halving tree over 64 slots (slots >= N hold +0):
 * v[0:off] + v[off:2 off] for off = 32 ... 1; the sum over the target samples j is serial, j ascending from +0.  No order
 * depends on B or the grid.
 *
 * gymrl_qr_q: q_out f32[B][A] = (sum_i quant[b][a][i]) / N; argmax_out i32[B] (may be NULL: untouched) = the FIRST maximum over
 * the actions (torch.argmax's tie rule).  Acting: q_out feeds gymrl_epsilon_greedy.
 *
 * gymrl_qr_loss, per row b (next_online, next_target f32[B][A][N]; act i32[B]; rew, flag f32[B]; w f32[B] or NULL = 1):
 *   1. a* = first maximum over a of the mean quantile of next_online[b] (double-Q; NULL: of next_target[b])
 *   2. g = (float)gamma_n * (1 - flag_b),  T_j = rew_b + g * next_target[b][a*][j]
 *   3. with theta_i = quant[b][act_b][i], u_ij = T_j - theta_i and wt_ij = |tau_i - 1{u_ij < 0}| (tau_i, or 1 - tau_i below 0):
 *        H(u) = 0.5 u^2 if |u| <= kappa, else kappa (|u| - 0.5 kappa)
 *        l_i = sum_j wt_ij H(u_ij),   g_i = sum_j wt_ij clamp(u_ij, -kappa, kappa)
 *      row_loss_out[b] = sum_i (l_i / kappa) / N (unweighted: the priority error of a PER trainer)
 *   4. dquant_out[b][act_b][i] = (w_b * (1 / B)) * -((g_i / kappa) / N); every other action's quantiles are written 0, so the
 *      caller needs no memset.  An act_b outside [0, A) touches nothing out of range: row_loss_out[b] = NaN, the row's gradient 0
 *   5. loss_sum f64[1] (may be NULL) += sum_b (double)(row_loss_b * w_b) in gymrl_c51_loss's reduction (one workgroup of four
 *      rows adds to loss_sum itself, more go through workspace >= gymrl_reduce_workspace_bytes(), required with loss_sum, and a
 *      finalize launch)
 * At u == 0 the indicator is 0 and both terms are 0; at |u| == kappa the two branches of H agree.
 */
int gymrl_qr_q(const float* quant, int B, int A, int N, float* q_out, int32_t* argmax_out, void* stream);
int gymrl_qr_loss(const float* quant, const float* next_online, const float* next_target,
                  const int32_t* act, const float* rew, const float* flag, const float* w, int B, int A,
                  int N, float kappa, double gamma_n, float* row_loss_out, float* dquant_out,
                  double* loss_sum, void* workspace, void* stream);

/*
 * A1: Actor.sample — sac_pendulum.py:76-87 — forward and backward.
 *   x = mean + exp(log_std)*eps; a = tanh(x)*bound;
 *   logp = sum_j [ Normal(mean,std).log_prob(x) - log(bound*(1 - tanh(x)^2) + 1e-6) ]
 * fwd: mean, log_std, eps f32[B,A] -> action f32[B,A], logp f32[B].
 * bwd: d_action f32[B,A] (may be NULL), d_logp f32[B] -> d_mean, d_log_std f32[B,A].
 */
int gymrl_sac_sample_fwd(const float* mean, const float* log_std, const float* eps, int B, int A,
                         float bound, float* action_out, float* logp_out, void* stream);
int gymrl_sac_sample_bwd(const float* mean, const float* log_std, const float* eps,
                         const float* d_action, const float* d_logp, int B, int A, float bound,
                         float* d_mean_out, float* d_log_std_out, void* stream);

/*
 * A4: SACTrainer.update pieces — sac_pendulum.py:233-263.
 *   target:  y = r + gamma*(1-done)*(min(q1n,q2n) - alpha*logp_n)            (:233-237)
 *   critic:  loss = mse(q1,y) + mse(q2,y); dq1 = 2(q1-y)/B, dq2 = 2(q2-y)/B   (:239-242)
 *   actor:   loss = mean(alpha*logp - min(q1,q2)); dlogp = alpha/B,
 *            dq_k = -(1/B) on the smaller critic (tie 1/2,1/2)                (:248-251)
 *   alpha:   loss = -mean(log_alpha*(logp + target_entropy)); one Adam step on the
 *            float64 scalar log_alpha (state m, v f64[1])                     (:257-263)
 * log_alpha f64[1] lives on the device; alpha = (float)exp(log_alpha) inside the kernels.
 * sums f64[4] += (critic loss sum, actor loss sum, sum(logp + target_entropy), 0).
 * alpha steps: bias_dev f64[2] or NULL = device-resident {1 - beta1^step, 1 - beta2^step}; with it `step`
 * is ignored and a captured hipGraph of the update replays unchanged (see gymrl_adam_step).
 */
int gymrl_sac_target(const float* rew, const float* done, const float* q1n, const float* q2n,
                     const float* logp_n, const double* log_alpha, int B, double gamma,
                     float* y_out, void* stream);
int gymrl_sac_critic_loss(const float* q1, const float* q2, const float* y, int B,
                          float* dq1_out, float* dq2_out, double* sums, void* workspace,
                          void* stream);
int gymrl_sac_actor_loss(const float* logp, const float* q1, const float* q2,
                         const double* log_alpha, int B, double target_entropy,
                         float* dlogp_out, float* dq1_out, float* dq2_out, double* sums,
                         void* workspace, void* stream);
int gymrl_sac_alpha_step(double* log_alpha, double* m, double* v, const double* sums, int B,
                         double lr, double beta1, double beta2, double eps, int64_t step,
                         const double* bias_dev, double* alpha_loss_out, void* stream);

/*
 * TD3 / DDPG — ddpg_pendulum.py:135-195, td3_pendulum.py:156-228.  Their Bellman target is
 * gymrl_sac_target with logp_n == 0 (r + gamma (1 - done) min(Q1', Q2'); DDPG passes Q' twice), TD3's critic
 * loss is gymrl_sac_critic_loss, the Polyak updates gymrl_soft_update; what is new:
 *   noisy_action : mode 0 = exploration noise of select_action (numpy float64: clip(mu + eps*std, +-bound),
 *                  :143-147 / :164-168), mode 1 = TD3 target-policy smoothing (torch float32:
 *                  clamp(mu + clamp(eps*std, +-noise_clip), +-bound), :191-196).  eps f64[n] explicit N(0,1)
 *                  draws or NULL -> Box-Muller on Philox(seed, counter, element).
 *   mse_loss     : one critic's F.mse_loss(q, y): dq = 2 (q - y)/B, sum_out += sum (q - y)^2   (ddpg :178-179)
 *   neg_mean_loss: actor loss -mean(Q(s, mu(s))): dq = -1/B, sum_out += sum q                  (ddpg :185, td3 :213)
 * sum_out f64[1] is accumulated into (zero it first); workspace as for the SAC losses.
 */
int gymrl_noisy_action(const float* mu, const double* eps, uint64_t seed, uint64_t counter, int64_t n,
                       int mode, double std, double noise_clip, double bound, float* out, void* stream);
int gymrl_mse_loss(const float* q, const float* y, int B, float* dq_out, double* sum_out, void* workspace,
                   void* stream);
int gymrl_neg_mean_loss(const float* q, int B, float* dq_out, double* sum_out, void* workspace, void* stream);

/*
 * Discrete SAC — sac_cartpole.py:148-227: expectation over the A <= 8 actions, float32 throughout
 * (log_alpha is a float32 scalar there).  probs = the actor's softmax output [B, A]; q* [B, A].
 *   dsac_target      : y = r + gamma (1 - done) (sum_a p'(a) min(Q1', Q2')(a) + alpha H(p')), log p = log(p + 1e-8)   :171-181
 *   dsac_critic_loss : F.mse_loss(q.gather(1, a), y) for both critics; dq [B, A] non-zero at the taken action;
 *                      sums f64[2] += (sum e1^2, sum e2^2)                                                         :183-186
 *   dsac_actor_loss  : L = mean(-alpha H(p) - sum_a p(a) min(Q1, Q2)(a)); dprobs = dL/dp (backprop through the
 *                      softmax by the caller); sums f64[2] += (sum (-alpha H - min_q), sum H)                      :196-203
 *   dsac_alpha_step  : L_alpha = exp(log_alpha) mean(H - H_target) from sums[1]; one float32 Adam step on log_alpha :209-215
 */
int gymrl_dsac_target(const float* probs_n, const float* q1n, const float* q2n, const float* rew,
                      const float* done, const float* log_alpha, int B, int A, double gamma, float* y_out,
                      void* stream);
int gymrl_dsac_critic_loss(const float* q1, const float* q2, const int32_t* act, const float* y, int B, int A,
                           float* dq1_out, float* dq2_out, double* sums, void* workspace, void* stream);
int gymrl_dsac_actor_loss(const float* probs, const float* q1, const float* q2, const float* log_alpha, int B,
                          int A, float* dprobs_out, double* sums, void* workspace, void* stream);
int gymrl_dsac_alpha_step(float* log_alpha, float* m, float* v, const double* sums, int B,
                          double target_entropy, double lr, double beta1, double beta2, double eps,
                          int64_t step, const double* bias_dev, double* alpha_loss_out, void* stream);

/*
 * N1-N3: utils/normalization.py — RunningMeanStd.update :12-22 (Welford, population
 * std, n == 1 sets std = x), Normalization.__call__ :29-35, RewardScaling :38-52.
 * stats f64[2 + 3*D] = (n, unused, mean[D] (float32 values), S[D], std[D]).
 * x f32[N,D] is consumed in env order 0..N-1 exactly like N successive reference calls
 * (the reference has ONE stream; this is its sequential-equivalent batch semantics).
 *   running_norm:   update (if update != 0) then y = (x - mean)/(std + 1e-8)
 *   reward_scaling: R[env] = gamma*R[env] + r[env]; update(R); y = r/(std + 1e-8);
 *                   R[env] := 0 where done (RewardScaling.reset at episode start)
 */
int gymrl_running_norm(const float* x, int N, int D, double* stats, int update, float* y_out,
                       void* stream);
int gymrl_reward_scaling(const float* r, const uint8_t* done, int N, double gamma, double* R,
                         double* stats, float* y_out, void* stream);
/* The same over the rows with live u8[N] != 0 only (the PPG / PPO-RNN trainers' finished envs of a round, which the
 * reference never steps): dead rows neither update the statistics nor R, and their outputs are not written. */
int gymrl_running_norm_masked(const float* x, const uint8_t* live, int N, int D, double* stats, int update,
                              float* y_out, void* stream);
int gymrl_reward_scaling_masked(const float* r, const uint8_t* done, const uint8_t* live, int N, double gamma,
                                double* R, double* stats, float* y_out, void* stream);

/* ============================================ fused off-policy vector step ===== */
/*
 * One SAC vector step of sac_pendulum.py:269-310 as five launches (gymrl_sac_act_step + gymrl_sac_update's four) instead
 * of ~60 (csrc/offpolicy_step.hip; round 3's step:
 * 3 gymrl_lin_fwd + sample + env step + append + index draw + gather + ~45 layer / loss / optimiser launches of 4-14 us).
 * A forward or input-gradient pass never mixes batch rows, so ONE workgroup carries a 16-row slab of the batch through a
 * whole chain of layers in LDS (tile bodies of csrc/lin_device.hpp: the very MFMA sequence of gymrl_lin_*), and only the
 * weight gradients, which reduce over the batch, need a kernel boundary:
 *   gymrl_sac_act_step   acting (:278-283): Actor forward on the N observations, reparameterised draw, Pendulum step with
 *                        auto-reset, replay row (obs, action, reward, TERMINAL next obs, done) at (cursor + env) % cap
 *   gymrl_sac_update     update() (:213-267), four launches:
 *     P1 rows   index draw (gymrl_uniform_indices' permutation) + ring gather; a', logp' = Actor.sample(s'); target
 *               Q(s', a'); y; Q(s, a); critic loss gradient; input-gradient chain of both Q networks
 *     P2 tiles  every critic weight / bias gradient tile (gymrl_lin_bwd_weight's order) + Adam on that tile + the soft target
 *               update of the element just written (gymrl_adam_step's expressions); critic loss sum
 *     P3 rows   a, logp = Actor.sample(s); Q(s, a) of the UPDATED critic; actor loss gradient; the chain back through both
 *               Q networks to the action, through the sample, through the actor
 *     P4 tiles  actor weight gradients + Adam; actor loss / temperature sums; the float64 temperature step
 * Results are those of the layer-by-layer path bit for bit (same products, same orders; tests/test_fused_step_gpu.py), which
 * tests/test_trainers_gpu.py pins against the reference.  Limits: H % 4 == 0, H <= 256, D <= 8, A <= 4, B <= 8192
 * (-22 otherwise: use the layer-by-layer path).  Above 256 rows the row kernels run on 1-D grids with a
 * slab's workgroups adjacent in dispatch order, above 512 the weight gradients are two launches (slice partials in
 * gymrl_lin_bwd_weight's cut, then their ordered sums + the optimiser step): still the layer path's bits.  Pointers are device pointers; W = [out][in] row-major (nn.Linear).
 */
typedef struct { float* w[4]; float* b[4]; } gymrl_sac_actor_params;     /* fc1, fc2, mean, log_std (sac_pendulum.py:58-61) */
typedef struct { float* w[6]; float* b[6]; } gymrl_sac_critic_params;    /* fc1..fc6: fc1-3 = Q1, fc4-6 = Q2 (:108-113) */
typedef struct {
  int N, D, A, H;                          /* envs, obs dim, action dim, hidden width */
  int env_kind;                            /* GYMRL_ENV_PENDULUM */
  void* env_state; uint64_t env_seed; int64_t env_id0;
  const float* obs;                        /* f32[N, D] the observations to act on */
  float* obs_out;                          /* f32[N, D] next observations (post-reset where an episode ended) */
  const float* eps;                        /* f32[N, A] N(0,1) draws, or NULL: Philox (noise_seed, noise_counter, stream 2, env * A + j) */
  uint64_t noise_seed, noise_counter; const uint64_t* noise_counter_dev;
  float bound, log_std_min, log_std_max;
  gymrl_sac_actor_params actor;
  /* replay ring (gymrl_replay_append's layout); cursor_dev int64[1] or NULL */
  float* r_state; uint32_t* r_action; float* r_reward; float* r_next; uint8_t* r_flag; int64_t cap, cursor;
  const int64_t* cursor_dev;
  /* per-step outputs of the episode bookkeeping (any may be NULL) */
  float* action_out; float* rew_out; uint8_t* done_out; float* ep_ret_out; double* ep_stats;
  const float* images;                     /* gymrl_sac_update_args.images of the same trainer, or NULL (reads actor.fc2 in place) */
} gymrl_sac_act_args;
typedef struct {
  int B, D, A, H;
  float gamma, bound, log_std_min, log_std_max, target_entropy;
  double tau;                              /* soft target update rate (a python float: rounded like gymrl_adam_step does) */
  const float* r_state; const uint32_t* r_action; const float* r_reward; const float* r_next; const uint8_t* r_flag;
  const int32_t* idx;                      /* i32[B] explicit rows, or NULL: the keyed permutation of gymrl_uniform_indices */
  uint64_t idx_seed, idx_counter; int64_t idx_size; const void* idx_dev;     /* idx_dev: {uint64 counter; int64 size} */
  const float* eps_next; const float* eps_cur;     /* f32[B, A] each, or NULL: Philox streams 3 / 4 of (noise_seed, noise_counter) */
  uint64_t noise_seed, noise_counter; const uint64_t* noise_counter_dev;
  gymrl_sac_actor_params actor; gymrl_sac_critic_params critic, target;
  /* flat parameter buffers and their Adam moments (same layout): m of a parameter p lives at critic_m + (p - critic_p) */
  float* actor_p; float* actor_m; float* actor_v; float* critic_p; float* critic_m; float* critic_v;
  float adam_critic[4], adam_actor[4];     /* gymrl_adam_bias' block {lr/(1-b1^t), 1/(1-b1^t), sqrt(1-b2^t), 0} */
  const float* adam_critic_dev; const float* adam_actor_dev;      /* the same from device memory (hipGraph replay) or NULL */
  double beta1, beta2, eps_adam;
  double* log_alpha; double* alpha_m; double* alpha_v; double lr_alpha;
  double alpha_bias[2]; const double* alpha_bias_dev;             /* {1 - 0.9^t, 1 - 0.999^t} (gymrl_sac_alpha_step) */
  double* sums;                            /* f64[3] out: critic loss sum, actor loss sum, sum of (logp + target_entropy) */
  double* alpha_loss;                      /* f64[1] out or NULL */
  void* workspace;                         /* >= gymrl_sac_update_workspace_bytes(B, D, A, H); ZEROED once before the first call (the
                                            * hand-off flags between the row phases' workgroups and the large-batch grids' tickets
                                            * live in it and are left zero) */
  /* Weight images of the H x H layers (H % 16 == 0), f32[8][H*H], or NULL (every layer read in place).  The MFMA operands of
   * actor.fc2, critic.fc2 / fc5, target.fc2 / fc5 (forward) and actor.fc2, critic.fc2 / fc5 (input gradient) as contiguous
   * 1 KiB blocks per wave-wide load (csrc/lin_device.hpp): a slab kernel streams a whole weight matrix through one compute
   * unit, 3x faster from the image.  gymrl_sac_update keeps the images equal to the parameters it updates;
   * gymrl_sac_pack_images rebuilds them after anything else wrote the parameters (load_state_dict, a checkpoint, ...). */
  float* images;
} gymrl_sac_update_args;
size_t gymrl_sac_update_workspace_bytes(int B, int D, int A, int H);
int gymrl_sac_pack_images(const gymrl_sac_update_args* args, void* stream);
size_t gymrl_sac_args_bytes(int which);      /* sizeof(gymrl_sac_act_args) (0) / sizeof(gymrl_sac_update_args) (1): a binding checks its mirror */
int gymrl_sac_act_step(const gymrl_sac_act_args* args, void* stream);
int gymrl_sac_update(const gymrl_sac_update_args* args, void* stream);

/*
 * The same treatment for Rainbow's vector step (rainbow_dqn_cartpole.py:363-405; csrc/offpolicy_step.hip).  The NoisyLinear
 * bookkeeping (which draw a forward uses, where its epsilons live) stays with gymrl_noisy_combine / gymrl_noisy_split, the sum
 * tree with gymrl_per_*; the Linear / loss / env / n-step launches between them — ~20 of a step's ~45 — become three:
 *   gymrl_rainbow_act_step     greedy acting on the noisy Q (:293-309, :371): fc1, fc2, the stacked noisy heads with the dueling
 *                              combination, argmax (first maximum), CartPole step with auto-reset, `terminal = done and step !=
 *                              max_steps - 1` (:376), the n-step window push and the emitted ring row (gymrl_nstep_push)
 *   gymrl_rainbow_update       rows: ring gather at the sampled indices; policy(s') | target(s') | policy(s) through fc1, fc2 and
 *                              their stacked heads (W_heads [3][A+1][H], b_heads [3][A+1] from gymrl_noisy_combine: first draw,
 *                              target means, second draw); double-DQN target, IS-weighted TD loss gradient (gymrl_dqn_td_loss's
 *                              expressions), dueling backward, input-gradient chain;  tiles: dW / db of the stacked head (for
 *                              gymrl_noisy_split), fc2 and fc1 written where the caller says (the flat gradient buffer's views:
 *                              clip_grad_norm_ needs every gradient before Adam), loss sum
 * Bit-identical to the layer-by-layer path (same tile bodies, same scalar expressions).  Limits: H % 4 == 0, H <= 256, D <= 8,
 * A <= 3, B <= 8192 (above 256 / 512 rows: as gymrl_sac_update); CartPole-v1 for the act step.
 */
typedef struct {
  int N, D, A, H;
  int env_kind;                              /* GYMRL_ENV_CARTPOLE */
  void* env_state; uint64_t env_seed; int64_t env_id0;
  const float* obs; float* obs_out;          /* f32[N, D] in / next observations out */
  const float* fc1_w; const float* fc1_b; const float* fc2_w; const float* fc2_b;
  const float* head_w; const float* head_b;  /* stacked effective head [A+1][H], [A+1] (advantage rows, then value) */
  int max_episode_steps;
  /* n-step windows + ring (gymrl_nstep_push's arguments) */
  float* w_state; int32_t* w_action; float* w_reward; float* w_next; uint8_t* w_terminal; uint8_t* w_done;
  int n_steps; int64_t pushes; double gamma;
  float* r_state; uint32_t* r_action; float* r_reward; float* r_next; uint8_t* r_flag; int64_t cap, cursor;
  const int64_t* push_dev;                   /* {pushes, cursor} from the device (hipGraph replay) or NULL */
  int32_t* action_out; float* rew_out; uint8_t* done_out; float* ep_ret_out; double* ep_stats;   /* any may be NULL */
  const float* fc2_img;                      /* forward weight image of fc2_w (gymrl_weight_image; H % 16 == 0) or NULL: read in place */
} gymrl_rainbow_act_args;
typedef struct {
  int B, D, A, H;
  float gamma_n;                             /* gamma ** n_steps */
  const float* r_state; const uint32_t* r_action; const float* r_reward; const float* r_next; const uint8_t* r_flag;
  const int32_t* idx; const float* is_weight;        /* i32[B] sampled rows, f32[B] importance weights (NULL: 1) */
  const float* p_fc1_w; const float* p_fc1_b; const float* p_fc2_w; const float* p_fc2_b;    /* policy network */
  const float* t_fc1_w; const float* t_fc1_b; const float* t_fc2_w; const float* t_fc2_b;    /* target network */
  const float* head_w; const float* head_b;  /* [3][A+1][H], [3][A+1]: policy on s' (first draw), target on s', policy on s (second draw) */
  float* td_out;                             /* f32[B] TD errors (update_priorities) */
  double* loss_sum;                          /* f64[1] out: sum of w * td^2 */
  float* d_fc1_w; float* d_fc1_b; float* d_fc2_w; float* d_fc2_b; float* d_head_w; float* d_head_b;   /* gradients (overwritten) */
  void* workspace;                           /* >= gymrl_rainbow_update_workspace_bytes(B, D, A, H); ZEROED once before the first call
                                              * (the hand-off flags between the row phase's three workgroups per slab live in it) */
  /* gymrl_noisy_split inside the weight-gradient launch (split_heads != 0; d_head_w / d_head_b are then not written): the stacked
   * head's gradient goes straight to the two NoisyLinear layers' parameters, [0] = advantage (rows 0 .. A-1), [1] = value (row A):
   * d mu = dW, d sigma = dW * eps with the SECOND draw's epsilons (rainbow_dqn_cartpole.py:92-93 under autograd) */
  int split_heads;
  float* dw_mu[2]; float* dw_sigma[2]; float* db_mu[2]; float* db_sigma[2]; const float* w_eps[2]; const float* b_eps[2];
  /* Weight images of the H x H layer (H % 16 == 0; gymrl_weight_image) or NULL (read in place): p_fc2_w forward and
   * input-gradient, t_fc2_w forward.  The CALLER keeps them equal to the parameters: the Rainbow trainer rebuilds all three in
   * the step's gymrl_noisy_combine_images launch, between the optimiser step and the next acting forward. */
  const float* p_fc2_img_f; const float* p_fc2_img_b; const float* t_fc2_img_f;
} gymrl_rainbow_update_args;
size_t gymrl_rainbow_update_workspace_bytes(int B, int D, int A, int H);
size_t gymrl_rainbow_args_bytes(int which);  /* sizeof(gymrl_rainbow_act_args) (0) / sizeof(gymrl_rainbow_update_args) (1) */
int gymrl_rainbow_act_step(const gymrl_rainbow_act_args* args, void* stream);
int gymrl_rainbow_update(const gymrl_rainbow_update_args* args, int phase, void* stream);   /* phase 0: both launches; 1: rows (td_out is complete after it: update_priorities may start); 2: tiles */

/*
 * TD3's and DDPG's Pendulum vector step on the same row-slab kernels (csrc/offpolicy_step.hip): td3_pendulum.py's train loop
 * :230-262 / update :171-228 and ddpg_pendulum.py's :196-228 / :150-194.  SAC's step with a deterministic tanh actor (:48-61),
 * clipped Gaussian noise in place of the reparameterised sample, no temperature, and a delayed actor phase:
 *   gymrl_td3_act_step   ONE launch: actor forward on the N observations (fc1, fc2 ReLU, fc3 tanh, times bound; :158-163),
 *                        exploration noise by gymrl_noisy_action mode 0's float64 expression (:164-168; explicit f64 eps or Philox
 *                        (noise_seed, noise_counter, stream 2, element)), Pendulum step with auto-reset, replay row (obs, action,
 *                        reward, TERMINAL next obs, done) at (cursor + env) % cap, the episode bookkeeping outputs
 *   gymrl_td3_update     update(), at most four launches, n_critics = 2 (TD3) or 1 (DDPG):
 *     R1 rows   index draw (gymrl_uniform_indices' permutation, or idx) + ring gather; actor_target(s') (:191); the smoothing noise
 *               by gymrl_noisy_action mode 1's float32 expression (:192-196; none when policy_noise == 0 or n_critics == 1);
 *               the target critic(s) (:197); y by gymrl_sac_target's expression with a zero log-prob (:198-199); critic(s) on
 *               (s, a) (:201); gymrl_sac_critic_loss's / gymrl_mse_loss's gradient (:203-204); the critics' input-gradient chain
 *     T2 tiles  critic weight / bias gradient tiles (gymrl_lin_bwd_weight's order) + Adam (:206-208); the critic target's Polyak
 *               update only on a DELAYED step (:223 sits inside the policy_freq branch; DDPG :190: every step); critic loss sum
 *     R3 rows   actor(s); critic.q1(s, actor(s)) of the UPDATED critic (:213; DDPG's single critic :185); gymrl_neg_mean_loss's
 *               gradient back through the critic to the action, through bound and tanh, through the actor
 *     T4 tiles  actor weight gradients + Adam (:215-217), the actor target's Polyak update (:222-224), actor loss sum
 *   Whether a step is delayed is ONE word: `delayed`, or delayed_dev[0] when that pointer is set, so that one captured hipGraph
 *   serves every step.  On a step that is not, every workgroup of R3 and T4 returns at once and T2 leaves the target alone; the
 *   decision is uniform over each grid and no workgroup waits for another anywhere in these kernels (one workgroup carries a
 *   slab through all of a row phase).
 * Results are the layer-by-layer path's bits (tests/test_td3_fused_step_gpu.py).  Limits: H % 4 == 0, H <= 256, D <= 8, A <= 4,
 * B <= 256 (-22 otherwise: the trainers stay on the layer path); Pendulum-v1 for the act step.
 */
typedef struct { float* w[3]; float* b[3]; } gymrl_td3_actor_params;     /* fc1, fc2, fc3 (td3_pendulum.py:52-54) */
typedef struct {
  int N, D, A, H;
  int env_kind;                            /* GYMRL_ENV_PENDULUM */
  void* env_state; uint64_t env_seed; int64_t env_id0;
  const float* obs; float* obs_out;        /* f32[N, D] in / next observations out (post-reset where an episode ended) */
  const double* eps;                       /* f64[N, A] N(0,1) draws, or NULL: Philox (noise_seed, noise_counter, stream 2, env * A + j) */
  uint64_t noise_seed, noise_counter; const uint64_t* noise_counter_dev;
  float bound; double noise_std;           /* action bound; exploration std (already times the bound, as select_action passes it) */
  gymrl_td3_actor_params actor;
  float* r_state; uint32_t* r_action; float* r_reward; float* r_next; uint8_t* r_flag; int64_t cap, cursor;
  const int64_t* cursor_dev;
  float* action_out; float* rew_out; uint8_t* done_out; float* ep_ret_out; double* ep_stats;     /* any may be NULL */
  const float* images;                     /* gymrl_td3_update_args.images of the same trainer, or NULL (reads actor.fc2 in place) */
} gymrl_td3_act_args;
typedef struct {
  int B, D, A, H;
  int n_critics;                           /* 2: TD3 (critic.fc1-3 = Q1, fc4-6 = Q2), 1: DDPG (fc1-3 only) */
  float gamma, bound, noise_clip;
  double policy_noise, tau;
  const float* r_state; const uint32_t* r_action; const float* r_reward; const float* r_next; const uint8_t* r_flag;
  const int32_t* idx;                      /* i32[B] explicit rows, or NULL: the keyed permutation of gymrl_uniform_indices */
  uint64_t idx_seed, idx_counter; int64_t idx_size; const void* idx_dev;     /* idx_dev: {uint64 counter; int64 size} */
  const double* eps;                       /* f64[B, A] smoothing draws, or NULL: Philox (noise_seed, noise_counter, stream 2, row * A + j) */
  uint64_t noise_seed, noise_counter; const uint64_t* noise_counter_dev;
  int delayed; const int32_t* delayed_dev; /* != 0: the actor phases run and the critic target moves (total_updates % policy_freq == 0) */
  gymrl_td3_actor_params actor, actor_target; gymrl_sac_critic_params critic, critic_target;
  float* actor_p; float* actor_m; float* actor_v; float* critic_p; float* critic_m; float* critic_v;
  float adam_critic[4], adam_actor[4];
  const float* adam_critic_dev; const float* adam_actor_dev;
  double beta1, beta2, eps_adam;
  double* sums;                            /* f64[2] out: critic loss sum; sum of Q(s, actor(s)) (written on delayed steps only) */
  void* workspace;                         /* >= gymrl_td3_update_workspace_bytes(B, D, A, H) */
  /* Weight images of the H x H layers (H % 16 == 0), f32[9][H*H], or NULL: forward actor.fc2, critic.fc2 / fc5,
   * critic_target.fc2 / fc5, actor_target.fc2; input gradient actor.fc2, critic.fc2 / fc5.  gymrl_td3_update keeps them equal to
   * the parameters it writes; gymrl_td3_pack_images rebuilds them after anything else did. */
  float* images;
} gymrl_td3_update_args;
size_t gymrl_td3_update_workspace_bytes(int B, int D, int A, int H);
int gymrl_td3_pack_images(const gymrl_td3_update_args* args, void* stream);
size_t gymrl_td3_args_bytes(int which);      /* sizeof(gymrl_td3_act_args) (0) / sizeof(gymrl_td3_update_args) (1) */
int gymrl_td3_act_step(const gymrl_td3_act_args* args, void* stream);
int gymrl_td3_update(const gymrl_td3_update_args* args, void* stream);

/*
 * Discrete SAC's CartPole vector step on the same row-slab kernels (csrc/dsac_step.hip): sac_cartpole.py's select_action
 * :127-138 with the env step and memory.push of its train loop, and update :148-227.  TD3's scheme (one workgroup carries a
 * 16-row slab through a whole row phase, nothing waits for another workgroup) with three-layer networks that end in A
 * columns, an expectation over the actions in place of a sampled one, two critics with separate flat buffers and optimisers,
 * no actor target and a float32 temperature:
 *   gymrl_dsac_act_step  ONE launch (:127-138 + env.step + memory.push): actor logits on the N observations (fc1, fc2 ReLU, fc3),
 *                        gymrl_categorical_sample's draw under its keys (seed, counter, env_id0 + env; or the explicit
 *                        noise_exp rows), CartPole step with auto-reset, replay row (obs, int32 action word, reward, TERMINAL
 *                        next obs, done) at (cursor + env) % cap, the episode bookkeeping outputs
 *   gymrl_dsac_update    update() (:148-227), four launches:
 *     R1 rows   index draw (gymrl_uniform_indices' permutation, or idx) + ring gather; actor(s'), critic1_target(s'),
 *               critic2_target(s') (:173, :177-178); the softmax of csrc/softmax_device.hpp; y by gymrl_dsac_target's expression
 *               (:174-183); critic1(s), critic2(s) (:185-186); gymrl_dsac_critic_loss's gradient (:187-188); both critics'
 *               input-gradient chains
 *     T2 tiles  both critics' weight / bias gradient tiles (gymrl_lin_bwd_weight's order) + Adam (:190-196) + the Polyak
 *               update of their targets (:219-220), each over its own flat buffer; the two critic loss sums
 *     R3 rows   actor(s) + softmax; critic1(s), critic2(s) of the UPDATED critics, forward only (:198-203);
 *               gymrl_dsac_actor_loss's two terms and dL/dprobs (:204-205); the softmax backward; the actor's chain
 *     T4 tiles  actor weight gradients + Adam (:207-209); actor loss and entropy sums; gymrl_dsac_alpha_step's float32
 *               temperature step on the finished entropy sum (:211-217)
 * Results are the layer-by-layer path's bits when that path runs its softmax through gymrl_softmax_rows_fwd / _bwd
 * (tests/test_dsac_fused_step_gpu.py).  Limits: H % 4 == 0, H <= 256, D <= 8, A <= 4, B <= 256 (-22 otherwise, before any
 * launch: the trainer stays on the layer path); CartPole-v1 (D = 4, A = 2) for the act step, MountainCar-v0 and Acrobot-v1
 * through gymrl_dsac_act_step_classic.
 */
typedef struct {
  int N, D, A, H;
  int env_kind;                            /* GYMRL_ENV_CARTPOLE; the _classic entry point: also GYMRL_ENV_MOUNTAINCAR | GYMRL_ENV_ACROBOT */
  void* env_state; uint64_t env_seed; int64_t env_id0;
  const float* obs; float* obs_out;        /* f32[N, D] in / next observations out (post-reset where an episode ended) */
  const float* noise_exp;                  /* f32[N, A] Exp(1) draws, or NULL: gymrl_categorical_sample's Philox keys */
  uint64_t seed, counter; const uint64_t* counter_dev;     /* select_action's (base seed, _act_counter) */
  gymrl_td3_actor_params actor;            /* fc1, fc2, fc3: the logits */
  float* r_state; uint32_t* r_action; float* r_reward; float* r_next; uint8_t* r_flag; int64_t cap, cursor;
  const int64_t* cursor_dev;
  int32_t* action_out; float* rew_out; uint8_t* done_out; float* ep_ret_out; double* ep_stats;     /* any may be NULL */
  const float* images;                     /* gymrl_dsac_update_args.images of the same trainer, or NULL (reads actor.fc2 in place) */
} gymrl_dsac_act_args;
typedef struct {
  int B, D, A, H;
  float gamma, target_entropy;
  double tau;
  const float* r_state; const uint32_t* r_action; const float* r_reward; const float* r_next; const uint8_t* r_flag;
  const int32_t* idx;                      /* i32[B] explicit rows, or NULL: the keyed permutation of gymrl_uniform_indices */
  uint64_t idx_seed, idx_counter; int64_t idx_size; const void* idx_dev;     /* idx_dev: {uint64 counter; int64 size} */
  gymrl_td3_actor_params actor, critic1, critic2, critic1_target, critic2_target;     /* fc1, fc2, fc3 each */
  /* flat parameter buffers and their Adam moments, one set per optimiser */
  float* actor_p; float* actor_m; float* actor_v; float* critic1_p; float* critic1_m; float* critic1_v;
  float* critic2_p; float* critic2_m; float* critic2_v;
  float adam_critic1[4], adam_critic2[4], adam_actor[4];     /* gymrl_adam_bias' blocks */
  const float* adam_critic1_dev; const float* adam_critic2_dev; const float* adam_actor_dev;
  double beta1, beta2, eps_adam;           /* the critics' optimisers' (the actor's are the same defaults) */
  float* log_alpha; float* alpha_m; float* alpha_v;        /* the float32 temperature and its Adam moments */
  double lr_alpha, alpha_beta1, alpha_beta2, alpha_eps;    /* gymrl_dsac_alpha_step's arguments (rounded to float32 there) */
  int64_t alpha_t; const double* alpha_bias_dev;           /* its step count, or {1 - b1^t, 1 - b2^t} from the device */
  double* sums;                            /* f64[4] out: critic1, critic2 loss sums; actor loss sum, entropy sum */
  double* alpha_loss;                      /* f64[1] out or NULL */
  void* workspace;                         /* >= gymrl_dsac_update_workspace_bytes(B, D, A, H) */
  /* Weight images of the H x H layers (H % 16 == 0), f32[8][H*H], or NULL: forward actor.fc2, critic1.fc2, critic2.fc2,
   * critic1_target.fc2, critic2_target.fc2; input gradient actor.fc2, critic1.fc2, critic2.fc2.  gymrl_dsac_update keeps them
   * equal to the parameters it writes; gymrl_dsac_pack_images rebuilds them after anything else did. */
  float* images;
} gymrl_dsac_update_args;
size_t gymrl_dsac_update_workspace_bytes(int B, int D, int A, int H);
int gymrl_dsac_pack_images(const gymrl_dsac_update_args* args, void* stream);
size_t gymrl_dsac_args_bytes(int which);     /* sizeof(gymrl_dsac_act_args) (0) / sizeof(gymrl_dsac_update_args) (1) */
int gymrl_dsac_act_step(const gymrl_dsac_act_args* args, void* stream);
/* gymrl_dsac_act_step for the env kind args->env_kind names: GYMRL_ENV_CARTPOLE (D = 4, A = 2; the launch above), GYMRL_ENV_MOUNTAINCAR
 * (D = 2, A = 3) or GYMRL_ENV_ACROBOT (D = 6, A = 3), the stepper's own arithmetic and auto-reset in the same launch.  -22 for every
 * other kind, for a (D, A) that is not the kind's, and for what gymrl_dsac_act_step refuses. */
int gymrl_dsac_act_step_classic(const gymrl_dsac_act_args* args, void* stream);
int gymrl_dsac_update(const gymrl_dsac_update_args* args, void* stream);
/* The softmax of csrc/softmax_device.hpp over the rows of z f32[B, A] (A <= 8) and its backward dz = p (g - sum g p): what
 * ops.softmax_rows runs in place of F.softmax (sac_cartpole.py:70-80) under Config.kernel_softmax. */
int gymrl_softmax_rows_fwd(const float* z, int B, int A, float* p_out, void* stream);
int gymrl_softmax_rows_bwd(const float* p, const float* g, int B, int A, float* dz_out, void* stream);

/* ---- evolution strategies on the population evaluators (csrc/es.hip, csrc/es_noise_device.hpp; no reference script) --------
 * OpenAI-ES around one evaluation launch: mirrored sampling, centred-rank fitness shaping, the search gradient for Adam.  The
 * perturbations are drawn in registers wherever they are needed and never stored.
 *
 * The noise.  eps(seed, generation, pair k, element i), a standard normal float32:
 *   r = Philox4x32-10(key = seed; c0 = i >> 2, c1 = k, c2 = generation & 0xffffffff, c3 = 0x70000000 | ((generation >> 32) & 0x0fffffff))
 *   z0 = rho(r.x) cos(2 pi u(r.y)), z1 = rho(r.x) sin(2 pi u(r.y)), z2 = rho(r.z) cos(2 pi u(r.w)), z3 = rho(r.z) sin(2 pi u(r.w))
 *   with rho(w) = sqrtf(-2 logf(((w >> 8) + 1) * 2^-24)), u(w) = (w >> 8) * 2^-24 (the library's reproducible logf / sincosf);
 *   eps = z[i & 3]: four consecutive elements of a pair share one call, and all four words of the call are used.
 * c3's tag has the value the tabular runs' draws carry; their c0 / c1 are a run id and c2 a step, and no program draws from both.
 *
 * gymrl_es_noise       out f32[K][n] = eps for pairs k0 .. k0 + K - 1, elements 0 .. n - 1: the window of tests and tools.
 * gymrl_es_perturb     params f32[P][stride]: row 2k = theta + sigma * eps_k, row 2k + 1 = theta - sigma * eps_k, each ONE float32
 *                      multiply and ONE float32 add / subtract (no fused multiply-add); columns n .. stride - 1 are not written.
 * gymrl_es_shape_grad  returns f32[P][E] (an evaluation launch's) -> weights f32[P], grad f32[n]:
 *   fitness  F_p = the float64 sum of returns[p][e] in ascending e
 *   ranks    less_p = #{q: F_q < F_p}, equal_p = #{q: F_q == F_p} (p itself counted), by counting, no sort;
 *            w_p = (float)(2 less_p + equal_p - 1) / (float)(2 (P - 1)) - 0.5f: ties share their mean rank, all-equal fitness gives
 *            w == 0 exactly.  A NaN fitness: unspecified weights.
 *   gradient u_k = w_2k - w_2k+1 (float32); S_i = sum_k (double)u_k * (double)eps_k[i], the pairs cut into consecutive chunks of
 *            GYMRL_ES_PAIR_CHUNK, a chunk summed from 0.0 in ascending k, the chunk sums added to 0.0 in ascending chunk order, every
 *            product and sum ONE float64 operation; grad[i] = (float)(-(1.0 / ((double)P * (double)sigma)) * S_i).  Negative: an
 *            optimiser that DESCENDS grad ascends the fitness.  No atomics: the bits do not depend on the grid.
 *   P <= 256: ONE launch (every workgroup counts the ranks itself); above: a rank launch, then the gradient's.
 * -EINVAL before any launch: NULL args or a NULL pointer, n < 1, P odd or outside 2..8192, E < 1, K < 1, k0 < 0, k0 + K > 4096,
 * stride < n or stride % 4 != 0, sigma <= 0 or not finite, theta / params not 16-byte aligned (the others: 4). */
#define GYMRL_ES_PAIR_CHUNK 16
typedef struct {
  int n;                                   /* elements per pair */
  int k0;                                  /* first pair */
  int K;                                   /* pairs */
  uint64_t seed;
  uint64_t generation;
  float* out;                              /* f32[K][n] */
} gymrl_es_noise_args;
typedef struct {
  int n;                                   /* parameters */
  int P;                                   /* population, even: P / 2 mirrored pairs */
  int64_t stride;                          /* floats between rows of params: >= n, % 4 == 0 (the evaluators' policy_stride) */
  float sigma;
  uint64_t seed;
  uint64_t generation;
  const float* theta;                      /* f32[n], the centre */
  float* params;                           /* f32[P][stride] out */
} gymrl_es_perturb_args;
typedef struct {
  int n;
  int P;
  int E;                                   /* episodes per policy */
  float sigma;
  uint64_t seed;
  uint64_t generation;
  const float* returns;                    /* f32[P][E] */
  float* grad;                             /* f32[n] out */
  float* weights;                          /* f32[P] out */
} gymrl_es_shape_grad_args;
int gymrl_es_pair_chunk(void);               /* GYMRL_ES_PAIR_CHUNK */
size_t gymrl_es_noise_args_bytes(void);      /* sizeof(gymrl_es_noise_args) */
size_t gymrl_es_perturb_args_bytes(void);    /* sizeof(gymrl_es_perturb_args) */
size_t gymrl_es_shape_grad_args_bytes(void); /* sizeof(gymrl_es_shape_grad_args) */
int gymrl_es_noise(const gymrl_es_noise_args* args, void* stream);
int gymrl_es_perturb(const gymrl_es_perturb_args* args, void* stream);
int gymrl_es_shape_grad(const gymrl_es_shape_grad_args* args, void* stream);

/* ---- tabular Q-learning: a population of independent runs in one launch (csrc/tabular.hip) --------------------------------
 * Replaces QLearningTrainer.train() / select_action() / update() / _shape_reward() / eval() of qlearning_frozenlake.py:56-153
 * and qlearning_cliffwalking.py:49-124 together with the gym.make(...).reset() / .step() calls inside them (:100,105 / :75,80),
 * for n_runs runs that share one Config and differ by their random stream.  One lane = one run; its table stays in LDS for the
 * launch.  The env rules (gymnasium toy_text, third-party):
 *   FrozenLake-v1 4x4  SFFF / FHFH / FFFH / HFFG, state row * 4 + col, start 0; 0 LEFT 1 DOWN 2 RIGHT 3 UP, clipped at the border;
 *                      slippery: the executed direction is (a - 1) % 4, a, (a + 1) % 4 with probability 1/3 each; reward 1 on
 *                      entering the goal 15; terminated on a hole {5, 7, 11, 12} or the goal; truncated at the env's 100th step
 *   CliffWalking-v0    4 x 12, state row * 12 + col, start 36, goal 47; 0 UP 1 RIGHT 2 DOWN 3 LEFT, clipped; the cliff 37..46
 *                      costs -100 and returns the agent to 36 without terminating, any other step costs -1; terminated at the
 *                      goal only; no time limit
 * One run's loop, float64 in the reference's operation order: k counts its training actions from 1 (sample_count);
 * eps_table[k - 1] = end + (start - end) * exp(-k / decay) comes from the host (max_episodes * max_steps entries, shared by
 * all runs); explore iff u < eps_k with a uniform action, else the FIRST maximum of Q[s, :]; done = terminated or truncated;
 * `shaped` (FrozenLake) replaces the reward by -10 hole / 100 goal / -5 next == state / -1; target = r if done else
 * r + gamma * max Q[s', :]; Q[s, a] = Q[s, a] + lr * (target - Q[s, a]); an episode also ends after max_steps steps without
 * done.  Draws: Philox4x32-10 keyed (seed; stream lo, stream hi, k, 0x70000000), stream = run_id0 + r: words 0, 1 -> u, word 2
 * -> the exploring action (w * 4) >> 32, word 3 -> the slip choice (w * 3) >> 32 (csrc/tabular_device.hpp).
 * gymrl_qlearn_train advances every run by at most max_iters steps from the record in `state` (gymrl_qlearn_state_bytes(n_runs)
 * bytes, 256-byte aligned; restart != 0: from the start of episode 0 instead) and leaves the record for the next call, which
 * continues bit for bit.  Q f64[n_runs, S, 4] in / out (S = 16 / 48); episode_rewards f64 / episode_lengths i32
 * [n_runs, max_episodes]: entry e is written when episode e ends; k_out / episodes_out i32[n_runs]: actions taken / episodes
 * finished.  -22 for a NULL or misaligned pointer, n_runs <= 0, an unknown env kind or max_episodes * max_steps >= 2^31.
 * gymrl_qlearn_eval runs n_episodes greedy episodes per run on Q (read only), one lane each, with the env's draws from stream
 * stream_id0 + run * n_episodes + episode at k = the episode's step; an episode stops at terminated / truncated or after `cap`
 * steps.  returns f64 / lengths i32 / flags u8 [n_runs, n_episodes]: the env's own reward summed, the steps taken, and whether
 * the goal was reached (FrozenLake: the reference's success; CliffWalking: finished — its `while not done` has no cap). */
enum { GYMRL_TABULAR_FROZENLAKE = 0, GYMRL_TABULAR_CLIFFWALKING = 1 };
size_t gymrl_qlearn_state_bytes(int n_runs);
int gymrl_qlearn_train(int env_kind, int is_slippery, int shaped, double* Q, void* state, int n_runs, int restart, uint64_t seed,
                       int64_t run_id0, const double* eps_table, int max_episodes, int max_steps, int max_iters, double lr,
                       double gamma, double* episode_rewards, int32_t* episode_lengths, int32_t* k_out, int32_t* episodes_out,
                       void* stream);
int gymrl_qlearn_eval(int env_kind, int is_slippery, const double* Q, int n_runs, int n_episodes, uint64_t seed,
                      int64_t stream_id0, int cap, double* returns, int32_t* lengths, uint8_t* flags, void* stream);
/* Three more temporal-difference control rules on the same envs, draws and layout (csrc/tabular.hip: td_train_kernel; no reference
 * script).  select(s): k += 1; (u, explore, _) = the draw of (seed, stream, k); explore if u < eps_k, else the FIRST maximum of
 * the row the rule acts on.  Float64, every operation one rounding in the order written, no fused multiply-add.
 *   GYMRL_TABULAR_RULE_SARSA
 *     s = start; a = select(s)
 *     for step in range(max_steps):
 *         s2, r, done = env.step(a)              (slip word: the draw of the k that chose a)
 *         if done: target = r
 *         else:    a2 = select(s2); target = r + gamma * Q[s2, a2]
 *         Q[s, a] = Q[s, a] + lr * (target - Q[s, a])
 *         if done: break
 *         s, a = s2, a2
 *     a2 is chosen from the table BEFORE this step's write (it matters when s2 == s).  When the loop runs out at max_steps
 *     without done, the last a2 has been drawn and k has advanced; it is dropped and the next episode draws afresh.  An episode
 *     takes up to max_steps + 1 draws: eps_table needs max_episodes * (max_steps + 1) entries, and that product is the one
 *     held below 2^31.  One iteration of the kernel is one draw, so max_iters counts draws here.
 *   GYMRL_TABULAR_RULE_EXPECTED_SARSA
 *     Q-learning's loop (one select per step) with, for eps = the eps_k that select used for this step and q0..q3 = Q[s2, :]
 *     before the write,
 *         target = r + gamma * (eps * 0.25 * (((q0 + q1) + q2) + q3) + (1.0 - eps) * max(q0..q3))
 *   GYMRL_TABULAR_RULE_DOUBLE_Q
 *     Q-learning's loop on two tables.  select acts on the row QA[s, j] + QB[s, j] (one add per action, first maximum).  The
 *     coin is word 2 of the step's draw & 1; the exploring action keeps that word's top bits, (w * 4) >> 32.
 *         coin 0: a* = first maximum of QA[s2, :], target = r + gamma * QB[s2, a*], QA[s, a] = QA[s, a] + lr * (target - QA[s, a])
 *         coin 1: the same with QA and QB exchanged
 *     done gives target = r.  Greedy evaluation: gymrl_qlearn_eval on the elementwise float64 sum QA + QB, formed by the caller.
 * gymrl_tabular_train is gymrl_qlearn_train behind one struct: `rule` in front of that call's arguments, behind them Q2 (QB:
 * f64[n_runs, S, 4] for DOUBLE_Q, NULL for every other rule) and eps_len, the entries of eps_table (at least max_episodes *
 * max_steps; SARSA: max_episodes * (max_steps + 1)).  `state` holds gymrl_tabular_state_bytes(rule, n_runs) bytes (0 for an
 * unknown rule or n_runs <= 0): gymrl_qlearn_train's record and SARSA's pending action behind it, so a call continues the one
 * before it bit for bit wherever max_iters cut it.  GYMRL_TABULAR_RULE_QLEARNING writes gymrl_qlearn_train's bits.  -22 before
 * anything is launched: NULL args, what gymrl_qlearn_train refuses, an unknown rule, Q2 present or absent against the rule or
 * misaligned, eps_len shorter than the rule needs, SARSA's max_episodes * (max_steps + 1) >= 2^31.  max_iters == 0 without
 * restart: 0, nothing launched. */
enum { GYMRL_TABULAR_RULE_QLEARNING = 0, GYMRL_TABULAR_RULE_SARSA = 1, GYMRL_TABULAR_RULE_EXPECTED_SARSA = 2, GYMRL_TABULAR_RULE_DOUBLE_Q = 3 };
typedef struct {
  int rule;                                /* GYMRL_TABULAR_RULE_* */
  int env_kind, is_slippery, shaped;
  double* Q; void* state;
  int n_runs, restart;
  uint64_t seed; int64_t run_id0;
  const double* eps_table;
  int max_episodes, max_steps, max_iters;
  double lr, gamma;
  double* episode_rewards; int32_t* episode_lengths; int32_t* k_out; int32_t* episodes_out;
  double* Q2;                              /* DOUBLE_Q: QB in / out; NULL otherwise */
  int64_t eps_len;                         /* entries of eps_table */
} gymrl_tabular_train_args;
size_t gymrl_tabular_state_bytes(int rule, int n_runs);
size_t gymrl_tabular_args_bytes(void);       /* sizeof(gymrl_tabular_train_args) */
int gymrl_tabular_train(const gymrl_tabular_train_args* args, void* stream);

/* ---- separable NES on the population evaluators (csrc/es.hip; no reference script) ------------------------------------------
 * The second learner on the evolution-strategies block's noise, ranks and summation contract (above the tabular runs; tests pin
 * what follows that block, so this one stands here): a centre mu f32[n] and a step size PER ELEMENT sigma f32[n], both moved by
 * the launch that weighs the noise.  eps, F_p, w_p and GYMRL_ES_PAIR_CHUNK are that block's.
 *
 * gymrl_snes_perturb  params f32[P][stride]: row 2k = mu[i] + sigma[i] * eps_k[i], row 2k + 1 = mu[i] - sigma[i] * eps_k[i], each ONE
 *                     float32 multiply and ONE float32 add / subtract (no fused multiply-add); columns n .. stride - 1 are not
 *                     written.
 * gymrl_snes_tell     the evaluators' returns -> weights f32[P], and mu and sigma moved IN PLACE.  Exactly one of returns
 *                     (f32[P][E]) and returns64 (f64[P][E], gymrl_lunar_policy_eval's) is non-NULL.
 *   fitness  F_p = the float64 sum of row p in ascending e: for returns64 the plain double sum, for returns each term the (double)
 *            of the float.
 *   ranks    w_p as gymrl_es_shape_grad's, written to weights.
 *   sums     u_k = w_2k - w_2k+1 and s_k = w_2k + w_2k+1 (float32);
 *            Smu_i = sum_k (double)u_k * (double)eps_k[i],
 *            Ssg_i = sum_k (double)s_k * ((double)eps_k[i] * (double)eps_k[i] - 1.0),
 *            both under gymrl_es_shape_grad's summation contract: chunks of GYMRL_ES_PAIR_CHUNK pairs, a chunk summed from 0.0 in
 *            ascending k, the chunk sums added to 0.0 in ascending chunk order, every product, difference and sum ONE float64
 *            operation.  No atomics: the bits do not depend on the grid.
 *   step     c = 4.0 / (double)P (with centred ranks sum_p |c w_p| is about 1, the usual SNES utility scale);
 *            mu[i]    <- (float)((double)mu[i] + (double)eta_mu * ((double)sigma[i] * (c * Smu_i))), sigma[i] the value BEFORE the call;
 *            sigma[i] <- min(max(sigma[i] * expf((float)(0.5 * (double)eta_sigma * (c * Ssg_i))), sigma_min), sigma_max)
 *            (the library's reproducible expf; max(v, lo) = v < lo ? lo : v, min(v, hi) = v > hi ? hi : v; one float32 product).
 *            There is no optimiser launch: the thread that closes element i's chunk sums is the only one that reads or writes
 *            mu[i] and sigma[i].  All-equal fitness gives w == 0, both sums 0.0, expf(0) == 1: mu and sigma keep their bits
 *            (a sigma outside the bounds is still clamped).  A NaN fitness: unspecified.
 *   P <= 256: ONE launch (every workgroup counts the ranks itself); above: a rank launch, then the step's.
 * -EINVAL before any launch: NULL args, a NULL mu / sigma / params / weights, both or neither of returns and returns64, n < 1,
 * P odd or outside 2..8192, E < 1, stride < n or stride % 4 != 0, eta_mu or eta_sigma not finite, sigma_min or sigma_max not
 * finite or !(0 < sigma_min <= sigma_max), mu / sigma / params not 16-byte aligned, returns64 not 8-byte, the others not 4-byte. */
typedef struct {
  int n;                                   /* parameters */
  int P;                                   /* population, even: P / 2 mirrored pairs */
  int64_t stride;                          /* floats between rows of params: >= n, % 4 == 0 */
  uint64_t seed;
  uint64_t generation;
  const float* mu;                         /* f32[n], the centre */
  const float* sigma;                      /* f32[n], the step size of every element */
  float* params;                           /* f32[P][stride] out */
} gymrl_snes_perturb_args;
typedef struct {
  int n;
  int P;
  int E;                                   /* episodes per policy */
  float eta_mu;                            /* learning rate of the centre */
  float eta_sigma;                         /* learning rate of the step sizes */
  float sigma_min;                         /* 0 < sigma_min <= sigma_max */
  float sigma_max;
  uint64_t seed;
  uint64_t generation;
  const float* returns;                    /* f32[P][E], or NULL */
  const double* returns64;                 /* f64[P][E], or NULL: exactly one of the two */
  float* mu;                               /* f32[n], in place */
  float* sigma;                            /* f32[n], in place */
  float* weights;                          /* f32[P] out */
} gymrl_snes_tell_args;
size_t gymrl_snes_perturb_args_bytes(void);  /* sizeof(gymrl_snes_perturb_args) */
size_t gymrl_snes_tell_args_bytes(void);     /* sizeof(gymrl_snes_tell_args) */
int gymrl_snes_perturb(const gymrl_snes_perturb_args* args, void* stream);
int gymrl_snes_tell(const gymrl_snes_tell_args* args, void* stream);

/* ----------------------------- Acrobot-v1 policies: whole episodes in one launch ---- */
/*
 * gymrl_mountaincar_net_eval (below: the three nets, the trunk, policy_stride, images, the outputs — all as described there) for
 * Acrobot-v1, (D, A) = (6, 3), TimeLimit 500 (csrc/eval_net.hip; the same kernels of csrc/eval_kernels_device.hpp and the
 * same episode loop of csrc/eval_episode_device.hpp, instantiated for env kind 5).  The state (th1, th2, dth1, dth2) is float64
 * in the lane's registers, the observation the six float32 of the rule at the head of this file, one step is csrc/
 * env_classic_device.hpp's acrobot_advance — the stepper's RK4 step — on the 16 lanes of the first wave, and the return takes -1 on
 * every step but a terminating one.  Episode i = p * E + e starts from the reset draw of (seed, stream_id0 + e, episode 0) or from
 * start[i].
 * -EINVAL before any launch: gymrl_mountaincar_net_eval's list with cap outside 1..500.
 */
typedef struct {
  int P, E, cap;
  int net;                                 /* 0: three-layer MLP | 1: dueling, torch's mean | 2: dueling, the DUELING epilogue's mean */
  int n_hidden, H;                         /* hidden layers of the trunk (net 0: 2; net 1 | 2: 1 | 2) and their width */
  const float* w[2]; const float* b[2];    /* fc1 [H][6], fc2 [H][H] and their biases, of policy 0; entry 1 is NULL when n_hidden == 1 */
  const float* head_w; const float* head_b;        /* net 0: fc3 [3][H], [3]; net 1 | 2: the advantage head [3][H], [3] */
  const float* value_w; const float* value_b;      /* net 1 | 2: the value head [1][H], [1]; net 0: NULL */
  int64_t policy_stride;                   /* floats between consecutive policies' tensors; 0 with P == 1 */
  const float* images;                     /* the forward image of fc2 (n_hidden == 2, H % 16 == 0, P == 1), or NULL: fc2 is read in place */
  uint64_t seed; int64_t stream_id0;
  const double* start;                     /* f64[P * E][4] (th1, th2, dth1, dth2), or NULL: the reset draw */
  float* returns; int32_t* lengths; uint8_t* terminated;
  float* final_obs;                        /* f32[P * E][6] or NULL */
} gymrl_acrobot_net_eval_args;
size_t gymrl_acrobot_net_eval_args_bytes(void);  /* sizeof(gymrl_acrobot_net_eval_args) */
int gymrl_acrobot_net_eval(const gymrl_acrobot_net_eval_args* args, void* stream);

/*
 * DQN's CartPole vector step on the same row-slab kernels (csrc/dqn_step.hip): dqn_cartpole.py's select_action :124-133 with
 * the env step and memory.push of its train loop :178-184, and update :135-168.  Discrete SAC's scheme with ONE online network
 * and its hard-copied target (two chains in the row phase where dSAC runs five), epsilon-greedy in place of the categorical
 * draw, and the reference's +-1 gradient clamp (:163-165) inside the tile kernel's Adam:
 *   gymrl_dqn_act_step   ONE launch (:124-133 + env.step + memory.push): policy_net on the N observations (net.0, net.2 ReLU,
 *                        net.4), gymrl_epsilon_greedy's choice under its keys (seed, counter, env_id0 + env; or the explicit
 *                        u rows) with epsilon / epsilon_dev[0], CartPole step with auto-reset, replay row (obs, int32 action
 *                        word, reward, TERMINAL next obs, done) at (cursor + env) % cap, the episode bookkeeping outputs
 *   gymrl_dqn_update     update() (:135-168), two launches:
 *     R1 rows   index draw (gymrl_uniform_indices' permutation, or idx) + ring gather; policy_net(s) and target_net(s') as two
 *               items of the same stages (:150-155); gymrl_dqn_td_loss's expressions for plain DQN (no online selector, no
 *               weights, gamma_n = gamma): a* = first argmax of the target row, y = r + gamma q' (1 - d), td, dq = 2 td / B
 *               on the taken action, the row's float64 td^2 (:157-161); the policy net's input-gradient chain
 *     T2 tiles  weight / bias gradient tiles (gymrl_lin_bwd_weight's order), each element clamped to +-clamp_abs, Adam
 *               (:162-166; gymrl_adam_step's arithmetic); the loss sum in gymrl_dqn_td_loss's order (B <= 256: one block's)
 *   The target network is read only: the hard copy (:193-194) stays with the caller, as does rebuilding the images after it.
 * Results are the layer-by-layer path's bits (tests/test_dqn_fused_step_gpu.py).  Limits: H % 4 == 0, H <= 256, D <= 8, A <= 4,
 * B <= 256 (-22 otherwise, before any launch: the trainer stays on the layer path); CartPole-v1 (D = 4, A = 2) for the act step,
 * MountainCar-v0 and Acrobot-v1 through gymrl_dqn_act_step_classic.
 */
typedef struct {
  int N, D, A, H;
  int env_kind;                            /* GYMRL_ENV_CARTPOLE; the _classic entry point: also GYMRL_ENV_MOUNTAINCAR | GYMRL_ENV_ACROBOT */
  void* env_state; uint64_t env_seed; int64_t env_id0;
  const float* obs; float* obs_out;        /* f32[N, D] in / next observations out (post-reset where an episode ended) */
  const float* u;                          /* f32[N, 2] uniforms {explore?, which action}, or NULL: gymrl_epsilon_greedy's Philox keys */
  uint64_t seed, counter; const uint64_t* counter_dev;     /* select_action's (base seed, _act_counter) */
  float epsilon; const float* epsilon_dev; /* get_epsilon()'s value as float32, or the same from the device (hipGraph replay) */
  gymrl_td3_actor_params policy;           /* net.0, net.2, net.4: the Q values */
  float* r_state; uint32_t* r_action; float* r_reward; float* r_next; uint8_t* r_flag; int64_t cap, cursor;
  const int64_t* cursor_dev;
  int32_t* action_out; float* rew_out; uint8_t* done_out; float* ep_ret_out; double* ep_stats;     /* any may be NULL */
  const float* images;                     /* gymrl_dqn_update_args.images of the same trainer, or NULL (reads net.2 in place) */
} gymrl_dqn_act_args;
typedef struct {
  int B, D, A, H;
  float gamma;
  const float* r_state; const uint32_t* r_action; const float* r_reward; const float* r_next; const uint8_t* r_flag;
  const int32_t* idx;                      /* i32[B] explicit rows, or NULL: the keyed permutation of gymrl_uniform_indices */
  uint64_t idx_seed, idx_counter; int64_t idx_size; const void* idx_dev;     /* idx_dev: {uint64 counter; int64 size} */
  gymrl_td3_actor_params policy, target;   /* net.0, net.2, net.4 each; the target is read only */
  float* policy_p; float* policy_m; float* policy_v;       /* the policy net's flat parameter buffer and its Adam moments */
  float adam_policy[4];                    /* gymrl_adam_bias' block */
  const float* adam_policy_dev;
  double beta1, beta2, eps_adam;
  float clamp_abs;                         /* gymrl_adam_step's clamp_abs (the reference: 1; 0: no clamp) */
  double* loss_sum;                        /* f64[1] out: sum of td^2 */
  void* workspace;                         /* >= gymrl_dqn_update_workspace_bytes(B, D, A, H) */
  /* Weight images of the H x H layer (H % 16 == 0), f32[3][H*H], or NULL: forward policy net.2, forward target net.2, input
   * gradient policy net.2.  gymrl_dqn_update keeps the policy's two equal to the parameters it writes; gymrl_dqn_pack_images
   * rebuilds all three after anything else wrote a parameter (the hard target copy, load_state_dict, a checkpoint, ...). */
  float* images;
} gymrl_dqn_update_args;
size_t gymrl_dqn_update_workspace_bytes(int B, int D, int A, int H);
int gymrl_dqn_pack_images(const gymrl_dqn_update_args* args, void* stream);
size_t gymrl_dqn_args_bytes(int which);      /* sizeof(gymrl_dqn_act_args) (0) / sizeof(gymrl_dqn_update_args) (1) */
int gymrl_dqn_act_step(const gymrl_dqn_act_args* args, void* stream);
/* gymrl_dqn_act_step for the env kind args->env_kind names: GYMRL_ENV_CARTPOLE (D = 4, A = 2; the launch above), GYMRL_ENV_MOUNTAINCAR
 * (D = 2, A = 3) or GYMRL_ENV_ACROBOT (D = 6, A = 3), the stepper's own arithmetic and auto-reset in the same launch; u stays
 * f32[N, 2] (u0 against epsilon, u1 the exploring action min((int)(u1 * A), A - 1)).  -22 for every other kind, for a (D, A) that is not
 * the kind's, and for what gymrl_dqn_act_step refuses.  gymrl_dqn_update and the non-dueling gymrl_ddqn_update take these shapes. */
int gymrl_dqn_act_step_classic(const gymrl_dqn_act_args* args, void* stream);
int gymrl_dqn_update(const gymrl_dqn_update_args* args, void* stream);

/*
 * Double DQN + prioritised replay's update on the same row-slab kernels (csrc/ddqn_step.hip): ddqn_per_cartpole.py's update
 * :197-244 between its sample() and its update_priorities().  gymrl_dqn_update with a third forward chain, a weight per row and
 * the TD errors as an output; acting is gymrl_dqn_act_step (the network is fc1, fc2 ReLU, fc3, the shape of DQN's), and the
 * stratified draw stays gymrl_per_sample(variant_b = 1): its weights' maximum is a reduction over the whole batch.
 *   gymrl_ddqn_update    two launches:
 *     R1 rows   ring gather by idx; policy_net(s), policy_net(s') and target_net(s') as three items of the same stages
 *               (:222-228); gymrl_dqn_td_loss's expressions with q_next_online and w: a* = first argmax of the online row,
 *               y = r + gamma q_target'[a*] (1 - d), td = q[a] - y -> td_out, dq = 2 td w / B on the taken action, the row's
 *               float64 td^2 w (:229-232); the policy net's input-gradient chain
 *     T2 tiles  as gymrl_dqn_update's: weight / bias gradient tiles, each element clamped to +-clamp_abs, Adam (:237-242); the
 *               loss sum in gymrl_dqn_td_loss's order
 *   The caller runs gymrl_per_update_td(idx, td_out, alpha, eps, clip = error_max) behind it (:234-235) and owns the hard
 *   target copy and the images' rebuild after it.
 * Results are the layer-by-layer path's bits (tests/test_ddqn_fused_step_gpu.py).  Limits: H % 4 == 0, H <= 256, D <= 8, A <= 4,
 * B <= 256 (-22 otherwise, before any launch: the trainer stays on the layer path).
 */
typedef struct {
  int B, D, A, H;
  int dueling;                             /* 0: fc1, fc2, fc3.  1: ddqn_per_duel_cartpole.py's net, policy / target = {fc1, value_stream
                                            * [1][H], advantage_stream [A][H]}, q = v + (a - mean a); A == 2; no images */
  float gamma;
  const float* r_state; const uint32_t* r_action; const float* r_reward; const float* r_next; const uint8_t* r_flag;
  int64_t cap;                             /* rows of the ring: an idx outside [0, cap) is not read (a zero row of weight 0) */
  const int32_t* idx;                      /* i32[B] ring rows of the sampled batch (gymrl_per_sample's tree index - cap + 1) */
  const float* is_weight;                  /* f32[B] importance weights (gymrl_per_sample's w_out) */
  gymrl_td3_actor_params policy, target;   /* fc1, fc2, fc3 each; the target is read only */
  float* policy_p; float* policy_m; float* policy_v;       /* the policy net's flat parameter buffer and its Adam moments */
  float adam_policy[4];                    /* gymrl_adam_bias' block */
  const float* adam_policy_dev;
  double beta1, beta2, eps_adam;
  float clamp_abs;                         /* gymrl_adam_step's clamp_abs (the reference: 1; 0: no clamp) */
  float* td_out;                           /* f32[B] out: the TD errors, for gymrl_per_update_td */
  double* loss_sum;                        /* f64[1] out: sum of td^2 * w */
  void* workspace;                         /* >= gymrl_ddqn_update_workspace_bytes(B, D, A, H) */
  float* images;                           /* f32[3][H*H] or NULL: gymrl_dqn_update_args.images' layout and rules (gymrl_ddqn_pack_images) */
} gymrl_ddqn_update_args;
size_t gymrl_ddqn_update_workspace_bytes(int B, int D, int A, int H);
int gymrl_ddqn_pack_images(const gymrl_ddqn_update_args* args, void* stream);
size_t gymrl_ddqn_args_bytes(int which);     /* sizeof(gymrl_ddqn_update_args) (1), 0 otherwise: there is no act struct of its own */
int gymrl_ddqn_update(const gymrl_ddqn_update_args* args, void* stream);
/* gymrl_dqn_act_step for the dueling network: args->policy = {fc1, value_stream, advantage_stream}, the combine in front of the
 * epsilon-greedy choice (gymrl_epsilon_greedy's keys); args->images is not read. */
int gymrl_ddqn_duel_act_step(const gymrl_dqn_act_args* args, void* stream);

/*
 * NoisyNet dueling DQN's CartPole vector step on the same row-slab kernels (csrc/noisy_dqn_step.hip): noisy_dqn_cartpole.py's
 * select_action :198-212 with the env step and memory.push of its train loop, and update :214-257.  All four layers are
 * NoisyLinear (fc1 D -> H, fc2 H -> H, value_stream H -> 1, advantage_stream H -> A), so a step first forms the EFFECTIVE
 * parameters W = mu + sigma * (eps_out (x) eps_in), b = mu + sigma * eps_out of its three draws, and the other launches read them:
 *   gymrl_ndqn_combine   ONE launch: set 0 = C (acting), set 1 = A (policy_net(states): the gradient flows through it), set 2 = B
 *                        (policy_net(next_states): the double-Q choice) into `workspace`; eps = f(Box-Muller on Philox(seed[layer],
 *                        counter[set]; stream 0 input side / 1 output side; element)), f(x) = sign(x) sqrt|x| — gymrl_noisy_noise's
 *                        bits for the same (seed, counter) — or f of the raw N(0,1) rows raw[set]; set A's eps vectors are kept
 *   gymrl_ndqn_act_step  ONE launch: the Q values on set C, q = v + (a - mean a), argmax (the first maximum), CartPole step with
 *                        auto-reset, replay row (obs, int32 action word, reward, TERMINAL next obs, done) at (cursor + env) % cap
 *   gymrl_ndqn_update    update(), three launches behind a gymrl_ndqn_combine:
 *     R1 rows   index draw (gymrl_uniform_indices' permutation, or idx) + ring gather; policy(s) on set A, policy(s') on set B,
 *               target(s') on the target's mu; a* = first argmax of the online row, y = r + gamma q_target'[a*] (1 - d),
 *               td = q[a] - y, dq = 2 td / B on the taken action (F.mse_loss: no weights, no clamp), the row's float64 td^2;
 *               the combine's backward and set A's input-gradient chain.  A row outside [0, cap) is a zero row without gradient
 *     T2 tiles  dW / db of set A's effective parameters (gymrl_lin_bwd_weight's order); the loss sum (gymrl_dqn_td_loss's order)
 *     A3        d mu = dW, d sigma = dW * eps_A (biases: db * eps_out), Adam on mu and sigma (gymrl_adam_step's arithmetic)
 *   The target network is read only (its mu): the hard copy stays with the caller.
 * Results are the layer-by-layer path's bits (tests/test_ndqn_fused_step_gpu.py).  Limits: A == 2, H % 4 == 0, H <= 256, D <= 8,
 * B <= 256 (-22 otherwise, before any launch: the trainer stays on the layer path); CartPole-v1 (D = 4) for the act step.
 * A raw row holds, per layer in the forward's order, the K input-side draws and then the N output-side draws:
 * (D + H) + (H + H) + (H + 1) + (H + A) floats.
 */
typedef struct { float* w_mu[4]; float* w_sigma[4]; float* b_mu[4]; float* b_sigma[4]; } gymrl_ndqn_params;     /* fc1, fc2, value_stream, advantage_stream */
typedef struct {
  int D, A, H;
  gymrl_ndqn_params policy;                /* read only here */
  uint64_t seed[4];                        /* per layer */
  uint64_t counter[3]; const uint64_t* counter_dev;     /* per set (C, A, B); counter_dev: u64[3] on the device (hipGraph replay) */
  const float* raw[3];                     /* per set: f32 raw row (parity mode), or NULL: the Philox draw */
  void* workspace;                         /* >= gymrl_ndqn_update_workspace_bytes(B, D, A, H) of the trainer's B */
} gymrl_ndqn_combine_args;
typedef struct {
  int N, D, A, H;
  int env_kind;                            /* GYMRL_ENV_CARTPOLE */
  void* env_state; uint64_t env_seed; int64_t env_id0;
  const float* obs; float* obs_out;        /* f32[N, D] in / next observations out (post-reset where an episode ended) */
  float* r_state; uint32_t* r_action; float* r_reward; float* r_next; uint8_t* r_flag; int64_t cap, cursor;
  const int64_t* cursor_dev;
  int32_t* action_out; float* rew_out; uint8_t* done_out; float* ep_ret_out; double* ep_stats;     /* any may be NULL */
  const void* workspace;                   /* the gymrl_ndqn_combine workspace: set C is read */
} gymrl_ndqn_act_args;
typedef struct {
  int B, D, A, H;
  float gamma;
  const float* r_state; const uint32_t* r_action; const float* r_reward; const float* r_next; const uint8_t* r_flag;
  int64_t cap;                             /* rows of the ring: an idx outside [0, cap) is not read */
  const int32_t* idx;                      /* i32[B] explicit rows, or NULL: the keyed permutation of gymrl_uniform_indices */
  uint64_t idx_seed, idx_counter; int64_t idx_size; const void* idx_dev;     /* idx_dev: {uint64 counter; int64 size} */
  gymrl_ndqn_params policy, target;        /* the target: its w_mu / b_mu are read, nothing is written */
  float* policy_p; float* policy_m; float* policy_v;       /* the policy net's flat parameter buffer and its Adam moments */
  float adam_policy[4];                    /* gymrl_adam_bias' block */
  const float* adam_policy_dev;
  double beta1, beta2, eps_adam;
  double* loss_sum;                        /* f64[1] out: sum of td^2 */
  void* workspace;                         /* the gymrl_ndqn_combine workspace: sets A and B are read, the hand-off lives behind them */
} gymrl_ndqn_update_args;
size_t gymrl_ndqn_args_bytes(int which);     /* sizeof(gymrl_ndqn_act_args) (0) / _update_args (1) / _combine_args (2) */
int gymrl_ndqn_combine(const gymrl_ndqn_combine_args* args, void* stream);
int gymrl_ndqn_act_step(const gymrl_ndqn_act_args* args, void* stream);
size_t gymrl_ndqn_update_workspace_bytes(int B, int D, int A, int H);
int gymrl_ndqn_update(const gymrl_ndqn_update_args* args, void* stream);

/* ----------------------------- MountainCar-v0 policies: whole episodes in one launch ---- */
/*
 * gymrl_classic_policy_eval and gymrl_classic_duel_eval (the section below: grid, lanes, uniform exit, starts, policy_stride,
 * outputs — all as described there) for MountainCar-v0, (D, A) = (2, 3), TimeLimit 200 (csrc/eval_net.hip; the kernels
 * and the episode loop are the ones below, stated once in csrc/eval_kernels_device.hpp and csrc/eval_episode_device.hpp).  The
 * state (position, velocity) is float64 in the lane's registers, the observation its float32 cast, one step is
 * csrc/env_classic_device.hpp's mountaincar_advance — the stepper's — and the return takes -1 on every step, the terminating one
 * included.  Episode i = p * E + e starts from the reset draw of (seed, stream_id0 + e, episode 0) or from start[i].
 *
 *   net 0  a three-layer MLP 2 -> H -> H -> 3: n_hidden = 2, head_w / head_b = fc3, value_w / value_b NULL; the action is the
 *          FIRST maximum of fc3's row (gymrl_epsilon_greedy's greedy branch, gymrl_categorical_sample's deterministic one).
 *   net 1  a dueling network: a ReLU trunk of n_hidden layers (1 | 2), value_w [1][H], head_w [3][H] = the advantage head, both
 *          in one two-item stage; q = v + (a - mean a) with the mean as ((a0 + a2) + a1) * (1 / 3) — torch's mean of a row of three — and the
 *          first maximum of q.  A NoisyLinear layer is passed as its weight_mu / bias_mu.
 *   net 2  the same network with the combine of gymrl_lin_fwd's GYMRL_ACT_DUELING epilogue (Rainbow's layer path):
 *          q = v + (a - ((a0 + a1) + (a2 + 0)) / 3).  From three actions on the two means are different floats.
 *
 * -EINVAL before any launch: NULL args, a NULL w[0] / b[0] / head_w / head_b / returns / lengths / terminated, P < 1, E < 1, cap
 * outside 1..200, net outside 0..2, n_hidden other than 2 with net 0 or outside {1, 2}, a non-NULL value_w / value_b with net 0 or
 * a NULL one with net 1 | 2, a NULL w[1] / b[1] with n_hidden == 2 or a non-NULL one with n_hidden == 1, H % 4 != 0 or H outside
 * 4..256, a negative policy_stride or one that is not a multiple of 4, policy_stride == 0 with P > 1, images with P > 1, with
 * n_hidden == 1 or with H % 16 != 0, P * E above INT32_MAX, stream_id0 < 0, a pointer that is not aligned (the weights, images: 16
 * bytes; start: 8; the others: 4).
 */
typedef struct {
  int P, E, cap;
  int net;                                 /* 0: three-layer MLP | 1: dueling, torch's mean | 2: dueling, the DUELING epilogue's mean */
  int n_hidden, H;                         /* hidden layers of the trunk (net 0: 2; net 1 | 2: 1 | 2) and their width */
  const float* w[2]; const float* b[2];    /* fc1 [H][2], fc2 [H][H] and their biases, of policy 0; entry 1 is NULL when n_hidden == 1 */
  const float* head_w; const float* head_b;        /* net 0: fc3 [3][H], [3]; net 1 | 2: the advantage head [3][H], [3] */
  const float* value_w; const float* value_b;      /* net 1 | 2: the value head [1][H], [1]; net 0: NULL */
  int64_t policy_stride;                   /* floats between consecutive policies' tensors; 0 with P == 1 */
  const float* images;                     /* the forward image of fc2 (n_hidden == 2, H % 16 == 0, P == 1), or NULL: fc2 is read in place */
  uint64_t seed; int64_t stream_id0;
  const double* start;                     /* f64[P * E][2] (position, velocity), or NULL: the reset draw */
  float* returns; int32_t* lengths; uint8_t* terminated;
  float* final_obs;                        /* f32[P * E][2] or NULL */
} gymrl_mountaincar_net_eval_args;
size_t gymrl_mountaincar_net_eval_args_bytes(void);  /* sizeof(gymrl_mountaincar_net_eval_args) */
int gymrl_mountaincar_net_eval(const gymrl_mountaincar_net_eval_args* args, void* stream);

/* ----------------------------- classic-control policies: whole episodes in one launch ---- */
/*
 * Replaces the eval() loops of dqn_cartpole.py:214-233, ddqn_per_cartpole.py, sac_cartpole.py, td3_pendulum.py and
 * ddpg_pendulum.py (select_action without exploration -> env.step, up to the TimeLimit) for P policies x E episodes at a time
 * (csrc/eval_classic.hip).  ONE workgroup of 1024 threads carries 16 episodes of one policy from reset to their end; the grid is
 * P * ceil(E / 16) workgroups.  Per step: lanes 0..15 of the first wave put the float32 observation of their float64 register
 * state into LDS, all sixteen waves run the D -> H -> H -> A forward (fc1, fc2 ReLU, fc3: the row-slab stages of the fused acting
 * kernels, so the bits are gymrl_lin_fwd's), the lanes take the action and advance their env in registers (csrc/
 * env_classic_device.hpp: the stepper's own cartpole_advance / pendulum_advance).  A finished lane idles with its state, return and
 * length frozen; the workgroup leaves when all 16 are finished (at `cap` at the latest) on one LDS word behind a barrier every
 * thread reaches.  No atomics, nothing waits for another workgroup, and inside the loop global memory is only read (the weights).
 *
 *   head 0  argmax: the FIRST maximum of fc3's row — gymrl_epsilon_greedy's greedy branch, gymrl_categorical_sample's
 *           deterministic one.  CartPole-v1 only, (D, A) = (4, 2).
 *   head 1  tanh: action = tanh(fc3) * bound, gymrl_td3_act_step's expression in front of its noise.  Pendulum-v1 only, (3, 1).
 *
 * Policy p reads w[k] + p * policy_stride and b[k] + p * policy_stride (floats; 0: P == 1).  Episode i = p * E + e starts from the
 * reset draw of (seed, stream_id0 + e, episode 0) — the SAME starts for every policy, the first episode of env e of a
 * gymrl_env_reset with env_id0 = stream_id0 — or from start[i] = the float64 state (x, x_dot, theta, theta_dot | theta, theta_dot).
 *
 * Outputs, each [P * E]: returns (the float32 cast of the float64 return: gymrl_env_step's ep_ret_out), lengths, terminated (1:
 * the env terminated on the last step; 0: the episode was cut at `cap` steps, the TimeLimit included), final_obs [P * E][D]
 * (optional) the observation after the last step (gymrl_env_step's term_obs_out).
 * -EINVAL before any launch: NULL args, a NULL w[k] / b[k] / returns / lengths / terminated, P < 1, E < 1, cap outside 1..TimeLimit
 * (500 / 200), an env kind other than CartPole-v1 / Pendulum-v1, a (head, D, A) that is not the kind's, H % 4 != 0 or H outside
 * 4..256, a negative policy_stride or one that is not a multiple of 4, policy_stride == 0 with P > 1, images with P > 1, P * E
 * above INT32_MAX, stream_id0 < 0, a pointer that is not aligned (w[k], images: 16 bytes; start: 8; the others: 4).
 * SAC-Pendulum's greedy action tanh(mean(fc2(fc1 s))) * bound is head 1 on (fc1, fc2, mean).  Dueling networks: the entry point below.
 * MountainCar-v0: gymrl_mountaincar_net_eval above, Acrobot-v1: gymrl_acrobot_net_eval further up (LunarLander-v3 under a PPO policy: gymrl_lunar_policy_eval below).
 */
typedef struct {
  int P, E, cap;
  int env_kind;                            /* GYMRL_ENV_CARTPOLE | GYMRL_ENV_PENDULUM */
  int head, D, A, H;
  float bound;                             /* head 1: the action bound */
  const float* w[3]; const float* b[3];    /* fc1 [H][D], fc2 [H][H], fc3 [A][H] and their biases, of policy 0 */
  int64_t policy_stride;                   /* floats between consecutive policies' tensors; 0 with P == 1 */
  const float* images;                     /* the forward image of fc2 (H % 16 == 0; P == 1), or NULL: fc2 is read in place */
  uint64_t seed; int64_t stream_id0;
  const double* start;                     /* f64[P * E][4 | 2], or NULL: the reset draw */
  float* returns; int32_t* lengths; uint8_t* terminated;
  float* final_obs;                        /* f32[P * E][D] or NULL */
} gymrl_classic_eval_args;
size_t gymrl_classic_eval_args_bytes(void);  /* sizeof(gymrl_classic_eval_args) */
int gymrl_classic_policy_eval(const gymrl_classic_eval_args* args, void* stream);

/*
 * The same launch for a DUELING network on CartPole-v1 (csrc/eval_duel.hip; the episode loop is the one above, stated once in
 * csrc/eval_episode_device.hpp): replaces the eval() loops of ddqn_per_duel_cartpole.py, noisy_dqn_cartpole.py and
 * rainbow_dqn_cartpole.py.  In evaluation mode the three networks are one function: a ReLU trunk of n_hidden layers (1: fc1; 2:
 * fc1, fc2), a value head [1][H] and an advantage head [A][H] on its output — both in ONE two-item row-slab stage, as
 * gymrl_ndqn_act_step runs them — q = v + (a - mean a) with the mean as sum * (1 / A), and the FIRST maximum of q.  A NoisyLinear
 * layer is passed as its weight_mu / bias_mu: no noise is drawn.  Grid, lanes, exit, starts, policy_stride (which shifts every
 * pointer of the block) and the outputs are gymrl_classic_policy_eval's.
 * -EINVAL before any launch: NULL args, a NULL w[0] / b[0] / value_w / value_b / adv_w / adv_b / returns / lengths / terminated,
 * P < 1, E < 1, cap outside 1..500, an env kind other than CartPole-v1, (D, A) other than (4, 2), n_hidden outside {1, 2}, a NULL
 * w[1] / b[1] with n_hidden == 2 or a non-NULL one with n_hidden == 1, H % 4 != 0 or H outside 4..256, a negative policy_stride or
 * one that is not a multiple of 4, policy_stride == 0 with P > 1, images with P > 1, with n_hidden == 1 or with H % 16 != 0,
 * P * E above INT32_MAX, stream_id0 < 0, a pointer that is not aligned (the weights, images: 16 bytes; start: 8; the others: 4).
 */
typedef struct {
  int P, E, cap;
  int env_kind;                            /* GYMRL_ENV_CARTPOLE */
  int n_hidden, D, A, H;                   /* hidden layers of the trunk (1 | 2); (D, A) = (4, 2) */
  const float* w[2]; const float* b[2];    /* fc1 [H][D], fc2 [H][H] and their biases, of policy 0; entry 1 is NULL when n_hidden == 1 */
  const float* value_w; const float* value_b;      /* the value head [1][H], [1] */
  const float* adv_w; const float* adv_b;          /* the advantage head [A][H], [A] */
  int64_t policy_stride;                   /* floats between consecutive policies' tensors; 0 with P == 1 */
  const float* images;                     /* the forward image of fc2 (n_hidden == 2, H % 16 == 0, P == 1), or NULL: fc2 is read in place */
  uint64_t seed; int64_t stream_id0;
  const double* start;                     /* f64[P * E][4], or NULL: the reset draw */
  float* returns; int32_t* lengths; uint8_t* terminated;
  float* final_obs;                        /* f32[P * E][4] or NULL */
} gymrl_classic_duel_eval_args;
size_t gymrl_classic_duel_eval_args_bytes(void);  /* sizeof(gymrl_classic_duel_eval_args) */
int gymrl_classic_duel_eval(const gymrl_classic_duel_eval_args* args, void* stream);

/* ------------------------------------------- MountainCar-v0 rule baseline ---- */
/*
 * Replaces RuleBasedAgent.select_action() / run_episode() / eval() of mountaincar_baseline.py:35-84 together with the
 * gym.make(...).reset() / .step() calls inside them, P policies x E episodes at a time.  An episode is a strictly serial chain of
 * at most 200 steps of six float64 operations and one cos; P * E of them are independent, so one LANE is one (policy p,
 * episode e) pair, i = p * E + e, and they all run to their end in one launch: position, velocity, step count and the nine
 * coefficients stay in registers, no LDS, no atomics, a wave leaves the loop when its last episode is over.
 *
 * The env is GYMRL_ENV_MOUNTAINCAR's (csrc/env_classic_device.hpp: the same device function steps both); episode i starts from
 * the reset draw of (seed, stream_id0 + i, episode 0), i.e. the first episode of env i of a gymrl_env_reset with
 * env_id0 = stream_id0, or from start[i] = (position, velocity) where `start` is given.
 *
 * The policy is select_action with its nine constants as k[0..8] (the reference's: -0.09, 0.25, 0.03, 0.3, 0.9, 0.008, -0.07,
 * 0.38, 0.07), in float64 on the float32 observation, powers as products:
 *   p = (double)(float)pos, v = (double)(float)vel
 *   lb = min(k0 * (p + k1)^2 + k2, k3 * (p + k4)^4 - k5), ub = k6 * (p + k7)^2 + k8, action = lb < v && v < ub ? 2 : 0
 *
 * Outputs, each [P * E]: returns (-1 per step), lengths, reached (1: the env terminated; 0: the episode was cut at `cap`
 * steps, the env's TimeLimit 200 included), final_state [P * E][2] (optional) the float64 state after the last step.
 * -EINVAL before any launch: NULL args or a NULL required output, P < 1, E < 1, cap outside 1..200, coefs == NULL with P != 1,
 * P * E above INT32_MAX, stream_id0 < 0, a pointer that is not aligned to its element.
 */
typedef struct {
  int P, E, cap;
  uint64_t seed; int64_t stream_id0;
  const double* coefs;                     /* f64[P][9], or NULL: the reference's constants (P == 1) */
  const double* start;                     /* f64[P * E][2] (position, velocity), or NULL: the reset draw */
  double* returns; int32_t* lengths; uint8_t* reached;
  double* final_state;                     /* f64[P * E][2] or NULL */
} gymrl_mountaincar_eval_args;
int gymrl_mountaincar_rule_eval(const gymrl_mountaincar_eval_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMRL_H */
