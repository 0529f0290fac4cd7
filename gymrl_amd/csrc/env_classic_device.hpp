// env_classic_device.hpp — CartPole-v1 / Pendulum-v1 / MountainCar-v0 / Acrobot-v1: state layout, reset draws and ONE env's step as device functions.
//
// The arithmetic of gym.make("CartPole-v1" | "Pendulum-v1" | "MountainCar-v0" | "Acrobot-v1").step()/reset() (gymnasium classic_control, third-party:
// SURVEY.md 8c.2) for one env = one lane.  Shared by the stand-alone steppers (env_classic.hip: gymrl_env_step) and the
// fused acting kernels (offpolicy_step.hip, rainbow_step.hip, td3_step.hip: forward + draw + env step + ring append in one launch), so both produce the
// same bits; each env's register-only core (*_advance) is shared with its one-launch episode kernels (mountaincar.hip; EpisodeEnv at the end of this file) in the same way.  State is float64 like gymnasium's, observations are the float32 cast; sin / cos are det_sincos.
#pragma once
#include "env_common.hpp"

namespace gymrl {

// The widths and the TimeLimit of an env kind, written here and nowhere else under csrc/: observations, actions (Pendulum-v1: the
// one torque), float64 fields of a state, gymnasium's max_episode_steps.  The steppers below, the size queries (env_classic.hip),
// the episode kernels (EpisodeEnv at the end of this file) and PPO's kernels (classic_ppo_device.hpp: ClassicEnv) read them.
template <int KIND> struct ClassicDims;
template <> struct ClassicDims<GYMRL_ENV_CARTPOLE> { static constexpr int kObs = 4, kActions = 2, kState = 4, kMaxSteps = 500; };
template <> struct ClassicDims<GYMRL_ENV_PENDULUM> { static constexpr int kObs = 3, kActions = 1, kState = 2, kMaxSteps = 200; };
template <> struct ClassicDims<GYMRL_ENV_MOUNTAINCAR> { static constexpr int kObs = 2, kActions = 3, kState = 2, kMaxSteps = 200; };
template <> struct ClassicDims<GYMRL_ENV_ACROBOT> { static constexpr int kObs = 6, kActions = 3, kState = 4, kMaxSteps = 500; };

struct CartPoleState {
  double *x, *xd, *th, *thd;
  EpisodeFields ep;
  __host__ __device__ CartPoleState(void* buf, int n) {
    Carver c(buf, n);
    x = c.take<double>(); xd = c.take<double>(); th = c.take<double>(); thd = c.take<double>();
    ep.ep_ret = c.take<double>(); ep.ep_len = c.take<int32_t>(); ep.episode = c.take<uint32_t>();
    bytes = c.off;
  }
  size_t bytes;
};

struct PendulumState {
  double *th, *thd;
  EpisodeFields ep;
  size_t bytes;
  __host__ __device__ PendulumState(void* buf, int n) {
    Carver c(buf, n);
    th = c.take<double>(); thd = c.take<double>();
    ep.ep_ret = c.take<double>(); ep.ep_len = c.take<int32_t>(); ep.episode = c.take<uint32_t>();
    bytes = c.off;
  }
};

struct MountainCarState {
  double *pos, *vel;
  EpisodeFields ep;
  size_t bytes;
  __host__ __device__ MountainCarState(void* buf, int n) {
    Carver c(buf, n);
    pos = c.take<double>(); vel = c.take<double>();
    ep.ep_ret = c.take<double>(); ep.ep_len = c.take<int32_t>(); ep.episode = c.take<uint32_t>();
    bytes = c.off;
  }
};

struct AcrobotState {
  double *th1, *th2, *dth1, *dth2;
  EpisodeFields ep;
  size_t bytes;
  __host__ __device__ AcrobotState(void* buf, int n) {
    Carver c(buf, n);
    th1 = c.take<double>(); th2 = c.take<double>(); dth1 = c.take<double>(); dth2 = c.take<double>();
    ep.ep_ret = c.take<double>(); ep.ep_len = c.take<int32_t>(); ep.episode = c.take<uint32_t>();
    bytes = c.off;
  }
};

__device__ __forceinline__ void cartpole_draw(uint64_t seed, uint64_t env, uint32_t episode,
                                              double (&s)[4]) {
  // reset: U(-0.05, 0.05)^4 in float64 (gymnasium CartPoleEnv.reset)
  const u32x4 a = philox4x32(seed, (uint32_t)env, (uint32_t)(env >> 32), episode, RNG_ENV_RESET | 0u);
  const u32x4 b = philox4x32(seed, (uint32_t)env, (uint32_t)(env >> 32), episode, RNG_ENV_RESET | 1u);
  s[0] = -0.05 + 0.1 * u01d(a.x, a.y);
  s[1] = -0.05 + 0.1 * u01d(a.z, a.w);
  s[2] = -0.05 + 0.1 * u01d(b.x, b.y);
  s[3] = -0.05 + 0.1 * u01d(b.z, b.w);
}

__device__ __forceinline__ void pendulum_draw(uint64_t seed, uint64_t env, uint32_t episode,
                                              double& th, double& thd) {
  const u32x4 a = philox4x32(seed, (uint32_t)env, (uint32_t)(env >> 32), episode, RNG_ENV_RESET | 0u);
  const double pi = 3.14159265358979323846;
  th = -pi + (2.0 * pi) * u01d(a.x, a.y);
  thd = -1.0 + 2.0 * u01d(a.z, a.w);
}

__device__ __forceinline__ void mountaincar_draw(uint64_t seed, uint64_t env, uint32_t episode,
                                                 double& pos, double& vel) {
  // reset: position U(-0.6, -0.4), velocity 0 (gymnasium MountainCarEnv.reset)
  const u32x4 a = philox4x32(seed, (uint32_t)env, (uint32_t)(env >> 32), episode, RNG_ENV_RESET | 0u);
  pos = -0.6 + 0.2 * u01d(a.x, a.y);
  vel = 0.0;
}

__device__ __forceinline__ void acrobot_draw(uint64_t seed, uint64_t env, uint32_t episode, double (&s)[4]) {
  // reset: U(-0.1, 0.1)^4 in float64 from cartpole_draw's words (gymnasium AcrobotEnv.reset; its float32 rounding of the state is not modelled)
  const u32x4 a = philox4x32(seed, (uint32_t)env, (uint32_t)(env >> 32), episode, RNG_ENV_RESET | 0u);
  const u32x4 b = philox4x32(seed, (uint32_t)env, (uint32_t)(env >> 32), episode, RNG_ENV_RESET | 1u);
  s[0] = -0.1 + 0.2 * u01d(a.x, a.y);
  s[1] = -0.1 + 0.2 * u01d(a.z, a.w);
  s[2] = -0.1 + 0.2 * u01d(b.x, b.y);
  s[3] = -0.1 + 0.2 * u01d(b.z, b.w);
}

__device__ __forceinline__ void pendulum_obs(double th, double thd, float (&o)[3]) {
  double s, c;
  det_sincos(th, &s, &c);
  o[0] = (float)c; o[1] = (float)s; o[2] = (float)thd;
}

__device__ __forceinline__ void acrobot_obs(const double (&s)[4], float (&o)[6]) {
  double s1, c1, s2, c2;
  det_sincos(s[0], &s1, &c1);
  det_sincos(s[1], &s2, &c2);
  o[0] = (float)c1; o[1] = (float)s1; o[2] = (float)c2; o[3] = (float)s2; o[4] = (float)s[2]; o[5] = (float)s[3];
}

// What one env's step hands back: the observation the policy sees next (post-reset where the episode ended), the
// terminal observation (what off-policy buffers store as next_state), reward, flags, and the finished episode's
// return / length (valid where done).
template <int D>
struct ClassicStep {
  float o_next[D], o_term[D];
  float reward;
  bool terminated, truncated, done;
  double ret;
  int len;
};

// CartPole-v1, registers only: explicit Euler with the pre-step velocities; -> terminated (beyond |x| > 2.4 or |theta| > 12 degrees).
// The stepper below and the policy episode kernel (eval_classic.hip) both call it.
__device__ __forceinline__ bool cartpole_advance(double& x, double& xd, double& th, double& thd, int action) {
  const double force = action == 1 ? 10.0 : -10.0;
  double s, c;
  det_sincos(th, &s, &c);                          // not ocml: reproducible on the host bit for bit
  const double temp = (force + 0.05 * (thd * thd) * s) / 1.1;
  const double thacc = (9.8 * s - c * temp) / (0.5 * (4.0 / 3.0 - 0.1 * (c * c) / 1.1));
  const double xacc = temp - 0.05 * thacc * c / 1.1;
  x = x + 0.02 * xd; xd = xd + 0.02 * xacc;
  th = th + 0.02 * thd; thd = thd + 0.02 * thacc;
  const double th_lim = 12.0 * 2.0 * 3.14159265358979323846 / 360.0;
  return x < -2.4 || x > 2.4 || th < -th_lim || th > th_lim;
}

// CartPole-v1: reward 1 on every step including the terminating one, the TimeLimit; auto-reset into episode + 1's draw.
__device__ __forceinline__ void cartpole_step_one(const CartPoleState& st, int i, uint64_t seed, int64_t env_id0, int action,
                                                  ClassicStep<4>& r) {
  double x = st.x[i], xd = st.xd[i], th = st.th[i], thd = st.thd[i];
  r.terminated = cartpole_advance(x, xd, th, thd, action);
  r.len = st.ep.ep_len[i] + 1;
  r.truncated = r.len >= ClassicDims<GYMRL_ENV_CARTPOLE>::kMaxSteps;
  r.done = r.terminated || r.truncated;
  r.ret = st.ep.ep_ret[i] + 1.0;
  r.reward = 1.0f;
  r.o_term[0] = (float)x; r.o_term[1] = (float)xd; r.o_term[2] = (float)th; r.o_term[3] = (float)thd;
  if (r.done) {
    const uint32_t e = st.ep.episode[i] + 1u;
    double d[4];
    cartpole_draw(seed, (uint64_t)(env_id0 + i), e, d);
    st.x[i] = d[0]; st.xd[i] = d[1]; st.th[i] = d[2]; st.thd[i] = d[3];
    st.ep.ep_ret[i] = 0.0; st.ep.ep_len[i] = 0; st.ep.episode[i] = e;
    r.o_next[0] = (float)d[0]; r.o_next[1] = (float)d[1]; r.o_next[2] = (float)d[2]; r.o_next[3] = (float)d[3];
  } else {
    st.x[i] = x; st.xd[i] = xd; st.th[i] = th; st.thd[i] = thd;
    st.ep.ep_ret[i] = r.ret; st.ep.ep_len[i] = r.len;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.o_next[k] = r.o_term[k];
  }
}

// Pendulum-v1, registers only: torque clipped to +-2, cost from the PRE-step state, speed clipped to +-8; -> cost (the reward is
// its negative).  The stepper below and the policy episode kernel (eval_classic.hip) both call it.
__device__ __forceinline__ double pendulum_advance(double& th, double& thd, float action) {
  const double pi = 3.14159265358979323846;
  double u = (double)action;
  u = u < -2.0 ? -2.0 : (u > 2.0 ? 2.0 : u);
  // angle_normalize(x) = ((x + pi) mod 2pi) - pi with python's floor-mod
  double a = th + pi;
  a = a - floor(a / (2.0 * pi)) * (2.0 * pi);
  const double an = a - pi;
  const double cost = an * an + 0.1 * (thd * thd) + 0.001 * (u * u);
  double sin_th, cos_th;
  det_sincos(th, &sin_th, &cos_th);
  double nthd = thd + (15.0 * sin_th + 3.0 * u) * 0.05;    // 3g/(2l) = 15, 3/(ml^2) = 3
  nthd = nthd < -8.0 ? -8.0 : (nthd > 8.0 ? 8.0 : nthd);
  th = th + nthd * 0.05;
  thd = nthd;
  return cost;
}

// Pendulum-v1: never terminates, the TimeLimit; auto-reset into episode + 1's draw.
__device__ __forceinline__ void pendulum_step_one(const PendulumState& st, int i, uint64_t seed, int64_t env_id0, float action,
                                                  ClassicStep<3>& r) {
  double nth = st.th[i], nthd = st.thd[i];
  const double cost = pendulum_advance(nth, nthd, action);
  r.len = st.ep.ep_len[i] + 1;
  r.terminated = false;
  r.truncated = r.len >= ClassicDims<GYMRL_ENV_PENDULUM>::kMaxSteps;
  r.done = r.truncated;
  r.ret = st.ep.ep_ret[i] + (-cost);
  r.reward = (float)(-cost);
  pendulum_obs(nth, nthd, r.o_term);
  if (r.done) {
    const uint32_t e = st.ep.episode[i] + 1u;
    double rth, rthd;
    pendulum_draw(seed, (uint64_t)(env_id0 + i), e, rth, rthd);
    st.th[i] = rth; st.thd[i] = rthd;
    st.ep.ep_ret[i] = 0.0; st.ep.ep_len[i] = 0; st.ep.episode[i] = e;
    pendulum_obs(rth, rthd, r.o_next);
  } else {
    st.th[i] = nth; st.thd[i] = nthd;
    st.ep.ep_ret[i] = r.ret; st.ep.ep_len[i] = r.len;
    r.o_next[0] = r.o_term[0]; r.o_next[1] = r.o_term[1]; r.o_next[2] = r.o_term[2];
  }
}

// MountainCar-v0, registers only: force 0.001 per action step against gravity 0.0025 * cos(3 pos), speed clipped to +-0.07,
// position to [-1.2, 0.6], the left wall is inelastic; -> terminated (at or past 0.5 and not moving left).  The stepper below
// and the episode kernel (mountaincar.hip) both call it.
__device__ __forceinline__ bool mountaincar_advance(double& pos, double& vel, int action) {
  double s, c;
  det_sincos(3.0 * pos, &s, &c);
  vel = vel + (((double)(action - 1)) * 0.001 + c * (-0.0025));
  vel = vel < -0.07 ? -0.07 : (vel > 0.07 ? 0.07 : vel);
  pos = pos + vel;
  pos = pos < -1.2 ? -1.2 : (pos > 0.6 ? 0.6 : pos);
  if (pos == -1.2 && vel < 0.0) vel = 0.0;
  return pos >= 0.5 && vel >= 0.0;
}

// MountainCar-v0: reward -1 on every step including the terminating one, the TimeLimit; auto-reset into episode + 1's draw.
__device__ __forceinline__ void mountaincar_step_one(const MountainCarState& st, int i, uint64_t seed, int64_t env_id0, int action,
                                                     ClassicStep<2>& r) {
  double pos = st.pos[i], vel = st.vel[i];
  r.terminated = mountaincar_advance(pos, vel, action);
  r.len = st.ep.ep_len[i] + 1;
  r.truncated = r.len >= ClassicDims<GYMRL_ENV_MOUNTAINCAR>::kMaxSteps;
  r.done = r.terminated || r.truncated;
  r.ret = st.ep.ep_ret[i] + (-1.0);
  r.reward = -1.0f;
  r.o_term[0] = (float)pos; r.o_term[1] = (float)vel;
  if (r.done) {
    const uint32_t e = st.ep.episode[i] + 1u;
    double rp, rv;
    mountaincar_draw(seed, (uint64_t)(env_id0 + i), e, rp, rv);
    st.pos[i] = rp; st.vel[i] = rv;
    st.ep.ep_ret[i] = 0.0; st.ep.ep_len[i] = 0; st.ep.episode[i] = e;
    r.o_next[0] = (float)rp; r.o_next[1] = (float)rv;
  } else {
    st.pos[i] = pos; st.vel[i] = vel;
    st.ep.ep_ret[i] = r.ret; st.ep.ep_len[i] = r.len;
    r.o_next[0] = r.o_term[0]; r.o_next[1] = r.o_term[1];
  }
}

// Acrobot-v1 (gymnasium's "book" dynamics, torque_noise_max = 0), registers only.  acrobot_deriv is the right-hand side
// f(th1, th2, dth1, dth2; a) of include/gymrl.h with the unit masses, lengths and inertias multiplied out (m1 = m2 = l1 = I1 =
// I2 = 1, lc1 = lc2 = 0.5, g = 9.8: every folded product is exact but 1.5 * 9.8, which the compiler rounds as the host does).
__device__ __forceinline__ void acrobot_deriv(const double (&y)[4], double a, double (&k)[4]) {
  const double half_pi = 3.14159265358979323846 / 2.0;
  double s2, c2, sn, c12, c1;
  det_sincos(y[1], &s2, &c2);
  det_sincos(y[0] + y[1] - half_pi, &sn, &c12);
  det_sincos(y[0] - half_pi, &sn, &c1);
  const double d1 = 0.25 + (1.25 + c2) + 1.0 + 1.0;
  const double d2 = (0.25 + 0.5 * c2) + 1.0;
  const double phi2 = 4.9 * c12;
  const double phi1 = -0.5 * (y[3] * y[3]) * s2 - y[3] * y[2] * s2 + (1.5 * 9.8) * c1 + phi2;
  const double ddth2 = (a + d2 / d1 * phi1 - 0.5 * (y[2] * y[2]) * s2 - phi2) / (1.25 - d2 * d2 / d1);
  const double ddth1 = -(d2 * ddth2 + phi1) / d1;
  k[0] = y[2]; k[1] = y[3]; k[2] = ddth1; k[3] = ddth2;
}

constexpr int kAcrobotWrapTrips = GYMRL_ACROBOT_WRAP_TRIPS;       // gymnasium's `while x > pi: x -= 2 pi` as a fixed trip count

// One classical RK4 step over dt = 0.2, the angles wrapped into [-pi, pi], the velocities clamped to +-4 pi / +-9 pi; ->
// terminated (the tip above the line one link length over the pivot, on the new state).  The stepper below and the policy
// episode kernels (EpisodeEnv below) both call it.
__device__ __forceinline__ bool acrobot_advance(double (&s)[4], int action) {
  const double pi = 3.14159265358979323846;
  const double a = (double)(action - 1);
  double k1[4], k2[4], k3[4], k4[4], y[4];
  acrobot_deriv(s, a, k1);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + 0.1 * k1[i];
  acrobot_deriv(y, a, k2);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + 0.1 * k2[i];
  acrobot_deriv(y, a, k3);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + 0.2 * k3[i];
  acrobot_deriv(y, a, k4);
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = s[i] + (0.2 / 6.0) * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    double x = s[i];
#pragma unroll
    for (int w = 0; w < kAcrobotWrapTrips; ++w) x = x > pi ? x - 2.0 * pi : x;
#pragma unroll
    for (int w = 0; w < kAcrobotWrapTrips; ++w) x = x < -pi ? x + 2.0 * pi : x;
    s[i] = x;
  }
  s[2] = s[2] < -4.0 * pi ? -4.0 * pi : (s[2] > 4.0 * pi ? 4.0 * pi : s[2]);
  s[3] = s[3] < -9.0 * pi ? -9.0 * pi : (s[3] > 9.0 * pi ? 9.0 * pi : s[3]);
  double sn, c1, c12;
  det_sincos(s[0], &sn, &c1);
  det_sincos(s[1] + s[0], &sn, &c12);
  return -c1 - c12 > 1.0;
}

// Acrobot-v1: reward -1 on every step but the terminating one (0), the TimeLimit; auto-reset into episode + 1's draw.
__device__ __forceinline__ void acrobot_step_one(const AcrobotState& st, int i, uint64_t seed, int64_t env_id0, int action,
                                                 ClassicStep<6>& r) {
  double s[4] = {st.th1[i], st.th2[i], st.dth1[i], st.dth2[i]};
  r.terminated = acrobot_advance(s, action);
  r.len = st.ep.ep_len[i] + 1;
  r.truncated = r.len >= ClassicDims<GYMRL_ENV_ACROBOT>::kMaxSteps;
  r.done = r.terminated || r.truncated;
  const double rew = r.terminated ? 0.0 : -1.0;
  r.ret = st.ep.ep_ret[i] + rew;
  r.reward = (float)rew;
  acrobot_obs(s, r.o_term);
  if (r.done) {
    const uint32_t e = st.ep.episode[i] + 1u;
    double d[4];
    acrobot_draw(seed, (uint64_t)(env_id0 + i), e, d);
    st.th1[i] = d[0]; st.th2[i] = d[1]; st.dth1[i] = d[2]; st.dth2[i] = d[3];
    st.ep.ep_ret[i] = 0.0; st.ep.ep_len[i] = 0; st.ep.episode[i] = e;
    acrobot_obs(d, r.o_next);
  } else {
    st.th1[i] = s[0]; st.th2[i] = s[1]; st.dth1[i] = s[2]; st.dth2[i] = s[3];
    st.ep.ep_ret[i] = r.ret; st.ep.ep_len[i] = r.len;
#pragma unroll
    for (int k = 0; k < 6; ++k) r.o_next[k] = r.o_term[k];
  }
}

// What an env kind is to the kernels that STEP it inside a launch of their own — PPO's rollout and evaluation (classic_ppo_device.hpp)
// and the DQN-family act kernels (slab_step_device.hpp: classic_act_tail): ClassicDims, the view of the env state buffer, ONE env's
// step with auto-reset (gymrl_env_step's arithmetic, above), and the vector an observation row of PPO's slab is stored with — 16
// bytes are one float4, 8 and 24 bytes are one and three float2, Pendulum-v1's 12 bytes are three floats.
template <int KIND> struct ClassicEnv;
template <> struct ClassicEnv<GYMRL_ENV_CARTPOLE> : ClassicDims<GYMRL_ENV_CARTPOLE> {
  using State = CartPoleState;
  using ObsVec = float4;
  static __device__ __forceinline__ void step(const State& st, int i, uint64_t seed, int64_t env_id0, int action, ClassicStep<4>& r) {
    cartpole_step_one(st, i, seed, env_id0, action, r);
  }
};
template <> struct ClassicEnv<GYMRL_ENV_MOUNTAINCAR> : ClassicDims<GYMRL_ENV_MOUNTAINCAR> {
  using State = MountainCarState;
  using ObsVec = float2;
  static __device__ __forceinline__ void step(const State& st, int i, uint64_t seed, int64_t env_id0, int action, ClassicStep<2>& r) {
    mountaincar_step_one(st, i, seed, env_id0, action, r);
  }
};
template <> struct ClassicEnv<GYMRL_ENV_ACROBOT> : ClassicDims<GYMRL_ENV_ACROBOT> {
  using State = AcrobotState;
  using ObsVec = float2;
  static __device__ __forceinline__ void step(const State& st, int i, uint64_t seed, int64_t env_id0, int action, ClassicStep<6>& r) {
    acrobot_step_one(st, i, seed, env_id0, action, r);
  }
};
// Pendulum-v1 (PPO's Gaussian rollout only): the action is the float torque, and a 12-byte observation row is three scalar stores —
// row i starts 12 i bytes into the slab, so nothing wider than 4 bytes is aligned for every i.
template <> struct ClassicEnv<GYMRL_ENV_PENDULUM> : ClassicDims<GYMRL_ENV_PENDULUM> {
  using State = PendulumState;
  using ObsVec = float;
  static __device__ __forceinline__ void step(const State& st, int i, uint64_t seed, int64_t env_id0, float action, ClassicStep<3>& r) {
    pendulum_step_one(st, i, seed, env_id0, action, r);
  }
};

// What an env kind is to the one-launch episode kernels (eval_episode_device.hpp: run_episodes): ClassicDims, the action its policy
// hands over (an index, or Pendulum-v1's float torque), and three register-only pieces on the lane's float64 state s[kState] —
//
//   draw      the reset of the stream's first episode (the steppers' draw at episode 0)
//   obs       the float32 observation of s, o[kObs]
//   advance   one step under `action`, the undiscounted reward added to `ret` in float64 as the stepper above adds it; -> terminated
//
// A fifth env is one more ClassicDims and one more EpisodeEnv; the loop, the kernels and the launcher take it as a template argument.
template <int KIND> struct EpisodeEnv;
template <> struct EpisodeEnv<GYMRL_ENV_CARTPOLE> : ClassicDims<GYMRL_ENV_CARTPOLE> {
  using Action = int;
  static __device__ __forceinline__ void draw(uint64_t seed, uint64_t stream, double (&s)[4]) { cartpole_draw(seed, stream, 0u, s); }
  static __device__ __forceinline__ void obs(const double (&s)[4], float* o) {
    o[0] = (float)s[0]; o[1] = (float)s[1]; o[2] = (float)s[2]; o[3] = (float)s[3];
  }
  static __device__ __forceinline__ bool advance(double (&s)[4], int action, double& ret) {
    const bool terminated = cartpole_advance(s[0], s[1], s[2], s[3], action);
    ret = ret + 1.0;
    return terminated;
  }
};
template <> struct EpisodeEnv<GYMRL_ENV_PENDULUM> : ClassicDims<GYMRL_ENV_PENDULUM> {
  using Action = float;
  static __device__ __forceinline__ void draw(uint64_t seed, uint64_t stream, double (&s)[4]) { pendulum_draw(seed, stream, 0u, s[0], s[1]); }
  static __device__ __forceinline__ void obs(const double (&s)[4], float* o) {
    float ob[3];
    pendulum_obs(s[0], s[1], ob);
    o[0] = ob[0]; o[1] = ob[1]; o[2] = ob[2];
  }
  static __device__ __forceinline__ bool advance(double (&s)[4], float action, double& ret) {
    ret = ret + (-pendulum_advance(s[0], s[1], action));
    return false;
  }
};
template <> struct EpisodeEnv<GYMRL_ENV_MOUNTAINCAR> : ClassicDims<GYMRL_ENV_MOUNTAINCAR> {
  using Action = int;
  static __device__ __forceinline__ void draw(uint64_t seed, uint64_t stream, double (&s)[4]) { mountaincar_draw(seed, stream, 0u, s[0], s[1]); }
  static __device__ __forceinline__ void obs(const double (&s)[4], float* o) { o[0] = (float)s[0]; o[1] = (float)s[1]; }
  static __device__ __forceinline__ bool advance(double (&s)[4], int action, double& ret) {
    const bool terminated = mountaincar_advance(s[0], s[1], action);
    ret = ret + (-1.0);                 // every step, the terminating one included
    return terminated;
  }
};
template <> struct EpisodeEnv<GYMRL_ENV_ACROBOT> : ClassicDims<GYMRL_ENV_ACROBOT> {
  using Action = int;
  static __device__ __forceinline__ void draw(uint64_t seed, uint64_t stream, double (&s)[4]) { acrobot_draw(seed, stream, 0u, s); }
  static __device__ __forceinline__ void obs(const double (&s)[4], float* o) {
    float ob[6];
    acrobot_obs(s, ob);
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = ob[k];
  }
  static __device__ __forceinline__ bool advance(double (&s)[4], int action, double& ret) {
    const bool terminated = acrobot_advance(s, action);
    ret = ret + (terminated ? 0.0 : -1.0);  // every step but the terminating one
    return terminated;
  }
};

}  // namespace gymrl
