"""Plain-Python float64 restatement of Acrobot-v1 (reset, the RK4 step, wrap and clamp, termination, TimeLimit, auto-reset) and of
the episode loop, written from the rule in include/gymrl.h.  Test infrastructure: no GPU, no gymrl_amd import.

sin / cos are the oracle's orc_sincos (the host restatement of the device's det_sincos) and the reset draw goes through
oracle.philox; python floats are IEEE float64 and every expression keeps the header's grouping, so the kernels' observations,
flags, returns and float64 states are compared with array_equal.
"""
import ctypes as C
import math

import numpy as np

from oracle import oracle as orc

RNG_ENV_RESET = 0x10000000
EVAL_STREAM0 = 1 << 40
MAX_STEPS = 500
WRAP_TRIPS = 8                       # GYMRL_ACROBOT_WRAP_TRIPS
PI = 3.14159265358979323846
MAX_VEL_1, MAX_VEL_2 = 4.0 * PI, 9.0 * PI

_sincos = None


def det_sincos(x):
    """(sin x, cos x) as the device computes them (csrc/gymrl_device.hpp det_sincos == oracle orc_sincos)."""
    global _sincos
    if _sincos is None:
        fn = orc.lib().orc_sincos
        fn.restype, fn.argtypes = None, [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _sincos = fn
    s, c = C.c_double(), C.c_double()
    _sincos(float(x), C.byref(s), C.byref(c))
    return s.value, c.value


def libm_sincos(x):
    return math.sin(x), math.cos(x)


def _u01d(hi, lo):
    return (float(hi >> 5) * 67108864.0 + float(lo >> 6)) * 2.0 ** -53


def draw(seed, stream, episode=0):
    """reset: U(-0.1, 0.1)^4 from the words of Philox(seed, stream, episode, RNG_ENV_RESET | 0) and | 1, as CartPole-v1 takes them."""
    a = orc.philox(seed, stream & 0xFFFFFFFF, stream >> 32, episode, RNG_ENV_RESET | 0)
    b = orc.philox(seed, stream & 0xFFFFFFFF, stream >> 32, episode, RNG_ENV_RESET | 1)
    return (-0.1 + 0.2 * _u01d(a[0], a[1]), -0.1 + 0.2 * _u01d(a[2], a[3]), -0.1 + 0.2 * _u01d(b[0], b[1]),
            -0.1 + 0.2 * _u01d(b[2], b[3]))


def deriv(y, a, sincos=det_sincos):
    """f(th1, th2, dth1, dth2; a) of the header."""
    th1, th2, dth1, dth2 = y
    half_pi = PI / 2.0
    s2, c2 = sincos(th2)
    _, c12 = sincos(th1 + th2 - half_pi)
    _, c1 = sincos(th1 - half_pi)
    d1 = 0.25 + (1.25 + c2) + 1.0 + 1.0
    d2 = (0.25 + 0.5 * c2) + 1.0
    phi2 = 4.9 * c12
    phi1 = -0.5 * (dth2 * dth2) * s2 - dth2 * dth1 * s2 + (1.5 * 9.8) * c1 + phi2
    ddth2 = (a + d2 / d1 * phi1 - 0.5 * (dth1 * dth1) * s2 - phi2) / (1.25 - d2 * d2 / d1)
    ddth1 = -(d2 * ddth2 + phi1) / d1
    return dth1, dth2, ddth1, ddth2


def rk4(y, action, sincos=det_sincos):
    """One classical RK4 step over dt = 0.2, before wrap and clamp."""
    a = float(action - 1)
    k1 = deriv(y, a, sincos)
    k2 = deriv(tuple(y[i] + 0.1 * k1[i] for i in range(4)), a, sincos)
    k3 = deriv(tuple(y[i] + 0.1 * k2[i] for i in range(4)), a, sincos)
    k4 = deriv(tuple(y[i] + 0.2 * k3[i] for i in range(4)), a, sincos)
    return tuple(y[i] + (0.2 / 6.0) * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) for i in range(4))


def wrap(x):
    """-> (x wrapped towards [-pi, pi], trips a `while` loop would have taken): WRAP_TRIPS conditional steps down, then up."""
    trips = 0
    for _ in range(WRAP_TRIPS):
        if x > PI:
            x, trips = x - 2.0 * PI, trips + 1
    for _ in range(WRAP_TRIPS):
        if x < -PI:
            x, trips = x + 2.0 * PI, trips + 1
    return x, trips


def clamp(x, bound):
    return -bound if x < -bound else (bound if x > bound else x)


def height_reached(th1, th2, sincos=det_sincos):
    _, c1 = sincos(th1)
    _, c12 = sincos(th2 + th1)
    return -c1 - c12 > 1.0


def advance(y, action, sincos=det_sincos):
    """One env step -> ((th1, th2, dth1, dth2), terminated)."""
    th1, th2, dth1, dth2 = rk4(y, action, sincos)
    y = (wrap(th1)[0], wrap(th2)[0], clamp(dth1, MAX_VEL_1), clamp(dth2, MAX_VEL_2))
    return y, height_reached(y[0], y[1], sincos)


def obs_of(y):
    """The float32 observation (cos th1, sin th1, cos th2, sin th2, dth1, dth2)."""
    s1, c1 = det_sincos(y[0])
    s2, c2 = det_sincos(y[1])
    return np.array([c1, s1, c2, s2, y[2], y[3]], np.float64).astype(np.float32)


# ---- host policies on the float32 observation o = (cos th1, sin th1, cos th2, sin th2, dth1, dth2) and the step index t -------
def pump(o, t=0):
    """The energy pump: torque against the first link's velocity — -1 (action 0) while dth1 >= 0, +1 (action 2) while it is
    negative.  From the reset draws it swings the tip over the line in 70 to 130 steps; the opposite sign never does."""
    return 0 if o[4] >= 0 else 2


def idle(o, t=0):
    return 1


def cycle(o, t=0):
    """The fixed action cycle 0, 1, 2, 0, .."""
    return t % 3


POLICIES = {"pump": pump, "idle": idle, "cycle": cycle}


def actions(obs, act, t=0):
    """act on every row of obs f32[N, 6] at step t -> i32[N]: the host policy of the stepper tests."""
    return np.array([act(o, t) for o in np.asarray(obs, np.float32)], np.int32)


def episode(y, act=pump, cap=MAX_STEPS):
    """One episode from the state y -> dict(ret, len, terminated, state, obs)."""
    ret, steps, terminated = 0.0, 0, False
    while steps < cap and not terminated:
        y, terminated = advance(y, act(obs_of(y), steps))
        ret, steps = ret + (0.0 if terminated else -1.0), steps + 1
    return dict(ret=ret, len=steps, terminated=terminated, state=y, obs=obs_of(y))


def eval_population(seed, stream_id0, E, acts, start=None, cap=MAX_STEPS):
    """What gymrl_acrobot_net_eval returns for P host policies `acts` -> (returns f32, lengths i32, terminated u8, final_obs
    f32[.., 6]), each [P, E]; episode e of every policy starts from the draw of stream_id0 + e, or from start[p][e]."""
    out = [[episode(draw(seed, stream_id0 + e) if start is None else tuple(float(v) for v in start[p][e]), act, cap)
            for e in range(E)] for p, act in enumerate(acts)]
    return (np.array([[o["ret"] for o in r] for r in out], np.float64).astype(np.float32),
            np.array([[o["len"] for o in r] for r in out], np.int32), np.array([[o["terminated"] for o in r] for r in out], np.uint8),
            np.array([[o["obs"] for o in r] for r in out], np.float32))


def stepper_trace(seed, env_id, act, T, abandon_cap=0, start=None):
    """T vector steps of ONE env of the batched stepper under the host policy `act` (fed the observation the stepper returned),
    with auto-reset; abandon_cap > 0 also runs gymrl_env_abandon(cap) after every step; start: the state written over the reset
    draw.  -> dict of [T] arrays: obs / term_obs f32[T, 6], rew f32, terminated / truncated / done / abandoned u8, ep_ret_out f32
    and ep_len_out i32 (0 where no episode ended at that step), action i32, and the state after the step: state f64[T, 4], ep_ret
    f64, ep_len i32, episode u32; obs0 f32[6]."""
    y = draw(seed, env_id, 0) if start is None else tuple(float(v) for v in start)
    ep_ret, ep_len, ep = 0.0, 0, 0
    obs0 = obs_of(y)
    o = obs0
    rows = []
    for t in range(T):
        a = act(o, t)
        y, terminated = advance(y, a)
        rew = 0.0 if terminated else -1.0
        length, ret = ep_len + 1, ep_ret + rew
        truncated = length >= MAX_STEPS
        done = terminated or truncated
        term = obs_of(y)
        ret_out, len_out, abandoned = 0.0, 0, False
        if done:
            ep += 1
            y = draw(seed, env_id, ep)
            ep_ret, ep_len, ret_out, len_out = 0.0, 0, ret, length
            o = obs_of(y)
        else:
            ep_ret, ep_len, o = ret, length, term
        if abandon_cap and ep_len >= abandon_cap:
            ret_out, len_out, abandoned = ep_ret, ep_len, True
            ep += 1
            y = draw(seed, env_id, ep)
            ep_ret, ep_len = 0.0, 0
            o = obs_of(y)
        rows.append((o, term, rew, terminated, truncated, done, abandoned, ret_out, len_out, a, y, ep_ret, ep_len, ep))
    col = lambda j, dt: np.array([r[j] for r in rows], dt)   # noqa: E731
    return dict(obs0=obs0, obs=col(0, np.float32), term_obs=col(1, np.float32), rew=col(2, np.float32),
                terminated=col(3, np.uint8), truncated=col(4, np.uint8), done=col(5, np.uint8), abandoned=col(6, np.uint8),
                ep_ret_out=col(7, np.float32), ep_len_out=col(8, np.int32), action=col(9, np.int32), state=col(10, np.float64),
                ep_ret=col(11, np.float64), ep_len=col(12, np.int32), episode=col(13, np.uint32))


def stepper_traces(seed, env_id0, N, act, T, abandon_cap=0, starts=None):
    """stepper_trace of envs env_id0 .. env_id0 + N - 1, stacked: every array becomes [T, N, ...] (obs0: [N, 6]); starts = {env
    index: state} overrides single envs' reset draws."""
    starts = starts or {}
    traces = [stepper_trace(seed, env_id0 + i, act, T, abandon_cap, starts.get(i)) for i in range(N)]
    return {k: np.stack([t[k] for t in traces], axis=0 if k == "obs0" else 1) for k in traces[0]}
