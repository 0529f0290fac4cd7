"""Plain-Python float64 restatement of MountainCar-v0 (reset, step, TimeLimit, auto-reset), the rule policy of
mountaincar_baseline.py and the episode loop, written from the rules in include/gymrl.h.  Test infrastructure: no GPU, no
gymrl_amd import.

cos is the oracle's orc_sincos (the host restatement of the device's det_sincos) and the reset draw goes through oracle.philox;
python floats are IEEE float64 and every expression keeps the header's operation order, so the kernels' observations, flags,
returns and float64 states are compared with array_equal.
"""
import ctypes as C
import math

import numpy as np

from oracle import oracle as orc

RNG_ENV_RESET = 0x10000000
EVAL_STREAM0 = 1 << 40
MAX_STEPS = 200
RULE_COEFS = (-0.09, 0.25, 0.03, 0.3, 0.9, 0.008, -0.07, 0.38, 0.07)

_sincos = None


def det_cos(x):
    """cos(x) as the device computes it (csrc/gymrl_device.hpp det_sincos == oracle orc_sincos)."""
    global _sincos
    if _sincos is None:
        fn = orc.lib().orc_sincos
        fn.restype, fn.argtypes = None, [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _sincos = fn
    s, c = C.c_double(), C.c_double()
    _sincos(float(x), C.byref(s), C.byref(c))
    return c.value


def f32(x):
    return float(np.float32(x))


def draw(seed, stream, episode=0):
    """reset: position U(-0.6, -0.4) from words 0, 1 of Philox(seed, stream, episode, RNG_ENV_RESET | 0), velocity 0."""
    x, y, _, _ = orc.philox(seed, stream & 0xFFFFFFFF, stream >> 32, episode, RNG_ENV_RESET)
    u = (float(x >> 5) * 67108864.0 + float(y >> 6)) * 2.0 ** -53
    return -0.6 + 0.2 * u, 0.0


def advance(pos, vel, action, cos=det_cos):
    """One step of the dynamics -> (pos, vel, terminated)."""
    c = cos(3.0 * pos)
    vel = vel + (float(action - 1) * 0.001 + c * (-0.0025))
    vel = -0.07 if vel < -0.07 else (0.07 if vel > 0.07 else vel)
    pos = pos + vel
    pos = -1.2 if pos < -1.2 else (0.6 if pos > 0.6 else pos)
    if pos == -1.2 and vel < 0.0:
        vel = 0.0
    return pos, vel, (pos >= 0.5 and vel >= 0.0)


def bounds(p, k=RULE_COEFS):
    """(lb, ub) of the rule at position p, float64, powers as products."""
    a = p + k[1]
    l1 = k[0] * (a * a) + k[2]
    b = p + k[4]
    b2 = b * b
    l2 = k[3] * (b2 * b2) - k[5]
    lb = l1 if l1 < l2 else l2
    c = p + k[7]
    ub = k[6] * (c * c) + k[8]
    return lb, ub


def rule(k=RULE_COEFS):
    """The rule policy with constants k as a function of the float32 observation (p, v), both given as python floats."""
    k = tuple(float(x) for x in k)

    def act(p, v):
        lb, ub = bounds(p, k)
        return 2 if lb < v < ub else 0
    return act


def pump(p, v):
    return 0 if v <= 0 else 2


def pump_left(p, v):
    return 0 if v <= 0 else 1


POLICIES = {"rule": rule(), "pump": pump, "pump-left": pump_left}


def actions(obs, act):
    """act on every row of obs f32[N, 2] -> i32[N]: the host policy of the stepper tests."""
    return np.array([act(float(p), float(v)) for p, v in np.asarray(obs, np.float32)], np.int32)


def episode(pos, vel, act=POLICIES["rule"], cap=MAX_STEPS, cos=det_cos):
    """One episode from (pos, vel) -> dict(ret, len, reached, pos, vel, hit_wall, margin: the smallest distance of an observed
    velocity to lb / ub of the reference rule along the way)."""
    ret, steps, reached, hit_wall, margin = 0.0, 0, False, False, math.inf
    while steps < cap and not reached:
        p, v = f32(pos), f32(vel)
        lb, ub = bounds(p)
        margin = min(margin, abs(v - lb), abs(v - ub))
        pos, vel, reached = advance(pos, vel, act(p, v), cos)
        hit_wall = hit_wall or pos == -1.2
        ret, steps = ret + (-1.0), steps + 1
    return dict(ret=ret, len=steps, reached=reached, pos=pos, vel=vel, hit_wall=hit_wall, margin=margin)


def eval_population(seed, stream_id0, E, coefs=None, start=None, cap=MAX_STEPS):
    """gymrl_mountaincar_rule_eval -> (returns f64, lengths i32, reached u8, final_state f64[.., 2]), each [P, E]."""
    coefs = [RULE_COEFS] if coefs is None else np.atleast_2d(np.asarray(coefs, np.float64)).tolist()
    out = []
    for p, k in enumerate(coefs):
        row = []
        for e in range(E):
            i = p * E + e
            pos, vel = draw(seed, stream_id0 + i) if start is None else (float(start[p][e][0]), float(start[p][e][1]))
            row.append(episode(pos, vel, rule(k), cap))
        out.append(row)
    return (np.array([[o["ret"] for o in r] for r in out], np.float64), np.array([[o["len"] for o in r] for r in out], np.int32),
            np.array([[o["reached"] for o in r] for r in out], np.uint8),
            np.array([[(o["pos"], o["vel"]) for o in r] for r in out], np.float64))


def stepper_trace(seed, env_id, act, T, abandon_cap=0):
    """T vector steps of ONE env of the batched stepper under the host policy `act` (fed the observation the stepper returned),
    with auto-reset; abandon_cap > 0 also runs gymrl_env_abandon(cap) after every step.  -> dict of [T] arrays: obs / term_obs
    f32[T, 2], rew f32, terminated / truncated / done / abandoned u8, ep_ret_out f32 and ep_len_out i32 (0 where no episode
    ended at that step), action i32, and the state after the step: pos, vel, ep_ret f64, ep_len i32, episode u32; obs0 f32[2]."""
    pos, vel = draw(seed, env_id, 0)
    ep_ret, ep_len, ep = 0.0, 0, 0
    obs0 = (np.float32(pos), np.float32(vel))
    o = obs0
    rows = []
    for _ in range(T):
        a = act(float(o[0]), float(o[1]))
        pos, vel, terminated = advance(pos, vel, a)
        length, ret = ep_len + 1, ep_ret + (-1.0)
        truncated = length >= MAX_STEPS
        done = terminated or truncated
        term = (np.float32(pos), np.float32(vel))
        ret_out, len_out, abandoned = 0.0, 0, False
        if done:
            ep += 1
            pos, vel = draw(seed, env_id, ep)
            ep_ret, ep_len, ret_out, len_out = 0.0, 0, ret, length
            o = (np.float32(pos), np.float32(vel))
        else:
            ep_ret, ep_len, o = ret, length, term
        if abandon_cap and ep_len >= abandon_cap:
            ret_out, len_out, abandoned = ep_ret, ep_len, True
            ep += 1
            pos, vel = draw(seed, env_id, ep)
            ep_ret, ep_len = 0.0, 0
            o = (np.float32(pos), np.float32(vel))
        rows.append((o, term, -1.0, terminated, truncated, done, abandoned, ret_out, len_out, a, pos, vel, ep_ret, ep_len, ep))
    col = lambda j, dt: np.array([r[j] for r in rows], dt)   # noqa: E731
    return dict(obs0=np.array(obs0, np.float32), obs=col(0, np.float32), term_obs=col(1, np.float32), rew=col(2, np.float32),
                terminated=col(3, np.uint8), truncated=col(4, np.uint8), done=col(5, np.uint8), abandoned=col(6, np.uint8),
                ep_ret_out=col(7, np.float32), ep_len_out=col(8, np.int32), action=col(9, np.int32), pos=col(10, np.float64),
                vel=col(11, np.float64), ep_ret=col(12, np.float64), ep_len=col(13, np.int32), episode=col(14, np.uint32))


def stepper_traces(seed, env_id0, N, act, T, abandon_cap=0):
    """stepper_trace of envs env_id0 .. env_id0 + N - 1, stacked: every array becomes [T, N, ...] (obs0: [N, 2])."""
    traces = [stepper_trace(seed, env_id0 + i, act, T, abandon_cap) for i in range(N)]
    return {k: np.stack([t[k] for t in traces], axis=0 if k == "obs0" else 1) for k in traces[0]}
