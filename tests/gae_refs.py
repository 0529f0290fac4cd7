"""Definitional references and input builders shared by tests/test_gae_edges.py (CPU) and tests/test_gae_edges_gpu.py.

The references are the textbook backward recursion, written from the formula and not from any kernel's operation order,
in numpy.longdouble:

    delta_t = r_t + gamma * V_{t+1} * (1 - d_t) - V_t          (V_T = the bootstrap value)
    A_t     = delta_t + decay * (1 - d_t) * A_{t+1}            (A_T = 0)
    ret_t   = A_t + V_t

`decay` is an argument, so that each kernel's documented rounding of gamma * lambda is stated once, here:
G1 (gymrl_gae) uses float32(gamma * lam), G3 (gymrl_gae_decoupled) the plain double products, G2 (gymrl_gae_dw) float32
gamma and float32(gamma * lam) in a float32 recursion (restated below in float32 too, in the order of utils/buffer.py:23,28).

Everything a builder returns is cached and read-only: one reference per case, shared and left unchanged."""
import functools

import numpy as np

LD = np.longdouble

G1 = (0.99, 0.95)                       # gamma, lambda of the G1 / G2 cases (the values of tests/test_hip_parity.py)
G3 = (0.995, 0.9, 0.97)                 # gamma, lambda_actor, lambda_critic

CARRY_T = (2047, 2048, 2049, 2064, 2177, 4096, 4100)     # 128 chunks of 16 steps = one carry round
CARRY_N = (4, 68)                                        # 68: two carry workgroups, 4 live lanes in the second
STRUCT_T, STRUCT_N = 2049 + 16, 8                        # 130 chunks, the last one of length 1
DW_T, DW_N = (1, 15, 16, 17, 33), (1, 63, 65)


def g1_decay(gamma, lam):
    return float(np.float32(gamma * lam))


def gae_inputs(T, N, seed, p_done=0.03):
    """_gae_inputs of tests/test_hip_parity.py: unit-normal rewards with 1 % spikes of 100x, coin-flip episode ends."""
    rng = np.random.default_rng(seed)
    rew = (rng.normal(size=(T, N)) * np.where(rng.random((T, N)) < 0.01, 100.0, 1.0)).astype(np.float32)
    val = rng.normal(size=(T, N)).astype(np.float32)
    done = (rng.random((T, N)) < p_done).astype(np.uint8)
    nv = rng.normal(size=N).astype(np.float32)
    return rew, val, done, nv


def gae_ref(rew, val, done, next_val, gamma, decay):
    """(A, ret) in longdouble, [T][N]."""
    T, N = rew.shape
    r, v = rew.astype(LD), val.astype(LD)
    live = LD(1) - (done != 0).astype(LD)
    gamma, decay = LD(gamma), LD(decay)
    adv = np.empty((T, N), LD)
    a_next, v_next = np.zeros(N, LD), next_val.astype(LD)
    for t in range(T - 1, -1, -1):
        delta = r[t] + gamma * v_next * live[t] - v[t]
        a_next = delta + decay * live[t] * a_next
        adv[t] = a_next
        v_next = v[t]
    return adv, adv + v


def gae_decoupled_ref(rew, val, done, next_val, gamma, lam_actor, lam_critic):
    """(A under lambda_actor, ret under lambda_critic): ppo_full_lunarlander.py:507-535."""
    adv, _ = gae_ref(rew, val, done, next_val, gamma, gamma * lam_actor)
    _, ret = gae_ref(rew, val, done, next_val, gamma, gamma * lam_critic)
    return adv, ret


def gae_dw_ref(rew, val, next_val, done, dw, gamma, lam, dtype=LD):
    """G2 (utils/buffer.py:21-35): delta masks the bootstrap with dw, the recursion is cut by done; next_val is a [T][N]
    slab.  Both flags enter independently.  dtype = numpy.float32 gives the float32 recursion in the reference program's
    order, `gamma * next_values * (1 - dw)` and `gamma * lamda * gae * (1 - d)` from left to right; dtype = longdouble the
    same formula without intermediate rounding, on the same float32-rounded constants.  Returns (A, A + V)."""
    T, N = rew.shape
    f = dtype
    r, v, nv = rew.astype(f), val.astype(f), next_val.astype(f)
    keep, live = f(1) - (dw != 0).astype(f), f(1) - (done != 0).astype(f)
    g, gl = f(np.float32(gamma)), f(np.float32(gamma * lam))
    adv = np.empty((T, N), f)
    a_next = np.zeros(N, f)
    for t in range(T - 1, -1, -1):
        delta = r[t] + g * nv[t] * keep[t] - v[t]
        a_next = gl * a_next * live[t] + delta
        adv[t] = a_next
    return adv, adv + v


def sums(adv):
    """(sum A, sum A^2) in longdouble: what the kernels' moments_out[1:] accumulate."""
    a = np.asarray(adv, LD)
    return np.array([a.sum(), (a * a).sum()], LD)


def structured_done(T):
    """[T][8] uint8, one pattern per env column; column 7 carries column 0's pattern with the byte 255 instead of 1."""
    t = np.arange(T)
    d = np.zeros((T, 8), np.uint8)
    d[t % 16 == 15, 0] = 1              # the last step of every chunk
    d[t % 16 == 0, 1] = 1               # the first step of every chunk
    d[T - 1, 2] = 1                     # only the last step: the bootstrap value must be ignored
    d[0, 3] = 1                         # only the first step
    d[:, 4] = 1                         # every step: A == delta == r - V
    #      5                              no step: A is a product of T decay factors
    if T > 2048:
        d[2047:2049, 6] = 1             # the two sides of chunk boundary 128
    d[:, 7] = d[:, 0] * 255
    return d


def _freeze(case):
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def carry_case(T, N):
    rew, val, done, nv = gae_inputs(T, N, seed=31 * T + N)
    return _freeze(_with_refs(rew, val, done, nv))


@functools.lru_cache(maxsize=None)
def structured_case(T=STRUCT_T):
    rew, val, _, nv = gae_inputs(T, STRUCT_N, seed=17 * T)
    rew[:, 7], val[:, 7], nv[7] = rew[:, 0], val[:, 0], nv[0]            # column 7 = column 0 but for the done byte
    return _freeze(_with_refs(rew, val, structured_done(T), nv))


def _with_refs(rew, val, done, nv):
    a1, r1 = gae_ref(rew, val, done, nv, G1[0], g1_decay(*G1))
    a3, r3 = gae_decoupled_ref(rew, val, done, nv, *G3)
    return dict(rew=rew, val=val, done=done, nv=nv, g1_adv=a1, g1_ret=r1, g1_sums=sums(a1), g3_adv=a3, g3_ret=r3)


@functools.lru_cache(maxsize=None)
def dw_case(T, N):
    """done and dw drawn independently (so dw = 1 with done = 0 occurs wherever T * N allows), the first min(N, 8) env
    columns with the structured done patterns instead."""
    rng = np.random.default_rng(1000 * T + N)
    rew, val, nval = (rng.normal(size=(T, N)).astype(np.float32) for _ in range(3))
    done = (rng.random((T, N)) < 0.15).astype(np.uint8)
    dw = (rng.random((T, N)) < 0.15).astype(np.uint8)
    k = min(N, 8)
    done[:, :k] = structured_done(T)[:, :k]
    if T * N >= 15:
        dw.flat[(T * N) // 2], done.flat[(T * N) // 2] = 1, 0            # pinned: dw without done ...
        dw.flat[(T * N) // 3], done.flat[(T * N) // 3] = 0, 1            # ... and done without dw
    a32, v32 = gae_dw_ref(rew, val, nval, done, dw, *G1, dtype=np.float32)
    ald, vld = gae_dw_ref(rew, val, nval, done, dw, *G1)
    return _freeze(dict(rew=rew, val=val, nval=nval, done=done, dw=dw, adv32=a32, vt32=v32, adv=ald, vt=vld,
                        sums=sums(a32.astype(np.float64))))


# ------------------------------------------------------------------ moments / normalise ---
def two_pass(x, ddof):
    """(mean, variance) of the float32 vector x, two passes in longdouble."""
    x = np.asarray(x, np.float32).astype(LD)
    mean = x.sum() / LD(x.size)
    dev = x - mean
    return mean, (dev * dev).sum() / LD(x.size - ddof)


def normalize_ref(x, ddof, eps=1e-8):
    """(x - mean) / (std + eps) in longdouble: ppo_lunarlander.py:236 (ddof 0), utils/buffer.py:33 (ddof 1)."""
    mean, var = two_pass(x, ddof)
    return (np.asarray(x, np.float32).astype(LD) - mean) / (np.sqrt(var) + LD(eps))


def moments_ref(x):
    x = np.asarray(x, np.float32).astype(LD)
    return np.array([LD(x.size), x.sum(), (x * x).sum()], LD)


MOMENTS_CLAMP = 2048 * 256 * 16         # gymrl_moments: one workgroup per 256 * 16 elements, at most 2048 workgroups
NORMALIZE_CLAMP = 2048 * 256 * 8        # gymrl_normalize: 256 * 8 elements per workgroup

# name -> (n, ddof values); the constant vectors leave out (n = 1, ddof = 1): see test_gae_edges_gpu.py
NORM_CASES = {"const_1": (1, (0,)), "const_5": (5, (0, 1)), "const_4099": (4099, (0, 1)), "negconst_4099": (4099, (0, 1)),
              "pair": (2, (1,)), "large_mean": (100003, (0, 1)),
              "below_normalize_clamp": (NORMALIZE_CLAMP - 3, (0,)), "above_normalize_clamp": (NORMALIZE_CLAMP + 5, (1,)),
              "below_moments_clamp": (MOMENTS_CLAMP - 3, ()), "above_moments_clamp": (MOMENTS_CLAMP + 5, ())}
NORM_SMALL = tuple(k for k, (n, _) in NORM_CASES.items() if n <= 100003)


@functools.lru_cache(maxsize=None)
def norm_input(name):
    n = NORM_CASES[name][0]
    rng = np.random.default_rng(n)
    if name.startswith("const"):
        x = np.full(n, 0.1, np.float32)
    elif name.startswith("negconst"):
        x = np.full(n, -1234.5678, np.float32)
    elif name == "large_mean":
        x = (1e4 + rng.normal(size=n)).astype(np.float32)              # spread / mean = 1e-4: sum x^2 - n mean^2 cancels
    else:
        x = (rng.normal(size=n) * 3 + 0.5).astype(np.float32)          # the distribution of test_moments_normalize
    x.setflags(write=False)
    return x
