"""The structured float32 input set of the reproducible-math sweep and the host twins it is held to (TEST INFRASTRUCTURE).

gymrl_device.hpp's det_expf / det_logf / det_tanhf / det_tanhf_sel / det_sincosf and gru_cell_device.hpp's det_sigmoidf promise
the bits of oracle/gymrl_oracle.c's orc_expf / orc_logf / orc_tanhf / orc_tanhf_sel / orc_sincosf.  This module builds, once and
with no randomness, the inputs at which a device build and a host build can part, and wraps the twins over arrays
(orc_map_f32: one C call per array).  Shared by tests/test_det_math_ref.py (CPU) and tests/test_det_math_gpu.py.  No torch.

    points()          ~2.4 million float32 bit patterns, sorted, unique (uint32 -> float32 view)
    sincos_points()   every float within 512 ulps of a multiple of pi/4 up to 8000, both signs (host sweep only: the device
                      reaches det_sincosf with RNG words alone)
    rows(x)           x padded with 0 to whole rows of H = 64 -> f32[B, 64]
"""
import functools

import numpy as np

F32 = np.float32
H = 64
WINDOW = 512                      # ulps on each side of a seam

# exhaustive maxima over all 2^32 inputs, printed by tools/check_det_f32.c (ulps of the correctly rounded float32 result of
# libm's double function; sincos over |x| < 8000, absolute).  DESIGN.md "The reproducible f32 math, swept" has the worst inputs.
MAX_ULP = {"exp": 1.0103, "log": 0.8265, "tanh": 1.3303, "sin": 687.9396, "cos": 687.9396}
MAX_ABS_SINCOS = 9.296e-08

EXP_LO, EXP_HI = F32(-87.33654), F32(88.72283)         # det_expf: x <= EXP_LO -> +0, x > EXP_HI -> +inf
TANH_SMALL, TANH_BIG = F32(0.625), F32(9.0)            # det_tanhf: polynomial below, +-1 above
LOG_SPLIT = F32(0.70710678)                            # det_logf's mantissa split
LOG2E = F32(1.44269504088896341)                       # det_expf's n = rintf(x * LOG2E)
TRAIN_SCALE = F32(2.885390081777927)                   # train_tanhf: exp2(x * TRAIN_SCALE)


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(F32)


def _ordered(u):
    """uint32 pattern -> an integer that ascends with the float's value (so +-k ulps is +-k, across zero too)."""
    u = np.asarray(u, np.int64)
    return np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)


def _unordered(k):
    k = np.asarray(k, np.int64)
    return np.where(k < 0, (-k) | 0x80000000, k).astype(np.uint32)


def window(center, ulps=WINDOW):
    """every float32 within `ulps` of center (a float32 value), clipped to the finite range and +-inf."""
    k = _ordered(bits(F32(center)).reshape(1))[0] + np.arange(-ulps, ulps + 1, dtype=np.int64)
    return _unordered(np.clip(k, -0x7F800000, 0x7F800000))


def train_tanh_overflow():
    """the smallest float32 x whose float32 product x * TRAIN_SCALE reaches 128, where the hardware exp2 returns +inf"""
    x = F32(128.0) / TRAIN_SCALE
    while F32(x * TRAIN_SCALE) >= F32(128.0):
        x = np.nextafter(x, F32(-np.inf), dtype=F32)
    while F32(x * TRAIN_SCALE) < F32(128.0):
        x = np.nextafter(x, F32(np.inf), dtype=F32)
    return x


def exp_ties():
    """for k = -127..128 the float32 x whose x * log2(e) is nearest k + 1/2: where rintf decides det_expf's n"""
    k = np.arange(-127, 129, dtype=np.float64)
    return ((k + 0.5) / 1.44269504088896340736).astype(F32)


@functools.lru_cache(maxsize=None)
def _points_bits():
    mant = np.concatenate([np.array([0, 1, 2, 0x7FFFFF, 0x7FFFFE], np.uint32),
                           (np.arange(4096, dtype=np.uint32) * np.uint32(2048) + np.uint32(0x2A5))])   # a fixed stride: 4096 more
    expo = np.arange(256, dtype=np.uint32) << np.uint32(23)
    grid = (expo[:, None] | mant[None, :]).ravel()
    parts = [grid, grid | np.uint32(0x80000000)]
    seams = [TANH_SMALL, -TANH_SMALL, TANH_BIG, -TANH_BIG, EXP_LO, EXP_HI, np.finfo(F32).tiny, -np.finfo(F32).tiny,
             np.finfo(F32).max, F32(1.0), F32(-1.0), LOG_SPLIT, train_tanh_overflow(), -train_tanh_overflow()]
    parts += [window(c) for c in seams]
    parts += [window(c) for c in exp_ties()]
    u = np.unique(np.concatenate(parts))
    u.setflags(write=False)
    return u


def points():
    """the structured set as float32 (read-only; NaNs with several payloads, +-0, +-inf and every denormal exponent included)"""
    return _points_bits().view(F32)


@functools.lru_cache(maxsize=None)
def _sincos_bits():
    m = np.arange(0, int(8000.0 / (np.pi / 4)) + 1, dtype=np.float64) * (np.pi / 4)
    c = _ordered(bits(m.astype(F32)))
    k = (c[:, None] + np.arange(-WINDOW, WINDOW + 1, dtype=np.int64)[None, :]).ravel()
    u = _unordered(k)
    u = np.unique(np.concatenate([u, u ^ np.uint32(0x80000000)]))
    x = u.view(F32)
    u = u[np.abs(x) < F32(8000.0)]
    u.setflags(write=False)
    return u


def sincos_points():
    return _sincos_bits().view(F32)


def rows(x, fill=0.0):
    """x f32[n] -> f32[ceil(n / 64), 64], the tail padded with `fill`"""
    x = np.asarray(x, F32).ravel()
    B = -(-x.size // H)
    out = np.full(B * H, fill, F32)
    out[:x.size] = x
    return out.reshape(B, H)


# ------------------------------------------------------------------ twins ----
def _orc():
    from oracle import oracle
    return oracle


def expf(x):
    """orc_expf = the bits of det_expf"""
    return _orc().map_f32(_orc().MAP_EXP, x)


def logf(x):
    """orc_logf = the bits of det_logf (finite x > 0)"""
    return _orc().map_f32(_orc().MAP_LOG, x)


def tanhf(x):
    """orc_tanhf = the bits of det_tanhf, the branchy form"""
    return _orc().map_f32(_orc().MAP_TANH, x)


def tanhf_sel(x):
    """orc_tanhf_sel = the bits of det_tanhf_sel, the select form"""
    return _orc().map_f32(_orc().MAP_TANH_SEL, x)


def sigmoidf(x):
    """det_sigmoidf: 1.0f / (1.0f + det_expf(-x))"""
    return _orc().map_f32(_orc().MAP_SIGMOID, x)


def sincosf(x):
    """orc_sincosf = the bits of det_sincosf -> (sin, cos)"""
    return _orc().map_f32(_orc().MAP_SINCOS, x)


def per_priority(td, alpha, eps):
    """per.hip's td_priority without the clip: exp((float)alpha * log(|td| + (float)eps)), float32 throughout"""
    e = np.abs(np.asarray(td, F32)) + F32(eps)
    return expf(F32(alpha) * logf(e))


def same_bits(got, want):
    """elementwise: equal as uint32, or both NaN"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def mismatch_report(name, x, got, want, limit=10):
    """'' when got and want carry the same bits (NaN = NaN), else the first `limit` offending inputs in hex with both results"""
    x, got, want = (np.asarray(a, F32).ravel() for a in (x, got, want))
    bad = np.flatnonzero(~same_bits(got, want))
    if bad.size == 0:
        return ""
    lines = [f"{name}: {bad.size} of {x.size} inputs differ; first {min(limit, bad.size)}:"]
    for i in bad[:limit]:
        lines.append(f"  x = 0x{bits(x[i:i + 1])[0]:08x} ({float(x[i])!r})  got 0x{bits(got[i:i + 1])[0]:08x} ({float(got[i])!r})"
                     f"  want 0x{bits(want[i:i + 1])[0]:08x} ({float(want[i])!r})")
    return "\n".join(lines)


# ------------------------------------------- the cells' exactness identities ----
# Each builds the inputs of a cell kernel around x [B, 64] so that every operation around the function under test is exact
# (the comments say why); the GPU tests hand them to the kernels, the CPU tests to the restatements.
NEG0 = F32(-0.0)


def gru_sigmoid_inputs(x):
    """gymrl_gru_cell_fwd -> h' = det_sigmoidf(x).  gi = (0, x, 0), gh = 0, h = 1:  z = s(x + 0) = s(x) (x + 0 is x but for
    -0 -> +0, and s(+-0) = 1 / (1 + 1) either way);  r = s(0) = 1/2,  n = tanh(0 + r * 0) = 0;
    h' = (1 - z) * 0 + z * 1 = (+0) + z = z for every z in [0, 1] (1 - z >= 0, so the product is +0) and NaN for NaN."""
    B = x.shape[0]
    gi = np.zeros((B, 3 * H), F32)
    gi[:, H:2 * H] = x
    return gi, np.zeros((B, 3 * H), F32), np.ones((B, H), F32)


def gru_tanh_inputs(x):
    """gymrl_gru_cell_fwd -> h' = det_tanhf_sel(x).  gi = (0, -200, x), gh = (0, 0, -0), h = -1:  exp(200) = +inf so
    z = 1 / (1 + inf) = +0;  r = 1/2 and r * (-0) = -0, x + (-0) = x for EVERY x (-0 included), n = tanh_sel(x);
    h' = (1 - 0) * n + 0 * (-1) = n + (-0) = n, the sign of a zero kept."""
    B = x.shape[0]
    gi = np.zeros((B, 3 * H), F32)
    gi[:, H:2 * H] = -200.0
    gi[:, 2 * H:] = x
    gh = np.zeros((B, 3 * H), F32)
    gh[:, 2 * H:] = NEG0
    return gi, gh, np.full((B, H), -1.0, F32)


def lstm_tanh_inputs(x):
    """gymrl_lstm_cell_fwd -> c' = det_tanhf_sel(x), h' = det_tanhf_sel(c').  gi = (200, -200, x, 200), gh = (0, 0, -0, 0),
    c = -1:  i = o = 1 / (1 + exp(-200)) = 1 / (1 + 0) = 1,  f = 1 / (1 + inf) = +0,  g = tanh_sel(x + (-0)) = tanh_sel(x);
    c' = (0 * -1) + (1 * g) = (-0) + g = g;  h' = 1 * tanh_sel(c')."""
    B = x.shape[0]
    gi = np.empty((B, 4 * H), F32)
    gi[:, :H], gi[:, H:2 * H], gi[:, 2 * H:3 * H], gi[:, 3 * H:] = 200.0, -200.0, x, 200.0
    gh = np.zeros((B, 4 * H), F32)
    gh[:, 2 * H:3 * H] = NEG0
    return gi, gh, np.full((B, H), -1.0, F32)


def sac_tanh_inputs(x):
    """gymrl_sac_sample_fwd(mean, log_std, eps, bound = 1) -> action = det_tanhf(x), the branchy form.  mean = x, log_std = 0,
    eps = -0:  std = exp(0) = 1,  1 * (-0) = -0,  mean + (-0) = mean for EVERY mean (-0, +-inf and NaN included);
    action = t * 1 = t, the sign of a zero kept."""
    return x, np.zeros_like(x), np.full_like(x, NEG0)


def gru_cell_fwd(gi, gh, h):
    """gru_point_fwd in numpy float32 on the twins (the oracle's orc_gru_cell_fwd states the same lines in C)"""
    gi, gh, h = (np.asarray(a, F32) for a in (gi, gh, h))
    n_h = h.shape[-1]
    r = sigmoidf(gi[:, :n_h] + gh[:, :n_h])
    z = sigmoidf(gi[:, n_h:2 * n_h] + gh[:, n_h:2 * n_h])
    n = tanhf_sel(gi[:, 2 * n_h:] + r * gh[:, 2 * n_h:])
    return (F32(1.0) - z) * n + z * h, (r, z, n)


# ------------------------------------------------------ saturated consumers ----
def _gates_at_inf(g, n_gates, n_h):
    """row 1: gate block k gets +inf in column k and -inf in column k + n_gates"""
    for k in range(n_gates):
        g[1, k * n_h + k] = np.inf
        g[1, k * n_h + k + n_gates] = -np.inf


def saturated_gru_case(B, n_h, scale=60.0):
    """tests/test_recurrent_gpu.py's cell inputs (N(0, 1) * 2) times `scale`: gates far beyond +-200; row 1 has gates at +-inf"""
    rng = np.random.default_rng(21)
    gi = ((rng.normal(size=(B, 3 * n_h)) * 2).astype(F32) * F32(scale)).astype(F32)
    gh = ((rng.normal(size=(B, 3 * n_h)) * 2).astype(F32) * F32(scale)).astype(F32)
    h, dh = rng.normal(size=(B, n_h)).astype(F32), rng.normal(size=(B, n_h)).astype(F32)
    gh[1] = 0.0
    _gates_at_inf(gi, 3, n_h)
    return gi, gh, h, dh


def saturated_lstm_case(B, n_h, scale=60.0):
    """tests/test_lstm_cell_gpu.py's _case pre-activations times `scale`; row 1 (B > 1) has gates at +-inf"""
    rng = np.random.default_rng(100 * B + n_h)
    gi, gh = (((rng.normal(size=(B, 4 * n_h)) * 2).astype(F32) * F32(scale)).astype(F32) for _ in range(2))
    c, dh, dc = (rng.normal(size=(B, n_h)).astype(F32) for _ in range(3))
    gh[1] = 0.0
    _gates_at_inf(gi, 4, n_h)
    return gi, gh, c, dh, dc


SOFTMAX_GAPS = (F32(87.0), F32(87.3365), F32(87.3366), F32(88.0), F32(200.0))


def softmax_case(A, B=257):
    """-> (z f32[B, A], top i[B], low i[B], gap f32[B]).  Row b < B - 1: the maximum m (0 on even rows, 64 on odd ones) at
    column top[b], one logit exactly gap[b] below it at column low[b] (m - gap and (m - gap) - m are exact in float32: 64 and
    every gap share a binade grid finer than the result's), the others within 3 below m.  Row B - 1: every logit 3e38."""
    rng = np.random.default_rng(7 * A)
    b = np.arange(B)
    top, low = b % A, (b + 1) % A
    gap = np.array(SOFTMAX_GAPS, F32)[b % len(SOFTMAX_GAPS)]
    m = np.where(b % 2 == 0, F32(0.0), F32(64.0)).astype(F32)
    z = (m[:, None] - (F32(3.0) * rng.random((B, A)).astype(F32))).astype(F32)
    z[b, top] = m
    z[b, low] = m - gap
    z[B - 1] = F32(3e38)
    return z, top, low, gap


def softmax_fwd(z):
    """softmax_row_fwd: m = max, e_k = det_expf(z_k - m), s = e_0 + e_1 + ... in ascending k, p_k = e_k / s (float32)"""
    z = np.asarray(z, F32)
    e = expf(z - z.max(axis=1, keepdims=True))
    s = np.zeros(z.shape[0], F32)
    for k in range(z.shape[1]):
        s = s + e[:, k]
    return e / s[:, None]


def softmax_bwd(p, g):
    """softmax_row_bwd: dot = sum_k g_k * p_k in ascending k, dz_k = p_k * (g_k - dot) (float32, no fused operation)"""
    p, g = np.asarray(p, F32), np.asarray(g, F32)
    dot = np.zeros(p.shape[0], F32)
    for k in range(p.shape[1]):
        dot = dot + g[:, k] * p[:, k]
    return p * (g - dot[:, None])
