"""The categorical (C51) head restated twice (TEST INFRASTRUCTURE).  No torch.

  * c51_q / c51_loss: csrc/c51_device.hpp + csrc/c51.hip in numpy float32, operation for operation and sum for sum (numpy's
    float32 +, -, *, / are the IEEE operations the kernels run under -ffp-contract=off; exp / log are the oracle's twins of
    det_expf / det_logf through tests/det_math_ref.py).  The GPU tests compare bits against these.
  * textbook_q / textbook_loss: the algorithm as the paper states it, in float64: softmax, the floor / ceil SCATTER of the
    projection with the l == u fix (an atom hit exactly keeps its mass), log_softmax.  tests/test_c51_ref.py bounds the float32
    restatement against it.
"""
import types

import numpy as np

import det_math_ref as dm

F32 = np.float32
WAVE = 64
ROWS_PER_BLOCK = 4                 # c51.hip: one wave per row, 256 threads
MAX_BLOCKS = 4096                  # ... and its grid cap: batches past ROWS_PER_BLOCK * MAX_BLOCKS rows wrap the grid-stride loop


def support(M, vmin, vmax):
    """-> (z f32[M], dz): z_j = vmin + (float)j * dz, dz = (vmax - vmin) / (float)(M - 1)"""
    vmin, vmax = F32(vmin), F32(vmax)
    dz = F32(F32(vmax - vmin) / F32(M - 1))
    return (vmin + np.arange(M, dtype=F32) * dz).astype(F32), dz


def tree_sum(v):
    """wave_allsum over the last axis: 64 slots (slots >= M hold +0), v[0:off] + v[off:2 off] for off = 32 ... 1"""
    v = np.asarray(v, F32)
    s = np.zeros(v.shape[:-1] + (WAVE,), F32)
    s[..., :v.shape[-1]] = v
    off = WAVE // 2
    while off:
        s = s[..., :off] + s[..., off:2 * off]
        off //= 2
    return s[..., 0]


def softmax_parts(x):
    """softmax_lane over the last axis -> (d = x - max, e = expf(d), s = tree_sum(e))"""
    x = np.asarray(x, F32)
    d = x - x.max(axis=-1, keepdims=True)
    e = dm.expf(d)
    return d, e, tree_sum(e)


def c51_q(logits, vmin, vmax):
    """gymrl_c51_q: logits f32[B, A, M] -> (q f32[B, A], first-maximum action i32[B])"""
    logits = np.asarray(logits, F32)
    z, _ = support(logits.shape[-1], vmin, vmax)
    _, e, s = softmax_parts(logits)
    q = tree_sum((e / s[..., None]) * z)
    return q, np.argmax(q, axis=1).astype(np.int32)


def c51_loss(logits, next_target, act, rew, flag, gamma_n, vmin, vmax, next_online=None, w=None):
    """gymrl_c51_loss -> namespace(row_loss f32[B], dlogits f32[B, A, M], terms f32[B] = row_loss * w (what the float64 loss sum
    adds up), astar i32[B], m f32[B, M])"""
    logits, next_target = np.asarray(logits, F32), np.asarray(next_target, F32)
    B, A, M = logits.shape
    act, rew, flag = np.asarray(act), np.asarray(rew, F32), np.asarray(flag, F32)
    z, dz = support(M, vmin, vmax)
    vmin, vmax = F32(vmin), F32(vmax)
    rows = np.arange(B)
    _, astar = c51_q(next_target if next_online is None else next_online, vmin, vmax)
    _, e, s = softmax_parts(next_target[rows, astar])
    pstar = e / s[:, None]
    g = F32(gamma_n) * (F32(1.0) - flag)
    tz = np.minimum(np.maximum(rew[:, None] + g[:, None] * z[None, :], vmin), vmax)
    pos = (tz - vmin) / dz
    lane = np.arange(M, dtype=F32)[None, :]
    m = np.zeros((B, M), F32)
    for j in range(M):                                                    # j ascending, from +0
        m = m + pstar[:, j:j + 1] * np.maximum(F32(0.0), F32(1.0) - np.abs(pos[:, j:j + 1] - lane))
    valid = (act >= 0) & (act < A)
    d, e, s = softmax_parts(logits[rows, np.where(valid, act, 0)])
    logp = d - dm.logf(s)[:, None]
    row_loss = np.where(valid, -tree_sum(m * logp), F32(np.nan)).astype(F32)
    wb = np.ones(B, F32) if w is None else np.asarray(w, F32)
    grad = (wb * (F32(1.0) / F32(B)))[:, None] * (e / s[:, None] - m)
    dlogits = np.zeros((B, A, M), F32)
    dlogits[rows[valid], act[valid]] = grad[valid]
    return types.SimpleNamespace(row_loss=row_loss, dlogits=dlogits, terms=(row_loss * wb).astype(F32), astar=astar, m=m)


# ------------------------------------------------------------------ the float64 textbook ----
def _softmax64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def textbook_q(logits, vmin, vmax):
    logits = np.asarray(logits, np.float64)
    z = np.linspace(float(vmin), float(vmax), logits.shape[-1])
    q = (_softmax64(logits) * z).sum(axis=-1)
    return q, np.argmax(q, axis=1).astype(np.int32)


def textbook_project(pstar, rew, flag, gamma_n, M, vmin, vmax):
    """Bellemare et al. 2017, Algorithm 1: m_l += p (u - b), m_u += p (b - l) with l = floor(b), u = ceil(b) — and, where
    l == u (both weights 0 as written), the whole p on that atom."""
    pstar, rew, flag = (np.asarray(a, np.float64) for a in (pstar, rew, flag))
    B = pstar.shape[0]
    vmin, vmax = float(vmin), float(vmax)
    z = np.linspace(vmin, vmax, M)
    dz = (vmax - vmin) / (M - 1)
    tz = np.clip(rew[:, None] + gamma_n * (1.0 - flag)[:, None] * z[None, :], vmin, vmax)
    b = np.clip((tz - vmin) / dz, 0.0, M - 1.0)
    lo, up = np.floor(b).astype(np.int64), np.ceil(b).astype(np.int64)
    m = np.zeros((B, M))
    r = np.repeat(np.arange(B), M)
    np.add.at(m, (r, lo.ravel()), (pstar * np.where(lo == up, 1.0, up - b)).ravel())
    np.add.at(m, (r, up.ravel()), (pstar * (b - lo)).ravel())
    return m


def textbook_loss(logits, next_target, act, rew, flag, gamma_n, vmin, vmax, next_online=None, w=None):
    """-> namespace(row_loss f64[B], dlogits f64[B, A, M] of mean_b(w_b row_loss_b), astar, m f64[B, M], logp f64[B, M])"""
    logits, next_target = np.asarray(logits, np.float64), np.asarray(next_target, np.float64)
    B, A, M = logits.shape
    act = np.asarray(act)
    rows = np.arange(B)
    _, astar = textbook_q(next_target if next_online is None else next_online, vmin, vmax)
    m = textbook_project(_softmax64(next_target[rows, astar]), rew, flag, float(gamma_n), M, vmin, vmax)
    x = logits[rows, act]
    sh = x - x.max(axis=1, keepdims=True)
    logp = sh - np.log(np.exp(sh).sum(axis=1, keepdims=True))
    wb = np.ones(B) if w is None else np.asarray(w, np.float64)
    dlogits = np.zeros((B, A, M))
    dlogits[rows, act] = (wb / B)[:, None] * (np.exp(logp) - m)
    return types.SimpleNamespace(row_loss=-(m * logp).sum(axis=1), dlogits=dlogits, astar=astar, m=m, logp=logp)


# ------------------------------------------------------------------ the shared cases ----
def case(B, A, M, vmin=0.0, vmax=100.0, seed=0):
    """One batch that walks the head's edges; rows cycle through the row kinds below, so every B >= 1 gets the first B of them.
    -> dict(logits, next_target, next_online f32[B, A, M]; act i32[B]; rew, flag, w f32[B]; gamma_n; vmin; vmax)."""
    rng = np.random.default_rng(1000 * B + 10 * A + M + seed)
    z, dz = support(M, vmin, vmax)
    logits, nt, no = ((2.0 * rng.normal(size=(B, A, M))).astype(F32) for _ in range(3))
    act = rng.integers(0, A, size=B).astype(np.int32)
    rew = (float(dz) * rng.uniform(-2.0, 3.0, size=B)).astype(F32)
    flag = (rng.random(B) < 0.25).astype(F32)
    w = rng.uniform(0.1, 2.0, size=B).astype(F32)
    mid = M // 2
    for b in range(B):
        k = b % 16
        if k == 1:                          # equal logits across the actions: every expected value ties, a* = 0
            nt[b], no[b] = nt[b, 0], no[b, 0]
        elif k == 2:                        # the two nets disagree on a*: each piles its mass at opposite ends for action 0 / A-1
            no[b], nt[b] = 0.0, 0.0
            no[b, 0, M - 1], nt[b, A - 1, M - 1] = 30.0, 30.0
            no[b, A - 1, 0], nt[b, 0, 0] = 30.0, 30.0
        elif k == 3:                        # a saturated softmax, both signs
            logits[b, act[b], mid], nt[b, :, 0] = 80.0, -80.0
        elif k == 4:
            logits[b, act[b], 0], nt[b, :, M - 1] = -80.0, 80.0
        elif k == 5:                        # rewards that clamp all the mass onto vmax / vmin
            rew[b], flag[b] = F32(vmax) + F32(1000.0), 0.0
        elif k == 6:
            rew[b], flag[b] = F32(vmin) - F32(1000.0), 0.0
        elif k == 7:                        # terminal rows: the reward exactly on an atom, on vmin, on vmax, between two atoms
            rew[b], flag[b] = z[mid], 1.0
        elif k == 8:
            rew[b], flag[b] = F32(vmin), 1.0
        elif k == 9:
            rew[b], flag[b] = F32(vmax), 1.0
        elif k == 10:
            rew[b], flag[b] = z[mid] + F32(0.25) * dz, 1.0
        elif k == 11:                       # a zero weight
            w[b] = 0.0
    return dict(logits=logits, next_target=nt, next_online=no, act=act, rew=rew, flag=flag, w=w, gamma_n=0.99 ** 3, vmin=vmin, vmax=vmax)
