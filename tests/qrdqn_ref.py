"""The quantile-regression (QR-DQN) head restated twice (TEST INFRASTRUCTURE).  No torch.

  * qr_q / qr_loss: csrc/qrdqn_device.hpp + csrc/qrdqn.hip in numpy float32, operation for operation and sum for sum (numpy's
    float32 +, -, *, / are the IEEE operations the kernels run under -ffp-contract=off; the head has no exp or log, so nothing
    else is needed).  The GPU tests compare bits against these.
  * textbook_q / textbook_loss: the loss as Dabney et al. 2018 state it, in float64 and as one [B, N, N] broadcast.
    tests/test_qrdqn_ref.py bounds the float32 restatement against it.
"""
import types

import numpy as np

from c51_ref import tree_sum        # the 64-slot halving tree of row_loss_device.hpp's wave_allsum

F32 = np.float32
ROWS_PER_BLOCK = 4                 # qrdqn.hip: one wave per row, 256 threads
MAX_BLOCKS = 4096                  # ... and its grid cap: batches past ROWS_PER_BLOCK * MAX_BLOCKS rows wrap the grid-stride loop


def qr_q(quant):
    """gymrl_qr_q: quant f32[B, A, N] -> (q f32[B, A] = tree_sum / (float)N, first-maximum action i32[B])"""
    quant = np.asarray(quant, F32)
    B, A, N = quant.shape
    q = (tree_sum(quant) / F32(N)).astype(F32)
    arg, best = np.zeros(B, np.int32), q[:, 0].copy()
    for a in range(1, A):                                                 # greedy_action: `q > best`, so a NaN never wins
        better = q[:, a] > best
        arg[better], best = a, np.where(better, q[:, a], best)
    return q, arg


def qr_loss(quant, next_target, act, rew, flag, gamma_n, kappa=1.0, next_online=None, w=None):
    """gymrl_qr_loss -> namespace(row_loss f32[B], dquant f32[B, A, N], terms f32[B] = row_loss * w (what the float64 loss sum
    adds up), astar i32[B])"""
    quant, next_target = np.asarray(quant, F32), np.asarray(next_target, F32)
    B, A, N = quant.shape
    act, rew, flag = np.asarray(act), np.asarray(rew, F32), np.asarray(flag, F32)
    kappa = F32(kappa)
    rows = np.arange(B)
    _, astar = qr_q(next_target if next_online is None else next_online)
    valid = (act >= 0) & (act < A)
    tau = (2 * np.arange(N) + 1).astype(F32) / F32(2 * N)
    below, half_kappa = F32(1.0) - tau, F32(0.5) * kappa
    with np.errstate(over="ignore", invalid="ignore"):                    # (0.5 u) u overflows in the branch that is not taken
        g = F32(gamma_n) * (F32(1.0) - flag)
        T = rew[:, None] + g[:, None] * next_target[rows, astar]
        theta = quant[rows, np.where(valid, act, 0)]
        l, gs = np.zeros((B, N), F32), np.zeros((B, N), F32)
        for j in range(N):                                                # pair_sums: j ascending, from +0
            u = T[:, j:j + 1] - theta
            au = np.abs(u)
            wt = np.where(u < 0, below, tau)
            H = np.where(au <= kappa, (F32(0.5) * u) * u, kappa * (au - half_kappa))
            c = np.where(u > kappa, kappa, np.where(u < -kappa, -kappa, u))
            l = l + wt * H
            gs = gs + wt * c
        row_loss = np.where(valid, tree_sum((l / kappa) / F32(N)), F32(np.nan)).astype(F32)
        wb = np.ones(B, F32) if w is None else np.asarray(w, F32)
        grad = (wb * (F32(1.0) / F32(B)))[:, None] * -((gs / kappa) / F32(N))
        terms = (row_loss * wb).astype(F32)
    dquant = np.zeros((B, A, N), F32)
    dquant[rows[valid], act[valid]] = grad[valid]
    return types.SimpleNamespace(row_loss=row_loss, dquant=dquant, terms=terms, astar=astar)


# ------------------------------------------------------------------ the float64 textbook ----
def textbook_q(quant):
    q = np.asarray(quant, np.float64).mean(axis=-1)
    return q, np.argmax(q, axis=1).astype(np.int32)


def textbook_loss(quant, next_target, act, rew, flag, gamma_n, kappa=1.0, next_online=None, w=None):
    """-> namespace(row_loss f64[B], dquant f64[B, A, N] of mean_b(w_b row_loss_b), astar, u f64[B, N, N] (u[b, i, j] = T_j -
    theta_i), T f64[B, N], theta f64[B, N], gnt f64[B, N] = gamma_n (1 - flag) next_target[b, a*])"""
    quant, next_target = np.asarray(quant, np.float64), np.asarray(next_target, np.float64)
    B, A, N = quant.shape
    act, rew, flag = np.asarray(act), np.asarray(rew, np.float64), np.asarray(flag, np.float64)
    kappa = float(kappa)
    rows = np.arange(B)
    _, astar = textbook_q(next_target if next_online is None else next_online)
    gnt = (float(gamma_n) * (1.0 - flag))[:, None] * next_target[rows, astar]
    T = rew[:, None] + gnt
    theta = quant[rows, act]
    tau = (2.0 * np.arange(N) + 1.0) / (2.0 * N)
    u = T[:, None, :] - theta[:, :, None]
    au = np.abs(u)
    with np.errstate(over="ignore"):
        H = np.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa))
    wt = np.abs(tau[None, :, None] - (u < 0))
    row_loss = (wt * H / kappa).sum(axis=2).sum(axis=1) / N
    dtheta = -(wt * np.clip(u, -kappa, kappa) / kappa).sum(axis=2) / N
    wb = np.ones(B) if w is None else np.asarray(w, np.float64)
    dquant = np.zeros((B, A, N))
    dquant[rows, act] = (wb / B)[:, None] * dtheta
    return types.SimpleNamespace(row_loss=row_loss, dquant=dquant, astar=astar, u=u, T=T, theta=theta, gnt=gnt)


# ------------------------------------------------------------------ the shared cases ----
LARGE = 1e30


def large_rows(B):
    """-> bool[B]: the rows case() scales to magnitudes near LARGE.  Their loss terms (about 1e32) swamp any float64 sum they
    are part of, so a check of loss_sum that is to see the other rows gives these w = 0."""
    return np.arange(B) % 16 == 6


def case(B, A, N, kappa=1.0, seed=0):
    """One batch that walks the head's edges; rows cycle through the row kinds below, so every B >= 1 gets the first B of them.
    -> dict(quant, next_target, next_online f32[B, A, N]; act i32[B]; rew, flag, w f32[B]; gamma_n; kappa)."""
    rng = np.random.default_rng(1000 * B + 10 * A + N + seed)
    gamma_n = 0.99 ** 3
    quant, nt, no = ((3.0 * rng.normal(size=(B, A, N))).astype(F32) for _ in range(3))
    act = rng.integers(0, A, size=B).astype(np.int32)
    rew = rng.choice([1.0, 0.0, -1.0, 0.37], size=B).astype(F32)
    flag = (rng.random(B) < 0.25).astype(F32)
    w = rng.uniform(0.1, 2.0, size=B).astype(F32)
    kap = F32(kappa)
    for b in range(B):
        k = b % 16
        if k == 1:                          # equal quantiles across the actions: every mean ties, a* = 0
            nt[b], no[b] = nt[b, 0], no[b, 0]
        elif k == 2:                        # the two nets disagree on a*: the online net lifts action 0, the target net A - 1
            no[b], nt[b] = F32(0.1) * no[b], F32(0.1) * nt[b]
            no[b, A - 1] -= F32(3.0)
            no[b, 0] += F32(3.0)
            nt[b, 0] -= F32(3.0)
            nt[b, A - 1] += F32(3.0)
        elif k == 3:                        # u == 0: some theta_i are exactly a T_j of a live row (every action the same target
            nt[b], flag[b] = nt[b, 0], 0.0  # quantiles, so whichever a* — but for this gamma_n only; rows 9 cover gamma_n = 0)
            T = rew[b] + F32(gamma_n) * (F32(1.0) - flag[b]) * nt[b, 0]
            for i in range(0, N, 2):
                quant[b, act[b], i] = T[(3 * i + 1) % N]
        elif k == 4:                        # |u| == kappa exactly, in binary-exact values: T_j = 0.5, theta_i = 0.5 -+ kappa
            rew[b], flag[b] = 0.5, 1.0
            quant[b, act[b]] = np.round(4.0 * quant[b, act[b]]) / 4.0
            quant[b, act[b], 0::3] = F32(0.5) - kap
            quant[b, act[b], 1::3] = F32(0.5) + kap
        elif k == 5:                        # fully crossed quantiles: both rows descending
            quant[b, act[b]] = -np.sort(-quant[b, act[b]])
            nt[b] = -np.sort(-nt[b], axis=-1)
        elif k == 6:                        # the linear branch at magnitudes near 1e30: (0.5 u) u overflows in the unused branch
            quant[b], nt[b], no[b], rew[b], flag[b] = quant[b] * F32(LARGE), nt[b] * F32(LARGE), no[b] * F32(LARGE), LARGE, 0.0
        elif k in (7, 8):                   # terminal rows: every T_j is the reward
            flag[b] = 1.0
        elif k == 9:                        # ... and every theta_i too: loss and gradient exactly 0
            flag[b] = 1.0
            quant[b, act[b]] = rew[b]
        elif k in (11, 12):                 # a zero weight
            w[b] = 0.0
    return dict(quant=quant, next_target=nt, next_online=no, act=act, rew=rew, flag=flag, w=w, gamma_n=gamma_n, kappa=float(kappa))
