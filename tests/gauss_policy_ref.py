"""Host restatement of the diagonal-Gaussian policy of include/gymrl.h ("Gaussian policy") — TEST INFRASTRUCTURE, no GPU.

Built on tests/det_math_ref.py: float32 throughout, numpy rounds every operation once (the library is built with
-ffp-contract=off), the grouping as the header writes it, sums over k ascending from 0.0f.  So the sampling side (draw, action,
log-probability, entropy) carries the kernels' bits; the loss side differs from the kernel only in the order of the float64
batch sums (the metrics and dlog_std).

    draw_eps            Philox4x32-10 + Box-Muller, the keys of gaussian_pick
    sample              a = mu + exp(log_std) * eps, logp, entropy
    loss                gymrl_ppo_gauss_loss_fwd_bwd: dmu, dvalue, dlog_std and the five metric sums
    loss_f64            the float64 reference: torch.distributions.Normal + autograd
    case / planted      the inputs the CPU and GPU tests share
"""
import json
import os

import numpy as np

import det_math_ref as dm

F32 = np.float32
M32 = np.uint64(0xFFFFFFFF)
RNG_POLICY = 0x30000000
HALF_LOG_2PI = F32(0.918938533)
ENTROPY0 = F32(1.418938533)
TWO_PI = F32(6.28318530717958647692)
CFG = (0.2, 3.0, 0.5, 0.01)                 # clip_eps, dual_clip, value_coef, entropy_coef (ppo_lunarlander.Config)
TOLERANCES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "ppo_gauss_tolerances.json")


def philox4x32(key, c0, c1, c2, c3):
    """Philox4x32-10 over uint64 arrays of 32-bit words (csrc/gymrl_device.hpp philox4x32) -> four word arrays."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64((key >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def box_muller(w0, w1):
    """two word arrays -> float32 N(0, 1): sqrtf(-2 det_logf(u1)) * det_cosf(2 pi u2), u1 in (0, 1], u2 in [0, 1)"""
    u1 = ((w0 >> np.uint64(8)) + np.uint64(1)).astype(F32) * F32(2.0 ** -24)
    u2 = (w1 >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)
    _, c = dm.sincosf(TWO_PI * u2)
    return np.sqrt(F32(-2.0) * dm.logf(u1)) * c


def draw_eps(seed, env_ids, counter, A):
    """eps f32[N, A] of envs `env_ids` at `counter`: block k / 2 of the categorical's key, words (x, y) then (z, w)."""
    env = np.asarray(env_ids, np.uint64)
    out = np.empty((env.size, A), F32)
    for blk in range((A + 1) // 2):
        c3 = RNG_POLICY | (((counter >> 32) & 0x3FFFFF) << 2) | blk
        w = philox4x32(seed, env & M32, env >> np.uint64(32), np.uint64(counter & 0xFFFFFFFF), np.uint64(c3))
        for h in range(2):
            if 2 * blk + h < A:
                out[:, 2 * blk + h] = box_muller(w[2 * h], w[2 * h + 1])
    return out


def _logp_entropy(z, log_std):
    lp, H = np.zeros(z.shape[0], F32), np.zeros(z.shape[0], F32)
    for k in range(z.shape[1]):
        lp = lp + ((F32(-0.5) * (z[:, k] * z[:, k]) - log_std[k]) - HALF_LOG_2PI)
        H = H + (ENTROPY0 + log_std[k])
    return lp, H


def sample(mu, log_std, eps=None, deterministic=False):
    """-> (action f32[N, A], logp f32[N], entropy f32[N]); eps f32[N, A] the normal draws (unused when deterministic)"""
    mu, log_std = np.asarray(mu, F32), np.asarray(log_std, F32)
    if deterministic:
        eps, act = np.zeros_like(mu), mu.copy()
    else:
        eps = np.asarray(eps, F32)
        act = mu + dm.expf(log_std)[None, :] * eps
    lp, H = _logp_entropy(eps, log_std)
    return act, lp, H


def normalise(adv, moments):
    """gymrl_ppo_loss_fwd_bwd's on-the-fly normalisation: float64 (adv - mean) / (population std + 1e-8), rounded to float32"""
    cnt, s, ss = (float(x) for x in moments)
    mean = s / cnt
    var = max(ss / cnt - mean * mean, 0.0)
    return ((np.asarray(adv, F32).astype(np.float64) - mean) / (np.sqrt(var) + 1e-8)).astype(F32)


def loss(mu, log_std, value, act, logp_old, adv, ret, cfg=CFG, moments=None):
    """-> dict(dmu f32[B, A], dvalue f32[B], dlog_std f32[A], metrics f64[5] sums, logp f32[B]) in the kernel's float32 lines"""
    mu, log_std, value, act, logp_old, adv, ret = (np.asarray(x, F32) for x in (mu, log_std, value, act, logp_old, adv, ret))
    clip_eps, dual_clip, value_coef, entropy_coef = (F32(c) for c in cfg)
    B, A = mu.shape
    if moments is not None:
        adv = normalise(adv, moments)
    invB = F32(1.0) / F32(B)
    inv_std = dm.expf(-log_std)
    z = (act - mu) * inv_std[None, :]
    lp, H = _logp_entropy(z, log_std)
    lo, hi = F32(1.0) - clip_eps, F32(1.0) + clip_eps
    with np.errstate(invalid="ignore"):
        ratio = dm.expf(lp - logp_old)
        s1 = ratio * adv
        s2 = np.minimum(np.maximum(ratio, lo), hi) * adv
        inr = ((ratio >= lo) & (ratio <= hi)).astype(F32)
        w1 = np.where(s1 < s2, F32(1.0), np.where(s1 == s2, F32(0.5), F32(0.0))).astype(F32)
        ms = np.minimum(s1, s2)
        dms = w1 * adv + (F32(1.0) - w1) * adv * inr
        dc = dual_clip * adv
        neg = adv < 0
        obj = np.where(neg, np.maximum(ms, dc), ms).astype(F32)
        wm = np.where(ms > dc, F32(1.0), np.where(ms == dc, F32(0.5), F32(0.0))).astype(F32)
        dms = np.where(neg, dms * wm, dms).astype(F32)
    g_lp = -invB * dms * ratio
    g_H = -entropy_coef * invB
    dmu = g_lp[:, None] * (z * inv_std[None, :])
    dls_rows = g_lp[:, None] * (z * z - F32(1.0)) + g_H
    dvr = value - ret
    dvalue = value_coef * F32(2.0) * dvr * invB
    m = np.stack([-obj, value_coef * (dvr * dvr), H, ((ratio < lo) | (ratio > hi)).astype(F32), logp_old - lp], axis=1)
    return dict(dmu=dmu.astype(F32), dvalue=dvalue.astype(F32), dlog_std=dls_rows.astype(np.float64).sum(axis=0).astype(F32),
                metrics=m.astype(np.float64).sum(axis=0), logp=lp, entropy=H)


def loss_f64(mu, log_std, value, act, logp_old, adv, ret, cfg=CFG, moments=None):
    """The float64 reference of the same loss: torch.distributions.Normal, autograd on the mean loss."""
    import torch
    clip_eps, dual_clip, value_coef, entropy_coef = cfg
    t = lambda x, g=False: torch.tensor(np.asarray(x, F32).astype(np.float64), requires_grad=g)   # noqa: E731
    mu_t, ls_t, v_t = t(mu, True), t(log_std, True), t(value, True)
    adv = np.asarray(adv, F32)
    if moments is not None:
        adv = normalise(adv, moments)
    dist = torch.distributions.Normal(mu_t, ls_t.exp().expand_as(mu_t))
    lp = dist.log_prob(t(act)).sum(-1)
    H = dist.entropy().sum(-1)
    ad, lpo = t(adv), t(logp_old)
    ratio = (lp - lpo).exp()
    obj = torch.min(ratio * ad, ratio.clamp(1.0 - clip_eps, 1.0 + clip_eps) * ad)
    obj = torch.where(ad < 0, torch.max(obj, dual_clip * ad), obj)
    vl = value_coef * (v_t - t(ret)) ** 2
    total = (-obj).mean() + vl.mean() - entropy_coef * H.mean()
    total.backward()
    lo, hi = 1.0 - clip_eps, 1.0 + clip_eps
    m = torch.stack([(-obj).sum(), vl.sum(), H.sum(), ((ratio < lo) | (ratio > hi)).double().sum(), (lpo - lp).sum()])
    return dict(dmu=mu_t.grad.numpy(), dvalue=v_t.grad.numpy(), dlog_std=ls_t.grad.numpy(), metrics=m.detach().numpy(),
                logp=lp.detach().numpy(), entropy=H.detach().numpy())


# every (side of a clip boundary) x (sign of the advantage) a row can land on; ratios keep 5 % clear of a boundary so that float32
# and float64 fall on the same side (at a boundary the loss has a kink and the two gradients legitimately differ)
PLANTED = ((0.75, 1.0), (0.85, 1.0), (1.15, 1.0), (1.25, 1.0), (0.75, -1.0), (0.85, -1.0), (1.15, -1.0), (1.25, -1.0),
           (2.85, -1.0), (3.15, -1.0), (5.0, -2.0), (3.15, 1.0), (1.0, 0.0))
SHAPES = tuple((B, A, ls) for B in (1, 65, 257) for A in (1, 3) for ls in (-3.0, 0.0, 1.0))


def case(B, A, log_std, seed=0):
    """Inputs of the loss at (B, A): random rows, with PLANTED (ratio, advantage) pairs written over the first rows that fit."""
    rng = np.random.default_rng(1000 * B + 10 * A + seed)
    ls = np.full(A, log_std, F32) + (0.1 * rng.normal(size=A)).astype(F32)
    mu = rng.normal(size=(B, A)).astype(F32)
    eps = rng.normal(size=(B, A)).astype(F32)
    act = (mu + np.exp(ls)[None, :] * eps).astype(F32)
    value, ret = rng.normal(size=B).astype(F32), rng.normal(size=B).astype(F32)
    adv = rng.normal(size=B).astype(F32)
    z = (act.astype(np.float64) - mu) * np.exp(-ls.astype(np.float64))
    lp = (-0.5 * z * z - ls.astype(np.float64) - 0.5 * np.log(2 * np.pi)).sum(axis=1)
    ratio = np.exp(0.1 * rng.normal(size=B))
    for k, (r, a) in enumerate(PLANTED[:B]):
        ratio[k], adv[k] = r, a
    logp_old = (lp - np.log(ratio)).astype(F32)
    return dict(mu=mu, log_std=ls, value=value, act=act, logp_old=logp_old, adv=adv, ret=ret)


def deviations(got, want, B):
    """name -> max |got - want| / max(1, |want|): gradients scaled by B to O(1), the metric sums as means"""
    rel = lambda g, w, s: float(np.max(np.abs(np.asarray(g, np.float64) * s - np.asarray(w, np.float64) * s) /   # noqa: E731
                                       np.maximum(1.0, np.abs(np.asarray(w, np.float64) * s))))
    return {"dmu": rel(got["dmu"], want["dmu"], B), "dvalue": rel(got["dvalue"], want["dvalue"], B),
            "dlog_std": rel(got["dlog_std"], want["dlog_std"], 1.0), "metrics": rel(got["metrics"], want["metrics"], 1.0 / B)}


def measure():
    """The float32 restatement against the float64 reference over SHAPES, with and without normalisation -> name -> the largest
    deviation.  tests/test_gauss_policy_ref.py holds profiles/ppo_gauss_tolerances.json to this."""
    worst = {"dmu": 0.0, "dvalue": 0.0, "dlog_std": 0.0, "metrics": 0.0, "logp": 0.0, "entropy": 0.0}
    for B, A, ls in SHAPES:
        c = case(B, A, ls)
        for moments in (None, (B, float(c["adv"].astype(np.float64).sum()), float((c["adv"].astype(np.float64) ** 2).sum()))):
            if moments is not None and B == 1:
                continue                        # one row has no spread: the normalised advantage is 0 / 1e-8
            got, want = loss(**c, moments=moments), loss_f64(**c, moments=moments)
            d = deviations(got, want, B)
            d["logp"] = float(np.max(np.abs(got["logp"] - want["logp"]) / np.maximum(1.0, np.abs(want["logp"]))))
            d["entropy"] = float(np.max(np.abs(got["entropy"] - want["entropy"]) / np.maximum(1.0, np.abs(want["entropy"]))))
            worst = {k: max(v, d[k]) for k, v in worst.items()}
    return worst


def write_tolerances(path=TOLERANCES):
    worst = measure()
    doc = {"what": "largest deviation of tests/gauss_policy_ref.py's float32 restatement from its float64 torch.distributions.Normal "
                   "reference over gauss_policy_ref.SHAPES (|got - want| / max(1, |want|); gradients scaled by B, metric sums as "
                   "means), and the bound the kernel is held to: 4 x that, the kernel differing from the restatement only in "
                   "the order of the batch reduction",
           "bounds": [{"name": k, "observed": v, "bound": 4.0 * v} for k, v in sorted(worst.items())]}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


def tolerances(path=TOLERANCES):
    with open(path) as f:
        return {b["name"]: b for b in json.load(f)["bounds"]}


if __name__ == "__main__":
    print(json.dumps(write_tolerances(), indent=1))
