"""The on-policy loss kernels' independent witnesses: float64 CPU-torch autograd references for L1
(gymrl_ppo_loss_fwd_bwd), L3 (gymrl_ppo_full_loss_fwd_bwd) and L4 (gymrl_ppo_rnn_loss_fwd_bwd), written from the reference
program's expressions (ppo_lunarlander.py:278-322, ppo_full_lunarlander.py:575-652, ppo_lstm_lunarlander.py:716-776) and not
from the kernels; one input builder that plants designed rows and keeps every discrete decision clear of its threshold;
and the comparisons, which tests/test_onpolicy_edges_gpu.py runs on the HIP kernels and tests/test_onpolicy_edges.py on the C
oracle that restates them.  A plain helper module: no fixtures, no hooks."""
import functools
import math
import types
import zlib
from fractions import Fraction

import numpy as np
import torch
from torch.distributions import Categorical

from conftest import bounded, rel_close

TOL = 1e-5                                       # the project's contract
MARGIN = 1e-3                                    # relative distance every decision quantity keeps from its threshold
PPO_CFG = (0.2, 3.0, 0.5, 0.01)                  # clip_eps, dual_clip, value_coef, entropy_coef
FULL_CFG = (0.2, 0.28, 3.0, 0.06, 0.06, 0.01)    # clip_eps_min, clip_eps_max, dual_clip, erc_beta_low, erc_beta_high, entropy_coef
SAT = (40.0, 0.0, -1.0, 0.5, 0.25, -0.5, 1.0, -2.0)   # p[0] = 1 - 1e-17: every other action has log p of about -40
N_METRICS = {"ppo": 5, "ppo_full": 9, "ppo_rnn": 10}
COUNT_METRICS = {"ppo": (3,), "ppo_full": (3, 5), "ppo_rnn": (3, 5, 9)}    # sums of 0 / 1 terms: integers, compared exactly


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _t(a, grad=False):
    return torch.tensor(_np(a).astype(np.float64), requires_grad=grad)


def _cfg32(cfg):
    """The configuration as the kernels receive it: float32 values (then carried in float64)."""
    return tuple(float(np.float32(c)) for c in cfg)


def _rows(idx, B, *arrs):
    i = np.arange(B) if idx is None else _np(idx).astype(np.int64)
    return [_np(a)[i] for a in arrs]


def _grads(loss, z, v):
    if loss.requires_grad:                       # masked_mean of an empty mask is a constant 0: nothing to differentiate
        loss.backward()
    return tuple(np.zeros(tuple(x.shape)) if x.grad is None else x.grad.numpy() for x in (z, v))


def norm_constants(adv_moments):
    """(mean, population std) of (count, sum, sum of squares), in exact rational arithmetic: the float64 subtraction
    sumsq / n - mean^2 cancels, and the reference must not share that rounding with the kernel."""
    cnt, s1, s2 = (Fraction(float(x)) for x in _np(adv_moments))
    mean = s1 / cnt
    var = max(s2 / cnt - mean * mean, Fraction(0))
    return float(mean), math.sqrt(float(var))


# ---------------------------------------------------------------------------------------------- references ----
def ref_ppo_loss(logits, value, act, logp_old, adv, ret, cfg, idx=None, adv_moments=None):
    """L1: ppo_lunarlander.py:278-322 (and :236 when adv_moments is given).  Returns (dlogits, dvalue, metric sums[5])."""
    clip_eps, dual_clip, value_coef, entropy_coef = _cfg32(cfg)
    B = len(logits)
    a, lpo, ad, rt = _rows(idx, B, act, logp_old, adv, ret)
    z, v, lpo, ad, rt = _t(logits, True), _t(value, True), _t(lpo), _t(ad), _t(rt)
    if adv_moments is not None:
        mean, std = norm_constants(adv_moments)
        ad = (ad - mean) / (std + 1e-8)                                                    # :236
    dist = Categorical(logits=z)
    new_log_probs, entropy = dist.log_prob(torch.from_numpy(a.astype(np.int64))), dist.entropy()
    ratio = torch.exp(new_log_probs - lpo)                                                 # :278
    surr1 = ratio * ad
    surr2 = torch.clamp(ratio, 1 - clip_eps, 1 + clip_eps) * ad
    min_surr = torch.min(surr1, surr2)
    obj = torch.where(ad < 0, torch.max(min_surr, dual_clip * ad), min_surr)               # :286-292
    policy_loss = -torch.mean(obj)
    value_loss = value_coef * torch.mean((v - rt).pow(2))
    entropy_loss = -entropy_coef * entropy.mean()
    dz, dv = _grads(policy_loss + value_loss + entropy_loss, z, v)
    with torch.no_grad():
        clipped = ((ratio < 1 - clip_eps) | (ratio > 1 + clip_eps)).double()
        met = [-obj.sum(), value_coef * (v - rt).pow(2).sum(), entropy.sum(), clipped.sum(), (lpo - new_log_probs).sum()]
    return dz, dv, np.array([float(m) for m in met])


def _full_common(logits, value, act, logp_old, ent_old, adv, ret, cfg, idx, corr_mul, entropy_coef_dev):
    cmin, cmax, dual_clip, beta_low, beta_high, ent_coef = _cfg32(cfg)
    if entropy_coef_dev is not None:
        ent_coef = float(np.float32(_np(entropy_coef_dev).ravel()[0]))
    B = len(logits)
    a, lpo, eo, ad, rt = _rows(idx, B, act, logp_old, ent_old, adv, ret)
    z, v, lpo, eo, ad, rt = _t(logits, True), _t(value, True), _t(lpo), _t(eo), _t(ad), _t(rt)
    dist = Categorical(logits=z)
    new_log_probs, new_entropies = dist.log_prob(torch.from_numpy(a.astype(np.int64))), dist.entropy()
    with torch.no_grad():                                                                  # the masks are constants
        entropy_ratio = new_entropies / (eo + 1e-8)                                        # :586
        erc_mask = ((entropy_ratio > 1 - beta_low) & (entropy_ratio < 1 + beta_high)).double()
        corr = torch.ones_like(ad) * erc_mask
        if corr_mul is not None:
            corr = corr * _t(corr_mul)                                                     # corr[clip_idx] = 0  :616
    ratio = (new_log_probs - lpo).exp()
    surr1 = ratio.clamp(0.0, dual_clip) * ad
    surr2 = torch.clamp(ratio, 1 - cmin, 1 + cmax) * ad
    with torch.no_grad():
        clipped = ((ratio < 1 - cmin) | (ratio > 1 + cmax)).double()
    tail = lambda: [float(x) for x in ((lpo - new_log_probs).sum(), (1 - erc_mask).sum(), new_log_probs.sum(), ad.sum(),   # noqa: E731
                                      (new_log_probs * ad).sum())]
    return types.SimpleNamespace(z=z, v=v, ad=ad, rt=rt, corr=corr, surr=-torch.min(surr1, surr2), H=dist.entropy(),
                                 clipped=clipped, ent_coef=ent_coef, cmin=cmin, cmax=cmax, tail=tail)


def ref_ppo_full_loss(logits, value, act, logp_old, ent_old, adv, ret, cfg, idx=None, corr_mul=None, entropy_coef_dev=None):
    """L3: ppo_full_lunarlander.py:575-652.  Returns (dlogits, dvalue, metric sums[9])."""
    c = _full_common(logits, value, act, logp_old, ent_old, adv, ret, cfg, idx, corr_mul, entropy_coef_dev)
    policy_loss = torch.mean(c.surr * c.corr)                                              # :624
    value_loss = torch.mean(0.5 * c.corr * (c.v - c.rt).pow(2))                            # :627-629
    entropy = (c.H * c.corr).mean()                                                        # :632
    entropy_loss = torch.mean(-c.ent_coef * entropy)
    dz, dv = _grads(policy_loss + value_loss + entropy_loss, c.z, c.v)
    with torch.no_grad():
        head = [float(x) for x in ((c.surr * c.corr).sum(), (0.5 * c.corr * (c.v - c.rt).pow(2)).sum(), (c.H * c.corr).sum(),
                                   (c.clipped * c.corr).sum())]
        return dz, dv, np.array(head + c.tail())


def masked_mean(x, mask):
    """ppo_lstm_lunarlander.py:646-655."""
    masked_count = mask.sum()
    if masked_count == 0:
        return torch.tensor(0.0, dtype=x.dtype)
    return (x * mask).sum() / masked_count


def ref_ppo_rnn_loss(logits, value, act, logp_old, ent_old, val_old, adv, ret, cfg, idx=None, corr_mul=None):
    """L4: ppo_lstm_lunarlander.py:716-776 without the RND term.  Returns (dlogits, dvalue, metric sums[10])."""
    c = _full_common(logits, value, act, logp_old, ent_old, adv, ret, cfg, idx, corr_mul, None)
    vo = _t(_rows(idx, len(logits), val_old)[0])
    policy_loss = masked_mean(c.surr, c.corr)                                              # :761
    value_clip = vo + (c.v - vo).clamp(-c.cmin, c.cmax)                                    # :763-765
    value_max = torch.max((c.v - c.rt).pow(2), (value_clip - c.rt).pow(2))
    value_loss = 0.5 * masked_mean(value_max, c.corr)
    entropy_loss = c.ent_coef * -masked_mean(c.H, c.corr)
    dz, dv = _grads(policy_loss + value_loss + entropy_loss, c.z, c.v)
    with torch.no_grad():
        head = [float(x) for x in ((c.surr * c.corr).sum(), (0.5 * c.corr * value_max).sum(), (c.H * c.corr).sum(),
                                   (c.clipped * c.corr).sum())]
        return dz, dv, np.array(head + c.tail() + [float(c.corr.sum())])


REFERENCES = {"ppo": ref_ppo_loss, "ppo_full": ref_ppo_full_loss, "ppo_rnn": ref_ppo_rnn_loss}


# ------------------------------------------------------------------------------------------------- builder ----
def _log_softmax64(logits):
    z = logits.astype(np.float64)
    ln = z - z.max(1, keepdims=True)
    ln = ln - np.log(np.exp(ln).sum(1, keepdims=True))
    return ln, -(np.exp(ln) * ln).sum(1)


def _plants(kind, A):
    """The designed rows, in planting order: name -> overrides.  dlp = lp - logp_old (ratio = exp(dlp)), ad = the advantage the
    loss sees, er = the entropy ratio, dv = v - v_old, dret = ret - v."""
    cmin, cmax = FULL_CFG[0], FULL_CFG[1]
    p = [("sat_likely", dict(sat=True, act=0, dlp=0.1, ad=1.3)),
         ("sat_unlikely", dict(sat=True, act=1, dlp=-0.1, ad=0.9)),                # |lp| = 40
         ("over_dual_adv_pos", dict(dlp=1.5, ad=1.1)),                             # ratio 4.48 > dual_clip
         ("over_dual_adv_neg", dict(dlp=1.5, ad=-1.1)),
         ("under_lo_adv_pos", dict(dlp=-0.5, ad=0.8)),                             # ratio 0.61 < lo
         ("under_lo_adv_neg", dict(dlp=-0.5, ad=-0.8)),
         ("adv_zero", dict(dlp=0.4, ad=0.0)),                                      # min(0, 0): the tie float32 and float64 share
         ("between_hi_and_dual_adv_neg", dict(dlp=math.log(2.0), ad=-1.0))]
    if kind == "ppo":
        p.append(("dual_clip_binds", dict(dlp=math.log(5.0), ad=-1.2)))            # adv < 0, ratio = 5
    else:
        p += [("erc_below", dict(er=0.8, dlp=0.1, ad=1.0)), ("erc_above", dict(er=1.2, dlp=-0.1, ad=-1.0)),
              ("corr_mul_zero", dict(er=1.0, corr_mul=0.0, dlp=0.05, ad=1.0))]
    if kind == "ppo_rnn":
        for tag, dv in (("m2", -2 * cmin), ("mh", -cmin / 2), ("ph", cmax / 2), ("p2", 2 * cmax)):
            p += [(f"vclip_{tag}_ret_above", dict(dv=dv, dret=0.75)), (f"vclip_{tag}_ret_below", dict(dv=dv, dret=-0.75))]
        p += [("v_equals_v_old_ret_above", dict(dv=0.0, dret=0.75)), ("v_equals_v_old_ret_below", dict(dv=0.0, dret=-0.75))]
    return p


def decisions(c):
    """Every discrete decision of the loss as (name, quantity, threshold, rows it applies to, array a near row is moved by),
    in float64 on the float32 inputs."""
    B = c.B
    i = np.arange(B) if c.idx is None else c.idx.astype(np.int64)
    lnp, H = _log_softmax64(c.logits)
    lp = lnp[np.arange(B), c.act[i]]
    ratio = np.exp(lp - c.logp_old[i].astype(np.float64))
    ad = c.adv[i].astype(np.float64)
    every = np.ones(B, bool)
    if c.kind == "ppo":
        clip_eps, dual_clip = _cfg32(c.cfg)[:2]
        if c.adv_moments is not None:
            mean, std = norm_constants(c.adv_moments)
            ad = (ad - mean) / (std + 1e-8)
        ms = np.minimum(ratio * ad, np.clip(ratio, 1 - clip_eps, 1 + clip_eps) * ad)
        return [("ratio|lo", ratio, 1 - clip_eps, every, "logp_old"), ("ratio|hi", ratio, 1 + clip_eps, every, "logp_old"),
                ("ms|dual_clip*adv", ms, dual_clip * ad, ad < 0, "logp_old")]
    cmin, cmax, dual_clip, beta_low, beta_high = _cfg32(c.cfg)[:5]
    er = H / (c.ent_old[i].astype(np.float64) + 1e-8)
    s1, s2 = np.clip(ratio, 0.0, dual_clip) * ad, np.clip(ratio, 1 - cmin, 1 + cmax) * ad
    outside = ((ratio < 1 - cmin) | (ratio > 1 + cmax)) & (ad != 0)        # inside [lo, hi], or at adv == 0, s1 == s2 is the intended tie
    out = [("ratio|lo", ratio, 1 - cmin, every, "logp_old"), ("ratio|hi", ratio, 1 + cmax, every, "logp_old"),
           ("ratio|dual_clip", ratio, dual_clip, every, "logp_old"),
           ("er|1-beta_low", er, 1 - beta_low, every, "ent_old"), ("er|1+beta_high", er, 1 + beta_high, every, "ent_old"),
           ("s1|s2", s1, s2, outside, "logp_old")]
    if c.kind == "ppo_rnn":
        v, vo, rt = (x.astype(np.float64) for x in (c.value, c.val_old[i], c.ret[i]))
        dv = v - vo
        l1, l2 = (v - rt) ** 2, (vo + np.clip(dv, -cmin, cmax) - rt) ** 2
        out += [("dv|-eps", dv, -cmin, every, "val_old"), ("dv|+eps", dv, cmax, every, "val_old"),
                ("l1|l2", l1, l2, (dv < -cmin) | (dv > cmax), "val_old")]      # unclipped rows: value_clip == v, the intended tie
    return out


STEP = {"logp_old": np.float32(0.05), "ent_old": np.float32(0.02), "val_old": np.float32(0.05)}


def _near(q, thr, rows):
    """Rows within MARGIN of the threshold, relative to it (to the larger of the two where the threshold is a per-row value)."""
    size = np.abs(thr) if np.ndim(thr) == 0 else np.maximum(np.abs(thr), np.abs(q))
    return rows & (np.abs(q - thr) < MARGIN * size)


def enforce_margins(c):
    """Moves every row that sits within MARGIN of a threshold by a fixed step of logp_old / ent_old / val_old, then asserts that
    no row of the batch is inside any margin.  No row is dropped: the comparisons see all B of them."""
    i = np.arange(c.B) if c.idx is None else c.idx.astype(np.int64)
    moved = np.zeros(c.B, bool)
    for _ in range(40):
        bad = {}
        for _, q, thr, rows, field in decisions(c):
            bad[field] = bad.get(field, np.zeros(c.B, bool)) | _near(q, thr, rows)
        if not any(b.any() for b in bad.values()):
            break
        for field, b in bad.items():
            getattr(c, field)[i[b]] += STEP[field]
            moved |= b
    for name, q, thr, rows, _ in decisions(c):
        assert not _near(q, thr, rows).any(), (name, int(_near(q, thr, rows).sum()))
    assert not moved[list(c.planted.values())].any(), "a planted row sat on a threshold"
    c.moved = int(moved.sum())
    return c


def make_case(rng, B, A, M=None, kind="ppo", adv_moments=None, mask=None, plant=True):
    """One input set for ref_* / ops.* / oracle.*: B rows of A logits, read through idx (a random subset of a rollout of M
    entries) when M is given.  kind: "ppo" (L1), "ppo_full" (L3), "ppo_rnn" (L4).  adv_moments: None, "rollout" (the moments
    of the rollout's own advantages) or "tiny" (a nearly constant advantage vector, variance 1e-10).  mask: None, "none"
    (every row outside the entropy band) or ("one", r) (row r alone inside).  The designed rows of _plants() go to rows
    1, 3, 5, ... below B; `planted` maps their names to their rows."""
    assert kind in REFERENCES and 2 <= A <= 8 and (M is None or M >= B)
    c = types.SimpleNamespace(kind=kind, B=B, A=A, M=M, cfg=PPO_CFG if kind == "ppo" else FULL_CFG, planted={}, sat_rows=[],
                              corr_mul=None, adv_moments=None, entropy_coef_dev=None)
    R = B if M is None else M
    c.idx = None if M is None else rng.permutation(M)[:B].astype(np.int32)
    i = np.arange(B) if c.idx is None else c.idx.astype(np.int64)
    c.logits = (rng.normal(size=(B, A)) * 1.5).astype(np.float32)
    c.value = rng.normal(size=B).astype(np.float32)
    act = rng.integers(0, A, size=R).astype(np.int32)
    dlp, ad, er = rng.normal(size=B) * 0.3, rng.normal(size=B), rng.uniform(0.85, 1.15, size=B)
    dv, dret = rng.uniform(-0.5, 0.5, size=B), rng.normal(size=B)
    corr_mul = (rng.random(B) >= 0.1).astype(np.float32)
    if mask is not None:
        er = np.where(np.arange(B) % 2 == 0, 0.8, 1.2)
        if mask != "none":
            er[mask[1]] = 1.0
        plant = False
    if plant:
        for j, (name, o) in enumerate(_plants(kind, A)):
            r = 1 + 2 * j
            if r >= B:
                break
            c.planted[name] = r
            er[r], corr_mul[r] = o.get("er", 1.0), o.get("corr_mul", 1.0)
            if o.get("sat"):
                c.logits[r] = SAT[:A]
                c.sat_rows.append(r)
            if "act" in o:
                act[i[r]] = o["act"]
            for arr, key, default in ((dlp, "dlp", 0.05), (ad, "ad", 1.0), (dv, "dv", 0.1), (dret, "dret", 0.6)):
                arr[r] = o.get(key, default)                           # what a plant does not design is well inside its branch
    lnp, H = _log_softmax64(c.logits)
    lp = lnp[np.arange(B), act[i]]
    c.act = act
    # the rollout-sized arrays: entries no row reads hold plausible values of their own
    c.logp_old, c.ent_old, c.val_old, c.adv, c.ret = ((rng.normal(size=R) * s + m).astype(np.float32)
                                                      for s, m in ((0.5, -1.2), (0.1, 0.9), (1.0, 0.0), (1.0, 0.0), (1.0, 0.0)))
    c.logp_old[i] = (lp - dlp).astype(np.float32)
    c.ent_old[i] = (H / er).astype(np.float32)
    c.val_old[i] = c.value - dv.astype(np.float32)
    c.val_old[i[dv == 0.0]] = c.value[dv == 0.0]                                   # v == v_old, bit for bit
    c.ret[i] = c.value + dret.astype(np.float32)
    if adv_moments == "tiny":                                                      # std 1e-5 beside the +1e-8 of :236
        c.adv = (0.5 + 1e-5 * rng.normal(size=R)).astype(np.float32)
        c.adv[i[list(c.planted.values())]] = (0.5 + 1e-5 * ad[list(c.planted.values())]).astype(np.float32)
    else:
        c.adv[i] = ad.astype(np.float32)
    if adv_moments is not None:
        a64 = c.adv.astype(np.float64)
        c.adv_moments = np.array([float(R), math.fsum(a64.tolist()), math.fsum((a64 * a64).tolist())])
        if adv_moments == "tiny":
            var = c.adv_moments[2] / R - (c.adv_moments[1] / R) ** 2
            assert 2e-11 < var < 5e-10, var
    if kind != "ppo" and mask is None:
        c.corr_mul = corr_mul
    assert c.idx is None or (np.unique(c.idx).size == B and 0 <= c.idx.min() and c.idx.max() < R)   # the kernels trust idx and act
    assert 0 <= c.act.min() and c.act.max() < A and all(len(x) == R for x in (c.act, c.logp_old, c.ent_old, c.val_old, c.adv, c.ret))
    return enforce_margins(c)


def case_args(c, as_array=lambda a: a):
    """(positional, keyword) arguments of ref_* / ops.* / oracle.* for case c."""
    f = lambda a: None if a is None else as_array(a)   # noqa: E731
    kw = dict(idx=f(c.idx))
    if c.kind == "ppo":
        return [f(x) for x in (c.logits, c.value, c.act, c.logp_old, c.adv, c.ret)] + [c.cfg], dict(kw, adv_moments=f(c.adv_moments))
    kw["corr_mul"] = f(c.corr_mul)
    if c.kind == "ppo_full":
        return ([f(x) for x in (c.logits, c.value, c.act, c.logp_old, c.ent_old, c.adv, c.ret)] + [c.cfg],
                dict(kw, entropy_coef_dev=f(c.entropy_coef_dev)))
    return [f(x) for x in (c.logits, c.value, c.act, c.logp_old, c.ent_old, c.val_old, c.adv, c.ret)] + [c.cfg], kw


def reference(c):
    """The float64 reference of case c, computed once and kept with the case."""
    if getattr(c, "ref", None) is None:
        args, kw = case_args(c)
        c.ref = REFERENCES[c.kind](*args, **kw)
    return c.ref


@functools.lru_cache(maxsize=None)
def get_case(kind, B, A, with_idx=False, adv_moments=None, mask=None, plant=True, entropy_coef_dev=None):
    """make_case by its parameters, built once per process (the GPU tests and their CPU twins share cases and references)."""
    key = repr((kind, B, A, with_idx, adv_moments, mask, plant))
    c = make_case(np.random.default_rng(zlib.crc32(key.encode())), B, A, 3 * B + 7 if with_idx else None, kind, adv_moments, mask, plant)
    if entropy_coef_dev is not None:
        c.entropy_coef_dev = np.array([entropy_coef_dev], np.float32)
    return c


# --------------------------------------------------------------------------------------------- comparisons ----
def grad_scale(c, ref):
    """Gradients are O(1 / B) (L1, L3) or O(1 / mask count) (L4): they are compared at O(1)."""
    return float(c.B) if c.kind != "ppo_rnn" else max(float(ref[2][9]), 1.0)


def improbable_bound(c, r):
    """The bound for planted row r, whose taken action has log p = lp of about -40.  The kernel forms lp = z[a] - lse and
    then lp - logp_old in float32: three roundings of numbers of size |lp|, each at most half an ulp (|lp| 2^-24), so the
    exponent of the ratio carries up to 1.5 |lp| 2^-23 — taken as 2 |lp| 2^-23 — and the ratio that relative error.  The
    policy gradient of the row, at O(1), is -d(obj)/d(ratio) ratio (onehot - p) with |d(obj)/d(ratio)| <= |adv|, so it is off
    by at most |adv| ratio 2 |lp| 2^-23 on top of the contract's 1e-5."""
    i = r if c.idx is None else int(c.idx[r])
    lnp, _ = _log_softmax64(c.logits[r:r + 1])
    lp = float(lnp[0, c.act[i]])
    ad = float(c.adv[i])
    if c.adv_moments is not None:
        mean, std = norm_constants(c.adv_moments)
        ad = (ad - mean) / (std + 1e-8)
    return TOL + abs(ad) * math.exp(lp - float(c.logp_old[i])) * 2.0 * abs(lp) * 2.0 ** -23


def compare(tag, c, got, per_row=False):
    """got = (dlogits, dvalue, metric sums) of case c against its float64 reference: gradients at O(1) and metric sums as means
    under the contract's 1e-5, the planted improbable-action rows under improbable_bound(); the 0 / 1 sums exactly.
    per_row: every planted row is bounded on its own as well."""
    dz, dv, met = (np.asarray(_np(g), np.float64) for g in got)
    rz, rv, rmet = reference(c)
    assert dz.shape == rz.shape and dv.shape == rv.shape and met.shape == rmet.shape == (N_METRICS[c.kind],)
    s = grad_scale(c, (rz, rv, rmet))
    special = [c.planted[n] for n in ("sat_unlikely",) if n in c.planted]
    rest = np.ones(c.B, bool)
    rest[special] = False
    bounded(f"{tag} dlogits", rel_close(dz[rest] * s, rz[rest] * s), TOL)
    bounded(f"{tag} dvalue", rel_close(dv * s, rv * s), TOL)
    for r in special:
        bounded(f"{tag} dlogits improbable action", rel_close(dz[r] * s, rz[r] * s), improbable_bound(c, r))
    bounded(f"{tag} metric means", rel_close(met / c.B, rmet / c.B), TOL)
    for k in COUNT_METRICS[c.kind]:
        assert met[k] == rmet[k], (tag, k, met[k], rmet[k])
    if per_row:
        for name, r in c.planted.items():
            tol = improbable_bound(c, r) if r in special else TOL
            bounded(f"{tag} planted {name}", max(rel_close(dz[r] * s, rz[r] * s), rel_close(dv[r] * s, rv[r] * s)), tol)
    return dz, dv, met


# ------------------------------------------------------------------------------------------ the test bodies ----
SEAM_SHAPES = [(B, 4) for B in (1, 63, 64, 65, 255, 256, 257, 1025)] + [(B, A) for A in (2, 3, 5, 8) for B in (1, 257)]
GRID_SHAPES = [(B, A) for B in (262145, 262144 + 300, 524293) for A in (3, 4)]
PLANTED_A = [2, 4, 6]
KINDS = ["ppo", "ppo_full", "ppo_rnn"]


def check_seam(run, tag, kind, B, A, with_idx, adv_moments=None):
    c = get_case(kind, B, A, with_idx, adv_moments)
    compare(f"{tag} {kind}", c, run(c))
    return c


def check_planted(run, tag, kind, A, adv_moments=None, entropy_coef_dev=None):
    """B = 257: every designed row on its own.  The planted rows must all be there, and must be what their names say."""
    c = get_case(kind, 257, A, True, adv_moments, entropy_coef_dev=entropy_coef_dev)
    assert list(c.planted) == [n for n, _ in _plants(kind, A)]
    p = c.planted
    dz, dv, _ = compare(f"{tag} {kind}", c, run(c), per_row=True)
    if kind != "ppo":                                                  # rows outside the mask get no gradient at all
        for name in ("erc_below", "erc_above", "corr_mul_zero", "sat_likely", "sat_unlikely"):
            assert not dz[p[name]].any() and dv[p[name]] == 0.0, name
    return c


def check_entropy_coef_dev(run, tag, A):
    """L3 reads its entropy coefficient from device memory when given one: the gradients follow that value (ten times cfg's),
    and differ from the ones cfg's value gives."""
    c = get_case("ppo_full", 257, A, True, entropy_coef_dev=0.1)
    assert float(c.entropy_coef_dev[0]) != c.cfg[5]
    dz, _, _ = compare(f"{tag} ppo_full entropy_coef_dev", c, run(c), per_row=True)
    plain = reference(get_case("ppo_full", 257, A, True))[0]
    assert rel_close(dz * c.B, plain * c.B) > 100 * TOL


def check_full_all_out(run, tag, A=4, B=257):
    """L3, every row outside the entropy band: gradients zero bit for bit, metric 5 == B, the unmasked sums still right."""
    c = get_case("ppo_full", B, A, True, mask="none")
    dz, dv, met = compare(f"{tag} ppo_full all rows out of band", c, run(c))
    assert not dz.any() and not dv.any()
    assert met[5] == B and not met[:4].any()
    assert all(abs(reference(c)[2][k]) > 0 for k in (4, 6, 7, 8))


def check_rnn_empty(run, tag, A=4, B=257):
    """L4, empty mask: masked_mean returns 0 for every term, so no gradient; the masked sums and the count are 0."""
    c = get_case("ppo_rnn", B, A, True, mask="none")
    dz, dv, met = compare(f"{tag} ppo_rnn empty mask", c, run(c))
    assert not dz.any() and not dv.any()
    assert met[9] == 0 and met[5] == B and not met[:4].any()


def check_rnn_one_live(run, tag, row, A=4, B=257):
    """L4, exactly one row in the mask: its gradient is the row's own (1 / count = 1), every other row's is zero."""
    r = row % B
    c = get_case("ppo_rnn", B, A, True, mask=("one", r))
    dz, dv, met = compare(f"{tag} ppo_rnn one live row", c, run(c))
    assert met[9] == 1 and met[5] == B - 1
    others = np.arange(B) != r
    assert not dz[others].any() and not dv[others].any()
    assert dz[r].any() and dv[r] != 0.0
    rz, rv, _ = reference(c)
    assert np.abs(rz[r]).max() > 1e-3                                  # O(1), not O(1 / B)


# ------------------------------------------------------------------------------ gymrl_categorical_sample ----
SAMPLE_SHAPES = [(A, n) for A in range(2, 9) for n in (1, 255, 257)]


@functools.lru_cache(maxsize=None)
def sample_case(A, n):
    """n rows of A logits: row 0 saturated, row 1 (when there is one) with its maximum at columns 0 and A - 1, and Exp(1)
    draws q, redrawn per row until the two largest p / q are at least MARGIN apart (relative) in float64."""
    rng = np.random.default_rng(9000 + 10 * n + A)
    logits = (rng.normal(size=(n, A)) * 1.5).astype(np.float32)
    logits[0] = SAT[:A]
    if n > 1:
        logits[1, 0] = logits[1, A - 1] = np.float32(np.abs(logits[1]).max() + 1.0)
    q = rng.exponential(size=(n, A)).astype(np.float32)
    lnp, H = _log_softmax64(logits)
    p = np.exp(lnp)
    for _ in range(100):
        top = np.sort(p / q.astype(np.float64), axis=1)
        close = top[:, -1] - top[:, -2] < MARGIN * top[:, -1]
        if not close.any():
            break
        q[close] = rng.exponential(size=(int(close.sum()), A)).astype(np.float32)
    top = np.sort(p / q.astype(np.float64), axis=1)
    assert np.all(top[:, -1] - top[:, -2] >= MARGIN * top[:, -1]) and np.all(q > 0)
    return types.SimpleNamespace(A=A, n=n, logits=logits, q=q, lnp=lnp, H=H, pick=np.argmax(p / q.astype(np.float64), axis=1))


def check_sample(sample, tag, A, n):
    """sample(logits, noise_exp, deterministic) -> (action, logp, entropy) against float64 log_softmax."""
    c = sample_case(A, n)
    rows = np.arange(n)
    act, logp, ent = (_np(x) for x in sample(c.logits, None, True))
    want = np.argmax(c.logits, axis=1)                                 # numpy: the first maximum
    assert n == 1 or want[1] == 0
    assert act.shape == (n,) and np.array_equal(act, want)
    bounded(f"{tag} categorical_sample logp", rel_close(logp, c.lnp[rows, want]), TOL)
    bounded(f"{tag} categorical_sample entropy", rel_close(ent, c.H), TOL)
    act, logp, ent = (_np(x) for x in sample(c.logits, c.q, False))
    assert np.array_equal(act, c.pick)
    bounded(f"{tag} categorical_sample logp", rel_close(logp, c.lnp[rows, c.pick]), TOL)
    bounded(f"{tag} categorical_sample entropy", rel_close(ent, c.H), TOL)
