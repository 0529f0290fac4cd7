"""Plain numpy references of the optimiser step (gymrl_amd/csrc/optim.hip), shared by tests/test_optim_ref.py (CPU) and
tests/test_optim_edges_gpu.py.  No torch, no autograd.

    adam_f64   the definition in float64: clip_grad_norm_'s rule, the optional clamp, torch.optim.Adam with its bias
               corrections, the optional zero_grad and Polyak target.  What the kernel is held to within a tolerance.
    adam_f32   adam_one of optim.hip, expression by expression in np.float32, taking the three step scalars as arguments
               so that the lr_dev and bias_dev forms can be handed exactly the scalars the kernel derives.  The library
               is built with -ffp-contract=off, numpy rounds every float32 operation once: the same bits.

Both state the rule for a gradient that is not finite the way torch does: a NaN norm makes the clip coefficient NaN
(torch.clamp(coef, max=1) keeps NaN), and clamping a NaN element leaves it NaN (Tensor.clamp_)."""
import math

import numpy as np

F32 = np.float32
BETAS = (0.9, 0.999)


def mixed_grad(rng, n, phase=0):
    """Unit normals in alternating blocks of 256 elements scaled by 3.0 and 0.01 (the two magnitudes of
    tests/golden/make_golden.py gen_adam_multi, here side by side in one vector); `phase` swaps the blocks."""
    mag = np.where(((np.arange(n) >> 8) + phase) & 1, 0.01, 3.0)
    return (rng.normal(size=n) * mag).astype(F32)


def sqnorm_fsum(g, grad_scale):
    """The exact sum of squares of the float32 products g * grad_scale (the scaling is rounded to float32 first, as
    the kernel's input to the norm is; the squares of float32 are exact in float64; fsum adds them without error)."""
    a = (np.asarray(g, F32) * F32(grad_scale)).astype(np.float64)
    return math.fsum(a * a)


def host_scalars(lr, beta1, beta2, step):
    """(float)(lr / bc1), (float)(1 / bc1), (float)sqrt(bc2) in double arithmetic: gymrl_adam_bias."""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return F32(lr / bc1), F32(1.0 / bc1), F32(math.sqrt(bc2))


def clip_scale_f32(sqnorm, max_norm):
    """The clip coefficient as adam_kernel derives it from the float64 squared norm: float32 from the root onwards."""
    with np.errstate(all="ignore"):
        total = F32(np.sqrt(np.float64(sqnorm)))
        coef = F32(max_norm) / (total + F32(1e-6))
    return F32(1.0) if coef >= F32(1.0) else coef          # a NaN coefficient is not >= 1: it stays NaN


def adam_f32(p, g, m, v, beta1, beta2, eps, step_size, bc2_sqrt, scale, grad_scale=1.0, clamp_abs=0.0, zero_grad=True):
    """One step of adam_one over float32 arrays; returns new (p, g, m, v)."""
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    omb1, b2, omb2, e = F32(1.0 - beta1), F32(beta2), F32(1.0 - beta2), F32(eps)
    step_size, bc2_sqrt, scale, c = F32(step_size), F32(bc2_sqrt), F32(scale), F32(clamp_abs)
    with np.errstate(all="ignore"):
        gg = g * F32(grad_scale)
        gg = gg * scale
        if c > 0:
            gg = np.where(np.isnan(gg), gg, np.minimum(np.maximum(gg, -c), c))
        m = m + (gg - m) * omb1
        v = v * b2 + omb2 * gg * gg
        denom = np.sqrt(v) / bc2_sqrt + e
        p = p - step_size * (m / denom)
    assert p.dtype == m.dtype == v.dtype == F32
    return p, (np.zeros_like(g) if zero_grad else g.copy()), m, v


def adam_f64(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, max_norm=0.0, clamp_abs=0.0, zero_grad=True,
             target=None, tau=0.0):
    """One step in float64 from float32 (or already float64) state; returns new (p, g, m, v, target), target None when
    none was given.  grad_scale, max_norm and clamp_abs are float32 arguments of the kernel: their float32 values are
    the inputs.  The clip is by the norm of the scaled gradient and comes before the clamp, as in adam_one."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        gg = g * float(F32(grad_scale))
        if max_norm > 0:
            coef = float(F32(max_norm)) / (np.sqrt(np.sum(gg * gg)) + 1e-6)
            gg = gg * (1.0 if coef >= 1.0 else coef)               # NaN stays NaN
        if clamp_abs > 0:
            c = float(F32(clamp_abs))
            gg = np.where(np.isnan(gg), gg, np.clip(gg, -c, c))
        m = beta1 * m + (1.0 - beta1) * gg
        v = beta2 * v + (1.0 - beta2) * gg * gg
        denom = np.sqrt(v) / math.sqrt(1.0 - beta2 ** step) + eps
        p = p - lr / (1.0 - beta1 ** step) * (m / denom)
        if target is not None:
            target = tau * p + (1.0 - tau) * np.asarray(target, np.float64)
    return p, (np.zeros_like(g) if zero_grad else g.copy()), m, v, target
