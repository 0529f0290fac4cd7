"""Plain numpy restatement of the evolution-strategies stages (gymrl_amd/csrc/es.hip, include/gymrl.h), shared by
tests/test_es_ref.py (CPU) and the GPU tests.  No torch.

    philox4x32 / eps_words   Philox4x32-10 in Python integers and the counter words of eps(seed, generation, k, i)
    eps_f64                  the draw map in float64 (libm's log / sin / cos): what the kernel's float32 eps is close to
    perturb                  rows 2k / 2k + 1 = theta +- sigma * eps_k, one float32 product and one float32 sum each
    fitness / weights        float64 row sums in ascending e; centred ranks by counting, ties averaged
    search_gradient          the chunked float64 sum, in the order the header states
    adam                     tests/optim_ref.py's adam_f32 under the host's step scalars: FusedAdam without clamp or clip

The library is built with -ffp-contract=off and numpy rounds every operation once, so perturb, weights and search_gradient
agree with the kernels bit for bit when they are handed the kernels' own eps."""
import math

import numpy as np

from optim_ref import BETAS, F32, adam_f32, host_scalars

RNG_ES = 0x70000000
M32 = 0xFFFFFFFF


def philox4x32(key, c0, c1, c2, c3):
    """Philox4x32-10 -> four 32-bit words (csrc/gymrl_device.hpp philox4x32)."""
    k0, k1 = key & M32, (key >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def eps_words(generation, k, i):
    """(c0, c1, c2, c3, which of the four normals) of element i of pair k."""
    return i >> 2, k, generation & M32, RNG_ES | ((generation >> 32) & 0x0FFFFFFF), i & 3


def eps_f64(seed, generation, k, i):
    c0, c1, c2, c3, which = eps_words(generation, k, i)
    r = philox4x32(seed, c0, c1, c2, c3)
    a, b = (r[0], r[1]) if which < 2 else (r[2], r[3])
    rho = math.sqrt(-2.0 * math.log(((a >> 8) + 1) * 2.0 ** -24))
    ang = 2.0 * math.pi * ((b >> 8) * 2.0 ** -24)
    return rho * (math.cos(ang) if which % 2 == 0 else math.sin(ang))


def perturb(theta, sigma, eps):
    """theta f32[n], eps f32[K, n] -> f32[2K, n]."""
    theta, eps = np.asarray(theta, F32), np.asarray(eps, F32)
    s = F32(sigma) * eps
    out = np.empty((2 * eps.shape[0], theta.size), F32)
    out[0::2], out[1::2] = theta + s, theta - s
    return out


def fitness(returns):
    """f32[P, E] -> f64[P]: the sum of each row in ascending e."""
    returns = np.asarray(returns, F32)
    F = np.zeros(returns.shape[0], np.float64)
    for e in range(returns.shape[1]):
        F = F + returns[:, e].astype(np.float64)
    return F


def weights(F):
    """Centred ranks of f64[P], ties averaged: (float)(2 less + equal - 1) / (float)(2 (P - 1)) - 0.5f."""
    F = np.asarray(F, np.float64)
    P = F.size
    less = (F[None, :] < F[:, None]).sum(axis=1)
    equal = (F[None, :] == F[:, None]).sum(axis=1)
    return (2 * less + equal - 1).astype(F32) / F32(2 * (P - 1)) - F32(0.5)


def search_gradient(w, eps, sigma, chunk):
    """w f32[P], eps f32[P / 2, n] -> f32[n]: -(1 / (P sigma)) sum_k (w_2k - w_2k+1) eps_k, pairs in consecutive chunks of `chunk`,
    a chunk from 0.0 in ascending k, the chunk sums onto 0.0 in ascending chunk order, all in float64."""
    w, eps = np.asarray(w, F32), np.asarray(eps, F32)
    P, K = w.size, eps.shape[0]
    assert P == 2 * K
    u = (w[0::2] - w[1::2]).astype(np.float64)
    S = np.zeros(eps.shape[1], np.float64)
    for c0 in range(0, K, chunk):
        acc = np.zeros(eps.shape[1], np.float64)
        for k in range(c0, min(K, c0 + chunk)):
            acc = acc + u[k] * eps[k].astype(np.float64)
        S = S + acc
    coef = -(1.0 / (float(P) * float(F32(sigma))))
    return (coef * S).astype(F32)


def adam(p, g, m, v, lr, step, betas=BETAS, eps=1e-8):
    """One FusedAdam step (no clamp, no clip) -> new (p, m, v), float32 bit for bit."""
    ss, _, bc2s = host_scalars(lr, betas[0], betas[1], step)
    p, _, m, v = adam_f32(p, g, m, v, betas[0], betas[1], eps, ss, bc2s, 1.0)
    return p, m, v


def tell(theta, m, v, returns, eps, sigma, lr, step, chunk):
    """OpenAIES.tell on the GPU's own eps -> (theta, m, v, weights, grad)."""
    w = weights(fitness(returns))
    g = search_gradient(w, eps, sigma, chunk)
    theta, m, v = adam(theta, g, m, v, lr, step)
    return theta, m, v, w, g
