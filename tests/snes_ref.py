"""Plain numpy restatement of the separable-NES stages (gymrl_amd/csrc/es.hip, include/gymrl.h), shared by
tests/test_snes_ref.py (CPU) and the GPU tests.  Built on tests/es_ref.py's Philox / eps / fitness / weights.  No torch.

    perturb        rows 2k / 2k + 1 = mu +- sigma * eps_k with sigma f32[n], one float32 product and one float32 sum each
    fitness        float64 row sums in ascending e, of float32 returns (each term widened) or of float64 returns
    moment_sums    Smu and Ssg, the chunked float64 sums in the order the header states
    tell           weights, the sums and the in-place step -> (mu, sigma, weights)

expf is the built oracle library's orc_expf (the bits of det_expf).  The library is built with -ffp-contract=off and numpy rounds
every operation once, so every stage agrees with the kernels bit for bit when it is handed the kernels' own eps."""
import numpy as np

import es_ref
from optim_ref import F32


def expf(x):
    from oracle import oracle
    return oracle.expf(np.asarray(x, F32))


def perturb(mu, sigma, eps):
    """mu, sigma f32[n], eps f32[K, n] -> f32[2K, n]."""
    mu, sigma, eps = np.asarray(mu, F32), np.asarray(sigma, F32), np.asarray(eps, F32)
    s = sigma[None, :] * eps
    out = np.empty((2 * eps.shape[0], mu.size), F32)
    out[0::2], out[1::2] = mu + s, mu - s
    return out


def fitness(returns):
    """[P, E] float32 or float64 -> f64[P]: the sum of each row in ascending e, every term (double)returns[p][e]."""
    returns = np.asarray(returns)
    assert returns.dtype in (np.float32, np.float64), returns.dtype
    F = np.zeros(returns.shape[0], np.float64)
    for e in range(returns.shape[1]):
        F = F + returns[:, e].astype(np.float64)
    return F


def moment_sums(w, eps, chunk):
    """w f32[P], eps f32[P / 2, n] -> (Smu, Ssg) f64[n]: sum_k u_k eps_k and sum_k s_k (eps_k^2 - 1) with u_k = w_2k - w_2k+1 and
    s_k = w_2k + w_2k+1 in float32; pairs in consecutive chunks of `chunk`, a chunk from 0.0 in ascending k, the chunk sums onto
    0.0 in ascending chunk order, all in float64."""
    w, eps = np.asarray(w, F32), np.asarray(eps, F32)
    K, n = eps.shape
    assert w.size == 2 * K
    u, s = (w[0::2] - w[1::2]).astype(np.float64), (w[0::2] + w[1::2]).astype(np.float64)
    Smu, Ssg = np.zeros(n, np.float64), np.zeros(n, np.float64)
    for c0 in range(0, K, chunk):
        am, asg = np.zeros(n, np.float64), np.zeros(n, np.float64)
        for k in range(c0, min(K, c0 + chunk)):
            z = eps[k].astype(np.float64)
            am = am + u[k] * z
            asg = asg + s[k] * (z * z - 1.0)
        Smu, Ssg = Smu + am, Ssg + asg
    return Smu, Ssg


def step(mu, sigma, Smu, Ssg, P, eta_mu, eta_sigma, sigma_min, sigma_max):
    """The in-place step of gymrl_snes_tell -> (mu, sigma) float32; eta_* and the bounds as the float32 fields carry them."""
    mu, sigma = np.asarray(mu, F32), np.asarray(sigma, F32)
    c = 4.0 / float(P)
    new_mu = (mu.astype(np.float64) + float(F32(eta_mu)) * (sigma.astype(np.float64) * (c * Smu))).astype(F32)
    v = sigma * expf((0.5 * float(F32(eta_sigma)) * (c * Ssg)).astype(F32))
    v = np.where(v < F32(sigma_min), F32(sigma_min), v)
    v = np.where(v > F32(sigma_max), F32(sigma_max), v)
    return new_mu, v.astype(F32)


def tell(mu, sigma, returns, eps, eta_mu, eta_sigma, sigma_min, sigma_max, chunk):
    """gymrl_snes_tell on the GPU's own eps -> (mu, sigma, weights)."""
    w = es_ref.weights(fitness(returns))
    Smu, Ssg = moment_sums(w, eps, chunk)
    mu, sigma = step(mu, sigma, Smu, Ssg, w.size, eta_mu, eta_sigma, sigma_min, sigma_max)
    return mu, sigma, w


def eps_matrix(seed, generation, K, n):
    """f32[K, n] of es_ref.eps_f64: libm's draws, for CPU-only tests (the GPU tests take the kernels' own eps)."""
    return np.array([[es_ref.eps_f64(seed, generation, k, i) for i in range(n)] for k in range(K)], F32)
