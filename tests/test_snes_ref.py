"""Properties of the separable-NES restatement (tests/snes_ref.py) on the CPU: what gymrl_snes_tell is held to bit for bit on
the GPU (tests/test_snes_kernels_gpu.py) is checked here for being the method — fixed points, symmetries, bounds, and descent on
a quadratic.  eps is es_ref.eps_f64's (libm) rounded to float32: the properties do not depend on the last place of a draw."""
import math

import numpy as np
import pytest

import es_ref
import snes_ref
from optim_ref import F32

CHUNK = 16
SEED = 77


def default_eta_sigma(n):
    return (3.0 + math.log(n)) / (5.0 * math.sqrt(n))


def ulps(a, b):
    """Distance in float32 places between same-signed finite arrays."""
    a, b = np.asarray(a, F32).view(np.int32).astype(np.int64), np.asarray(b, F32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


@pytest.fixture(scope="module")
def eps():
    return snes_ref.eps_matrix(SEED, 3, 24, 10)                      # 24 pairs: a full chunk and a chunk of 8


def test_all_equal_fitness_leaves_mu_and_sigma_as_they_are(eps):
    rng = np.random.default_rng(0)
    mu, sigma = rng.normal(size=10).astype(F32), rng.uniform(0.01, 1.0, size=10).astype(F32)
    for dtype in (np.float32, np.float64):
        returns = np.full((48, 3), -200.0, dtype)
        m, s, w = snes_ref.tell(mu, sigma, returns, eps, 1.0, 0.5, 1e-5, 10.0, CHUNK)
        assert not w.any()
        assert np.array_equal(m.view(np.uint32), mu.view(np.uint32)) and np.array_equal(s.view(np.uint32), sigma.view(np.uint32))


def test_negated_returns_negate_both_steps(eps):
    """w(-R) = -w(R) up to the two float32 roundings of a centred rank (2^-24 absolute), so u_k and s_k negate to within 2^-22 and
    a sum of K terms to within K * max|term factor| * 2^-22 (the float64 accumulation adds nothing visible at that scale)."""
    rng = np.random.default_rng(1)
    returns = rng.normal(size=(48, 2)).astype(F32)
    w_pos, w_neg = es_ref.weights(snes_ref.fitness(returns)), es_ref.weights(snes_ref.fitness(-returns))
    assert np.abs(w_pos + w_neg).max() <= 2.0 ** -24
    mu_p, sg_p = snes_ref.moment_sums(w_pos, eps, CHUNK)
    mu_n, sg_n = snes_ref.moment_sums(w_neg, eps, CHUNK)
    z = eps.astype(np.float64)
    assert np.abs(mu_p).max() > 0.1 and np.abs(sg_p).max() > 0.1
    assert np.abs(mu_p + mu_n).max() <= 24 * np.abs(z).max() * 2.0 ** -22
    assert np.abs(sg_p + sg_n).max() <= 24 * np.abs(z * z - 1.0).max() * 2.0 ** -22
    # through the step: the centre moves the other way, the step sizes by the inverse factor
    mu0, sigma0 = np.zeros(10, F32), np.full(10, 0.5, F32)
    m_p, s_p = snes_ref.step(mu0, sigma0, mu_p, sg_p, 48, 1.0, 0.3, 1e-5, 10.0)
    m_n, s_n = snes_ref.step(mu0, sigma0, mu_n, sg_n, 48, 1.0, 0.3, 1e-5, 10.0)
    assert np.abs(m_p).max() > 1e-3 and np.allclose(m_p, -m_n, rtol=0.0, atol=1e-6)
    assert np.all((s_p > sigma0) == (s_n < sigma0)) and np.allclose(s_p * s_n, sigma0 * sigma0, rtol=1e-5, atol=0.0)


def test_reversing_the_pairs_of_a_chunk_moves_at_most_the_last_place():
    """P = 32 is one chunk: the pairs in reverse order are the same sixteen terms summed the other way round in float64, which
    the float32 results see in their last place at the most."""
    e = snes_ref.eps_matrix(SEED, 0, 16, 12)
    rng = np.random.default_rng(2)
    returns = rng.normal(size=(32, 1))
    mu, sigma = rng.normal(size=12).astype(F32), rng.uniform(0.05, 0.5, size=12).astype(F32)
    order = np.arange(32).reshape(16, 2)[::-1].ravel()               # pair 15 first, each pair's two rows kept in order
    a = snes_ref.tell(mu, sigma, returns, e, 1.0, 0.4, 1e-5, 10.0, CHUNK)
    b = snes_ref.tell(mu, sigma, returns[order], e[::-1], 1.0, 0.4, 1e-5, 10.0, CHUNK)
    assert np.array_equal(a[2][order], b[2])                         # the same ranks, row for row
    assert not np.array_equal(a[0], mu) and not np.array_equal(a[1], sigma)
    assert ulps(a[0], b[0]).max() <= 1 and ulps(a[1], b[1]).max() <= 1


def test_sigma_never_leaves_its_bounds():
    rng = np.random.default_rng(3)
    e = snes_ref.eps_matrix(SEED, 1, 8, 16)
    lo, hi = 1e-3, 2.0
    sigma = np.geomspace(lo, hi, 16).astype(F32)
    mu = np.zeros(16, F32)
    low = high = False
    for trial in range(20):
        returns = rng.normal(size=(16, 1)).astype(F32)
        _, s, _ = snes_ref.tell(mu, sigma, returns, e, 1.0, 40.0, lo, hi, CHUNK)     # eta_sigma = 40: factors far past the bounds
        assert np.all(s >= F32(lo)) and np.all(s <= F32(hi)) and np.isfinite(s).all()
        low, high = low or bool((s == F32(lo)).any()), high or bool((s == F32(hi)).any())
    assert low and high                                              # both clamps were reached, not just approached


def test_descends_a_quadratic():
    """f(x) = -|x - x*|^2, n = 8, P = 32, 200 generations at the learner's defaults (eta_mu = 1, the paper's eta_sigma)."""
    n, P = 8, 32
    rng = np.random.default_rng(4)
    target = rng.normal(size=n) * 2.0
    mu, sigma = np.zeros(n, F32), np.full(n, 0.5, F32)
    start = float(np.linalg.norm(mu - target))
    for generation in range(200):
        e = snes_ref.eps_matrix(SEED, generation, P // 2, n)
        pop = snes_ref.perturb(mu, sigma, e)
        returns = -((pop.astype(np.float64) - target) ** 2).sum(axis=1, keepdims=True)
        mu, sigma, _ = snes_ref.tell(mu, sigma, returns, e, 1.0, default_eta_sigma(n), 1e-5, 5.0, CHUNK)
    end = float(np.linalg.norm(mu - target))
    print(f"|mu - x*|: {start:.4f} -> {end:.4f}; sigma in [{sigma.min():.2e}, {sigma.max():.2e}]")
    assert end < start
