"""The numpy restatement of the evolution-strategies stages (tests/es_ref.py) held to its own properties (CPU)."""
import math

import numpy as np
import pytest

import es_ref
from optim_ref import F32


def test_philox_known_answers():
    """Random123's published vectors for Philox4x32-10."""
    assert es_ref.philox4x32(0, 0, 0, 0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    ones = 0xFFFFFFFF
    assert es_ref.philox4x32((ones << 32) | ones, ones, ones, ones, ones) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert es_ref.philox4x32((0x299F31D0 << 32) | 0xA4093822, 0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_draw_map_counter_words():
    assert es_ref.eps_words(0, 0, 0) == (0, 0, 0, 0x70000000, 0)
    assert es_ref.eps_words(5, 7, 4 * 9 + 3) == (9, 7, 5, 0x70000000, 3)
    assert es_ref.eps_words((3 << 32) | 11, 2, 6) == (1, 2, 11, 0x70000003, 2)
    assert es_ref.eps_words(1 << 60, 0, 0)[3] == 0x70000000          # the fold keeps 28 high bits: generations below 2^60
    # four elements share a call, the next four take the next one
    assert len({es_ref.eps_words(0, 1, i)[:4] for i in range(4)}) == 1
    assert es_ref.eps_words(0, 1, 4)[0] == 1


def test_eps_f64_is_standard_normal_sized():
    x = np.array([es_ref.eps_f64(42, 3, k, i) for k in range(8) for i in range(512)])
    n = x.size
    assert abs(x.mean()) < 5.0 / math.sqrt(n) and abs(x.var() - 1.0) < 5.0 * math.sqrt(2.0 / n)
    assert es_ref.eps_f64(42, 3, 0, 0) != es_ref.eps_f64(42, 4, 0, 0) != es_ref.eps_f64(43, 4, 0, 0)


def test_perturb_is_mirrored_and_two_roundings():
    rng = np.random.default_rng(0)
    theta, eps = rng.normal(size=37).astype(F32), rng.normal(size=(3, 37)).astype(F32)
    out = es_ref.perturb(theta, 0.1, eps)
    assert out.shape == (6, 37) and out.dtype == F32
    s = F32(0.1) * eps
    assert np.array_equal(out[0::2], theta + s) and np.array_equal(out[1::2], theta - s)
    fused = (theta.astype(np.float64) + np.float64(F32(0.1)) * eps.astype(np.float64)).astype(F32)      # one rounding
    assert not np.array_equal(out[0::2], fused)


def test_fitness_is_the_float64_row_sum_in_order():
    r = np.array([[1e8, 1.0, -1e8], [1.0, 2.0, 3.0]], F32)
    assert es_ref.fitness(r).tolist() == [1.0, 6.0]                  # float32 accumulation would lose the 1
    assert es_ref.fitness(r).dtype == np.float64


@pytest.mark.parametrize("P", [2, 4, 6, 34, 130])
def test_weights_sum_to_zero_and_are_antisymmetric(P):
    rng = np.random.default_rng(P)
    F = rng.normal(size=P)
    w = es_ref.weights(F)
    # the quotient in [0, 1] is rounded once (<= 2^-25), the subtraction of 0.5 once more below 0.25 (<= 2^-26): the exact
    # centred ranks sum to 0 and are antisymmetric, the float32 ones to within those roundings
    assert w.dtype == F32 and abs(w.astype(np.float64).sum()) <= P * 2.0 ** -24
    assert w.min() == F32(-0.5) and w.max() == F32(0.5)
    flipped = es_ref.weights(-F)                                     # reversing the order flips every weight
    assert np.abs(flipped.astype(np.float64) + w.astype(np.float64)).max() <= 2.0 ** -24
    assert np.array_equal(np.argsort(flipped), np.argsort(-w))
    order = np.argsort(F)
    assert np.array_equal(w[order], (np.arange(P) * 2).astype(F32) / F32(2 * (P - 1)) - F32(0.5))


def test_ties_share_a_weight_and_all_equal_is_zero():
    F = np.array([3.0, 1.0, 3.0, 2.0, 3.0, 1.0])
    w = es_ref.weights(F)
    assert w[0] == w[2] == w[4] and w[1] == w[5]
    assert abs(w.astype(np.float64).sum()) <= 6 * 2.0 ** -24
    # ranks 0..5: the ones share (0 + 1) / 2, the two sits at 2, the threes share 4
    assert np.array_equal(w, np.array([4, 0.5, 4, 2, 4, 0.5], F32) / F32(5) - F32(0.5))
    assert np.array_equal(es_ref.weights(np.full(8, -200.0)), np.zeros(8, F32))
    assert np.array_equal(es_ref.weights(np.array([1.0, 1.0])), np.zeros(2, F32))


def test_population_of_two():
    assert es_ref.weights(np.array([1.0, 2.0])).tolist() == [-0.5, 0.5]
    eps = np.array([[1.0, -2.0, 0.5]], F32)
    g = es_ref.search_gradient(es_ref.weights(np.array([1.0, 2.0])), eps, 0.5, 16)
    assert g.tolist() == [1.0, -2.0, 0.5]                            # -(1 / (2 * 0.5)) * (-0.5 - 0.5) * eps: descend = away from the better -eps
    g = es_ref.search_gradient(es_ref.weights(np.array([2.0, 1.0])), eps, 0.5, 16)
    assert g.tolist() == [-1.0, 2.0, -0.5]


def test_search_gradient_order_is_chunked():
    """The chunk size is part of the result: a float64 sum in another order differs in the last bits, and the restatement
    follows the stated one."""
    rng = np.random.default_rng(3)
    K, n = 53, 257
    eps = rng.normal(size=(K, n)).astype(F32)
    w = es_ref.weights(rng.normal(size=2 * K))
    u = (w[0::2] - w[1::2]).astype(np.float64)
    for chunk in (1, 16, 64):
        S = np.zeros(n)
        for c0 in range(0, K, chunk):
            acc = np.zeros(n)
            for k in range(c0, min(K, c0 + chunk)):
                acc = acc + u[k] * eps[k].astype(np.float64)
            S = S + acc
        want = (-(1.0 / (2 * K * float(F32(0.1)))) * S).astype(F32)
        assert np.array_equal(es_ref.search_gradient(w, eps, 0.1, chunk), want)
    exact = -(1.0 / (2 * K * float(F32(0.1)))) * (u[:, None] * eps.astype(np.float64)).sum(axis=0)
    assert np.allclose(es_ref.search_gradient(w, eps, 0.1, 16), exact, rtol=1e-6, atol=1e-7)
    assert np.array_equal(es_ref.search_gradient(np.zeros(2 * K, F32), eps, 0.1, 16), np.zeros(n, F32))


def test_tell_moves_the_centre_towards_the_better_half():
    rng = np.random.default_rng(4)
    n, K = 9, 8
    theta, eps = np.zeros(n, F32), rng.normal(size=(K, n)).astype(F32)
    target = rng.normal(size=n).astype(F32)
    pop = es_ref.perturb(theta, 0.1, eps)
    returns = -((pop - target) ** 2).sum(axis=1, keepdims=True).astype(F32)
    new, m, v, w, g = es_ref.tell(theta, np.zeros(n, F32), np.zeros(n, F32), returns, eps, 0.1, 0.05, 1, 16)
    assert np.dot(new - theta, target) > 0.0 and new.dtype == F32
    same, _, _, w0, g0 = es_ref.tell(theta, np.zeros(n, F32), np.zeros(n, F32), np.full((2 * K, 1), -200.0, F32), eps, 0.1, 0.05, 1, 16)
    assert np.array_equal(same.view(np.uint32), theta.view(np.uint32)) and not w0.any() and not g0.any()
