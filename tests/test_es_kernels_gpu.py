"""The evolution-strategies kernels (gymrl_amd/csrc/es.hip) on the GPU: the noise against the normal law and its draw map,
the population and the search gradient bit for bit against the numpy restatement (tests/es_ref.py) on the GPU's own noise."""
import math

import numpy as np
import pytest

import es_ref
from optim_ref import F32
from test_rng_distributions import Z2

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = 20240531
SIGMA = 0.1
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def dev():
    from gymrl_amd import ops
    assert torch.cuda.is_available() and ops.device_ok()
    return torch.device("cuda")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


_EPS = {}


def gpu_eps(dev, n, K, generation=3):
    """The kernels' own eps f32[K, n] at (SEED, generation): drawn once per (n, generation) at the widest K asked for so far."""
    from gymrl_amd import ops
    got = _EPS.get((n, generation))
    if got is None or got.shape[0] < K:
        got = _EPS[(n, generation)] = ops.es_noise(n, 0, K, SEED, generation, dev).cpu().numpy()
    return got[:K]


# ------------------------------------------------------------------ noise ---
def test_noise_has_the_normal_moments_and_no_lag_one_correlation(dev):
    """2^20 draws: 16 pairs x 65536 elements.  The sampling sd of the mean, variance, skewness and excess kurtosis of N normal
    draws are sqrt(1 / N), sqrt(2 / N), sqrt(6 / N), sqrt(24 / N), of a correlation sqrt(1 / N); the two-sided 1e-6 quantile
    (about 4.9 sd) is tests/test_rng_distributions.py's rule."""
    from gymrl_amd import ops
    K, n = 16, 65536
    x = ops.es_noise(n, 0, K, SEED, 0, dev).cpu().numpy().astype(np.float64)
    N = x.size
    assert N == 1 << 20 and np.isfinite(x).all()
    m, v = x.mean(), x.var()
    z = (x - m) / math.sqrt(v)
    skew, kurt = (z ** 3).mean(), (z ** 4).mean() - 3.0
    print(f"mean {m:.3e} variance-1 {v - 1:.3e} skew {skew:.3e} excess kurtosis {kurt:.3e}")
    assert abs(m) < Z2 * math.sqrt(1.0 / N)
    assert abs(v - 1.0) < Z2 * math.sqrt(2.0 / N)
    assert abs(skew) < Z2 * math.sqrt(6.0 / N)
    assert abs(kurt) < Z2 * math.sqrt(24.0 / N)
    along_i = float(np.corrcoef(x[:, :-1].ravel(), x[:, 1:].ravel())[0, 1])
    across_k = float(np.corrcoef(x[:-1].ravel(), x[1:].ravel())[0, 1])
    print(f"lag-1 correlation along i {along_i:.3e} across k {across_k:.3e}")
    assert abs(along_i) < Z2 / math.sqrt(K * (n - 1))
    assert abs(across_k) < Z2 / math.sqrt((K - 1) * n)
    # the four outputs of a call, each against the next: the cosine / sine of one pair and the two pairs of a call
    quad = x.reshape(K, n // 4, 4)
    for a, b in ((0, 1), (1, 2), (2, 3), (0, 2)):
        r = float(np.corrcoef(quad[:, :, a].ravel(), quad[:, :, b].ravel())[0, 1])
        assert abs(r) < Z2 / math.sqrt(K * n / 4), (a, b, r)


def test_noise_follows_the_documented_draw_map(dev):
    """eps against the map of include/gymrl.h in float64 under libm.  The kernel's float32 chain: the angle 2 pi u < 6.29 is rounded
    to 2^-22 and so are its sine and cosine arguments (|d sin| <= 4.8e-7), the library's logf and sincosf are good to a few
    ulp (1e-6 relative on rho <= 5.8): 2e-5 absolute covers both with room, and is far below any wrong word or quadrant."""
    from gymrl_amd import ops
    n, k0, K = 23, 5, 3
    for generation in (0, 7, (5 << 32) | 9):
        got = ops.es_noise(n, k0, K, SEED, generation, dev).cpu().numpy()
        want = np.array([[es_ref.eps_f64(SEED, generation, k0 + r, i) for i in range(n)] for r in range(K)])
        assert np.abs(got - want).max() < 2e-5, generation


def test_noise_rows_differ_by_pair_generation_and_seed_and_repeat_bit_for_bit(dev):
    from gymrl_amd import ops
    n, K = 1027, 6
    base = ops.es_noise(n, 0, K, SEED, 1, dev).cpu().numpy()
    assert np.array_equal(bits(base), bits(ops.es_noise(n, 0, K, SEED, 1, dev).cpu().numpy()))
    for a in range(K):
        for b in range(a + 1, K):
            assert (base[a] != base[b]).mean() > 0.99, (a, b)
    for generation in (0, 2, 1 << 32, (1 << 32) | 1, 3 << 40):
        other = ops.es_noise(n, 0, K, SEED, generation, dev).cpu().numpy()
        assert (other != base).mean() > 0.99, generation
    assert (ops.es_noise(n, 0, K, SEED, (1 << 32) | 1, dev).cpu().numpy() != ops.es_noise(n, 0, K, SEED, (2 << 32) | 1, dev).cpu().numpy()).mean() > 0.99
    assert (ops.es_noise(n, 0, K, SEED + 1, 1, dev).cpu().numpy() != base).mean() > 0.99
    # a window that starts at a later pair is the same rows
    assert np.array_equal(bits(ops.es_noise(n, 2, 3, SEED, 1, dev).cpu().numpy()), bits(base[2:5]))
    assert np.array_equal(bits(ops.es_noise(n, 4095, 1, SEED, 1, dev).cpu().numpy()), bits(ops.es_noise(n, 4090, 6, SEED, 1, dev).cpu().numpy()[5:]))
    # a narrower row is a prefix: element i does not depend on n
    assert np.array_equal(bits(ops.es_noise(5, 0, K, SEED, 1, dev).cpu().numpy()), bits(base[:, :5]))


# ---------------------------------------------------------------- perturb ---
@pytest.mark.parametrize("n", [1, 5, 1027, 70001])
def test_perturb_matches_the_restatement_bit_for_bit(dev, n):
    from gymrl_amd import ops
    rng = np.random.default_rng(n)
    theta = rng.normal(size=n).astype(F32)
    theta_d = torch.from_numpy(theta).to(dev)
    for P in (2, 6, 130):
        eps = gpu_eps(dev, n, 65)[:P // 2]
        want = es_ref.perturb(theta, SIGMA, eps)
        for stride in (ops.es_stride(n), ops.es_stride(n + 8)):     # n + 8, on the next multiple of four (the stride rule)
            assert stride >= n and stride % 4 == 0
            stack = torch.full((P, stride), SENTINEL, dtype=torch.float32, device=dev)
            out = ops.es_perturb(theta_d, SIGMA, SEED, 3, stack)
            assert out is stack
            got = stack.cpu().numpy()
            assert np.array_equal(bits(got[:, :n]), bits(want)), (P, stride)
            assert (got[:, n:] == SENTINEL).all(), (P, stride)
    assert np.array_equal(theta_d.cpu().numpy(), theta)


def test_perturb_takes_the_strides_the_issue_names(dev):
    """stride = ceil4(n) and stride = n + 8 where that is a multiple of four; otherwise the next one above n + 4."""
    from gymrl_amd import ops
    assert ops.es_stride(70001) == 70004 and ops.es_stride(1027) == 1028
    theta = torch.zeros(8, device=dev)
    stack = torch.full((2, 16), SENTINEL, device=dev)                # n + 8 exactly
    ops.es_perturb(theta, SIGMA, SEED, 0, stack)
    eps = ops.es_noise(8, 0, 1, SEED, 0, dev)
    assert torch.equal(stack[0, :8], SIGMA * eps[0]) and torch.equal(stack[1, :8], -(SIGMA * eps[0]))
    assert (stack[:, 8:] == SENTINEL).all()


# -------------------------------------------------------------- shape_grad ---
def _returns(kind, rng, P, E):
    if kind == "ties":
        return rng.integers(0, 4, size=(P, E)).astype(F32)
    if kind == "equal":
        return np.full((P, E), -200.0, F32)
    return (rng.normal(size=(P, E)) * 1e30).astype(F32)              # huge spread: only the order matters


def _check_shape_grad(dev, P, n, E, kind, rng, generation=3):
    from gymrl_amd import ops
    returns = _returns(kind, rng, P, E)
    eps = gpu_eps(dev, n, P // 2, generation)
    grad = torch.full((n,), SENTINEL, dtype=torch.float32, device=dev)
    g, w = ops.es_shape_grad(torch.from_numpy(returns).to(dev), SIGMA, SEED, generation, grad)
    assert g is grad
    w_want = es_ref.weights(es_ref.fitness(returns))
    g_want = es_ref.search_gradient(w_want, eps, SIGMA, ops.ES_PAIR_CHUNK)
    what = (P, n, E, kind)
    assert np.array_equal(bits(w.cpu().numpy()), bits(w_want)), what
    assert np.array_equal(bits(g.cpu().numpy()), bits(g_want)), what
    if kind == "equal":
        assert not w.cpu().numpy().any() and not g.cpu().numpy().any(), what
    else:
        assert g.cpu().numpy().any(), what


@pytest.mark.parametrize("n", [1, 5, 70001])
@pytest.mark.parametrize("pairs", ["1", "C", "C+1", "3C+5"])
def test_shape_grad_matches_the_restatement_bit_for_bit(dev, pairs, n):
    from gymrl_amd import ops
    C = ops.ES_PAIR_CHUNK
    P = 2 * {"1": 1, "C": C, "C+1": C + 1, "3C+5": 3 * C + 5}[pairs]
    rng = np.random.default_rng(1000 * P + n)
    for E in (1, 3):
        for kind in ("ties", "equal", "huge"):
            if P == 2 and kind == "ties":
                _check_shape_grad(dev, P, n, E, "huge", rng)             # two policies: a tie IS all-equal
                continue
            _check_shape_grad(dev, P, n, E, kind, rng)


@pytest.mark.parametrize("P,n", [(256, 1027), (258, 1027), (258, 5), (8192, 64)])
def test_shape_grad_on_both_sides_of_the_one_launch_threshold_and_at_the_cap(dev, P, n):
    """Up to 256 policies every gradient workgroup counts the ranks itself; above, a rank launch runs first.  8192 is the cap:
    256 chunk slots, one quad of elements per workgroup."""
    rng = np.random.default_rng(P + n)
    for kind in ("ties", "huge", "equal"):
        _check_shape_grad(dev, P, n, 1 if P == 8192 else 3, kind, rng, generation=(1 << 32) | 5)


def test_shape_grad_reads_the_fitness_in_float64(dev):
    """Rows whose float32 running sums tie and whose float64 sums do not: the ranks are the float64 ones."""
    from gymrl_amd import ops
    returns = np.array([[1e8, 1.0, -1e8], [1e8, 2.0, -1e8], [0.0, 0.5, 0.0], [0.0, 3.0, 0.0]], F32)
    grad = torch.zeros(5, device=dev)
    _, w = ops.es_shape_grad(torch.from_numpy(returns).to(dev), SIGMA, SEED, 0, grad)
    assert np.array_equal(w.cpu().numpy(), es_ref.weights(np.array([1.0, 2.0, 0.5, 3.0])))
