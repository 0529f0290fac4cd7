"""The separable-NES kernels (gymrl_amd/csrc/es.hip: gymrl_snes_perturb, gymrl_snes_tell) on the GPU: the population, the
weights, the centre and the step sizes bit for bit against the numpy restatement (tests/snes_ref.py) on the GPU's own noise,
under float32 and float64 returns, on both sides of the one-launch threshold and at the cap."""
import math

import numpy as np
import pytest

import es_ref
import snes_ref
from optim_ref import F32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = 20240917
SENTINEL = 12345.0
LO, HI = 1e-5, 1.0
# (P, n), E: one pair and a scalar tail; exactly one chunk; 17 pairs (a second chunk holding one); the top of the fused rank
# path; the first size with the separate rank launch; the cap (256 chunk slots)
SHAPES = [(2, 5, 1), (32, 4, 1), (34, 68, 3), (256, 4672, 3), (258, 4672, 3), (8192, 8, 1)]


@pytest.fixture(scope="module")
def dev():
    from gymrl_amd import ops
    assert torch.cuda.is_available() and ops.device_ok()
    return torch.device("cuda")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def generation_of(P):
    return (1 << 32) | 5 if P >= 256 else 3


_EPS = {}


def gpu_eps(dev, P, n):
    """The kernels' own eps f32[P / 2, n] at (SEED, generation_of(P)), drawn once per shape."""
    from gymrl_amd import ops
    key = (P, n)
    if key not in _EPS:
        _EPS[key] = ops.es_noise(n, 0, P // 2, SEED, generation_of(P), dev).cpu().numpy()
    return _EPS[key]


def centre(P, n):
    rng = np.random.default_rng(7 * P + n)
    return rng.normal(size=n).astype(F32), rng.uniform(0.05, 0.2, size=n).astype(F32)


def eta_sigma_of(n):
    return (3.0 + math.log(n)) / (5.0 * math.sqrt(n))


def run_tell(dev, returns, mu, sigma, P, eta_sigma, lo=LO, hi=HI):
    """-> (mu, sigma, weights) of one gymrl_snes_tell on copies of mu / sigma, as numpy arrays."""
    from gymrl_amd import ops
    mu_d, sigma_d = torch.from_numpy(mu.copy()).to(dev), torch.from_numpy(sigma.copy()).to(dev)
    w = ops.snes_tell(torch.from_numpy(returns).to(dev), mu_d, sigma_d, SEED, generation_of(P), 1.0, eta_sigma, lo, hi)
    return mu_d.cpu().numpy(), sigma_d.cpu().numpy(), w.cpu().numpy()


def check_tell(dev, returns, P, n, mu, sigma, eta_sigma, lo=LO, hi=HI):
    got = run_tell(dev, returns, mu, sigma, P, eta_sigma, lo, hi)
    want = snes_ref.tell(mu, sigma, returns, gpu_eps(dev, P, n), 1.0, eta_sigma, lo, hi, 16)
    what = (P, n, returns.dtype)
    assert np.array_equal(bits(got[2]), bits(want[2])), what
    assert np.array_equal(bits(got[0]), bits(want[0])), what
    assert np.array_equal(bits(got[1]), bits(want[1])), what
    return got


@pytest.mark.parametrize("P,n,E", SHAPES)
def test_perturb_matches_the_restatement_and_writes_nothing_else(dev, P, n, E):
    from gymrl_amd import ops
    assert ops.ES_PAIR_CHUNK == 16
    mu, sigma = centre(P, n)
    mu_d, sigma_d = torch.from_numpy(mu).to(dev), torch.from_numpy(sigma).to(dev)
    want = snes_ref.perturb(mu, sigma, gpu_eps(dev, P, n))
    for stride in (ops.es_stride(n), ops.es_stride(n) + 8):
        stack = torch.full((P + 1, stride), SENTINEL, dtype=torch.float32, device=dev)       # row P: a guard
        out = ops.snes_perturb(mu_d, sigma_d, SEED, generation_of(P), stack[:P])
        assert out.data_ptr() == stack.data_ptr()
        got = stack.cpu().numpy()
        assert np.array_equal(bits(got[:P, :n]), bits(want)), stride
        assert (got[:P, n:] == SENTINEL).all() and (got[P] == SENTINEL).all(), stride
    assert np.array_equal(mu_d.cpu().numpy(), mu) and np.array_equal(sigma_d.cpu().numpy(), sigma)


@pytest.mark.parametrize("P,n,E", SHAPES)
def test_tell_matches_the_restatement_under_float32_and_float64_returns(dev, P, n, E):
    """The float64 returns are small integers plus p * 1e-12: distinct doubles whose float32 casts tie.  The float32 run ranks
    the casts (mean ranks), the float64 run the doubles, so the two must disagree; each equals its own restatement."""
    rng = np.random.default_rng(1000 * P + n)
    mu, sigma = centre(P, n)
    eta = eta_sigma_of(n)
    plain = rng.normal(size=(P, E)).astype(F32)
    got = check_tell(dev, plain, P, n, mu, sigma, eta)
    assert not np.array_equal(bits(got[0]), bits(mu))
    # one pair: w = +-0.5, s_0 = 0 exactly, and a single pair cannot tell a step size anything
    assert np.array_equal(bits(got[1]), bits(sigma)) == (P == 2)
    whole = rng.integers(1, 5, size=(P, E))                          # from 1: p * 1e-12 is far below half a float32 place of it
    whole[1] = whole[0]                                              # a tie among the casts whatever the draw
    wide = whole.astype(np.float64) + np.arange(P)[:, None] * 1e-12
    cast = wide.astype(F32)
    assert np.array_equal(cast, whole.astype(F32))
    assert len(np.unique(snes_ref.fitness(wide))) == P and len(np.unique(snes_ref.fitness(cast))) < P
    got64 = check_tell(dev, wide, P, n, mu, sigma, eta)
    got32 = check_tell(dev, cast, P, n, mu, sigma, eta)              # tied fitness: mean ranks
    assert len(np.unique(got64[2])) == P and len(np.unique(got32[2])) < P
    assert not np.array_equal(bits(got64[2]), bits(got32[2]))
    assert not np.array_equal(bits(got64[0]), bits(got32[0]))


@pytest.mark.parametrize("P,n,E", SHAPES)
def test_all_equal_fitness_leaves_mu_and_sigma_as_they_are(dev, P, n, E):
    mu, sigma = centre(P, n)
    for dtype in (F32, np.float64):
        m, s, w = run_tell(dev, np.full((P, E), -200.0, dtype), mu, sigma, P, eta_sigma_of(n))
        assert not w.any()
        assert np.array_equal(bits(m), bits(mu)) and np.array_equal(bits(s), bits(sigma)), dtype


@pytest.mark.parametrize("P,n,E", [(34, 68, 3), (258, 4672, 3)])
def test_both_clamps_bind(dev, P, n, E):
    """sigma spans [sigma_min, sigma_max] and eta_sigma = 40 turns the factors far past the bounds: the restatement reaches both
    bounds exactly (checked first), and the kernel's step sizes are its bits."""
    rng = np.random.default_rng(P)
    lo, hi = 1e-3, 2.0
    mu = rng.normal(size=n).astype(F32)
    sigma = np.geomspace(lo, hi, n).astype(F32)
    sigma[0], sigma[-1] = F32(lo), F32(hi)
    returns = rng.normal(size=(P, E)).astype(F32)
    want = snes_ref.tell(mu, sigma, returns, gpu_eps(dev, P, n), 1.0, 40.0, lo, hi, 16)
    assert (want[1] == F32(lo)).any() and (want[1] == F32(hi)).any()
    assert ((want[1] > F32(lo)) & (want[1] < F32(hi))).any()
    got = check_tell(dev, returns, P, n, mu, sigma, 40.0, lo, hi)
    assert got[1].min() == F32(lo) and got[1].max() == F32(hi)
