"""The host restatement of the Gaussian policy (tests/gauss_policy_ref.py) against torch.distributions.Normal in float64, and its
Box-Muller draw against the standard normal.  CPU only: what the GPU tests compare the kernels with is checked here first."""
import math

import numpy as np
import pytest

import gauss_policy_ref as ref
from test_rng_distributions import Z2, assert_standard_normal


@pytest.fixture(scope="module")
def recorded():
    return ref.tolerances()


@pytest.mark.parametrize("B,A,ls", ref.SHAPES)
def test_restatement_matches_float64_normal(recorded, B, A, ls):
    """logp, entropy, dmu, dvalue, dlog_std and the metrics within the RECORDED deviation (profiles/ppo_gauss_tolerances.json's
    `observed`: the float32 lines' own rounding, measured over these very inputs)."""
    c = ref.case(B, A, ls)
    got, want = ref.loss(**c), ref.loss_f64(**c)
    d = ref.deviations(got, want, B)
    d["logp"] = float(np.max(np.abs(got["logp"] - want["logp"]) / np.maximum(1.0, np.abs(want["logp"]))))
    d["entropy"] = float(np.max(np.abs(got["entropy"] - want["entropy"]) / np.maximum(1.0, np.abs(want["entropy"]))))
    for name, err in d.items():
        print(f"{name} B={B} A={A} log_std={ls}: {err:.3e} (recorded {recorded[name]['observed']:.3e})")
        assert err <= recorded[name]["observed"], (name, err)


def test_recorded_tolerances_are_the_measured_ones(recorded):
    """profiles/ppo_gauss_tolerances.json holds this measurement and 4 x it, nothing hand-written."""
    worst = ref.measure()
    assert set(worst) == set(recorded)
    for name, v in worst.items():
        assert recorded[name]["observed"] == pytest.approx(v, rel=1e-12, abs=0.0), name
        assert recorded[name]["bound"] == pytest.approx(4.0 * v, rel=1e-12, abs=0.0), name
        assert 0.0 < recorded[name]["bound"] < 1e-4, name                   # float32 lines: a handful of 6e-8 roundings


def test_planted_rows_cover_both_sides_of_every_boundary():
    """the case's first rows sit below / inside / above the clip band under both signs, and on both sides of the dual clip"""
    c = ref.case(257, 3, 0.0)
    want = ref.loss_f64(**c)
    ratio = np.exp(want["logp"] - c["logp_old"].astype(np.float64))[:len(ref.PLANTED)]
    assert np.allclose(ratio, [r for r, _ in ref.PLANTED], rtol=1e-4)
    lo, hi, dual = 1.0 - ref.CFG[0], 1.0 + ref.CFG[0], ref.CFG[1]
    for sign in (1.0, -1.0):
        r = np.array([r for r, a in ref.PLANTED if a * sign > 0])
        assert (r < lo).any() and ((r > lo) & (r < 1.0)).any() and ((r > 1.0) & (r < hi)).any() and (r > hi).any()
    r_neg = np.array([r for r, a in ref.PLANTED if a < 0])
    assert ((r_neg > hi) & (r_neg < dual)).any() and (r_neg > dual).any()
    # past the dual clip under a negative advantage the surrogate is flat: no gradient reaches mu or log_std from that row
    k = [i for i, (r, a) in enumerate(ref.PLANTED) if a < 0 and r > dual]
    assert np.all(ref.loss(**c)["dmu"][k] == 0.0) and np.all(want["dmu"][k] == 0.0)


def test_sample_matches_float64_normal():
    rng = np.random.default_rng(5)
    for A in (1, 3):
        for ls0 in (-3.0, 0.0, 1.0):
            mu, eps = rng.normal(size=(257, A)).astype(np.float32), rng.normal(size=(257, A)).astype(np.float32)
            ls = np.full(A, ls0, np.float32)
            act, lp, H = ref.sample(mu, ls, eps)
            import torch
            dist = torch.distributions.Normal(torch.from_numpy(mu.astype(np.float64)), torch.from_numpy(np.exp(ls.astype(np.float64))).expand(257, A))
            want_lp = dist.log_prob(torch.from_numpy(act.astype(np.float64))).sum(-1).numpy()
            # the draw's logp is a function of eps; at the stored (rounded) action the float64 density differs by the rounding of a
            tol = 1e-5 + 4e-7 * np.abs(eps).max() * np.abs(mu).max() * math.exp(-ls0)
            assert np.max(np.abs(lp - want_lp) / np.maximum(1.0, np.abs(want_lp))) < tol
            assert np.max(np.abs(H - dist.entropy().sum(-1).numpy())) < 1e-5
            det_act, det_lp, _ = ref.sample(mu, ls, deterministic=True)
            assert np.array_equal(det_act, mu) and np.all(det_lp == ref.sample(mu, ls, np.zeros_like(mu))[1])


def test_box_muller_is_standard_normal():
    """2^16 keys (envs 0..2^16-1 at one counter, A = 1), then both halves of a block (A = 2): mean and variance inside the bounds
    tests/test_rng_distributions.py holds its normals to, KS and kurtosis with them."""
    n = 1 << 16
    eps = ref.draw_eps(12345, np.arange(n), 7, 1)[:, 0]
    assert np.isfinite(eps).all()
    assert abs(eps.astype(np.float64).mean()) < Z2 * math.sqrt(1.0 / n)
    assert abs(eps.astype(np.float64).var() - 1.0) < Z2 * math.sqrt(2.0 / n)
    assert_standard_normal(eps, "gaussian_pick eps, A = 1")
    two = ref.draw_eps(12345, np.arange(n), 7, 2)
    assert np.array_equal(two[:, 0], eps)                                   # component 0 does not depend on A
    assert_standard_normal(two[:, 1], "gaussian_pick eps, component 1")
    assert abs(np.corrcoef(two[:, 0].astype(np.float64), two[:, 1].astype(np.float64))[0, 1]) < Z2 / math.sqrt(n)
    other = ref.draw_eps(12345, np.arange(n), 8, 1)[:, 0]                   # the next counter is another stream
    assert abs(np.corrcoef(other.astype(np.float64), eps.astype(np.float64))[0, 1]) < Z2 / math.sqrt(n)


def test_philox_matches_the_scalar_restatement():
    from es_ref import philox4x32
    w = ref.philox4x32(0x0123456789ABCDEF, np.array([1, 2**32 - 1]), np.array([0, 5]), np.uint64(77), np.uint64(ref.RNG_POLICY | 3))
    for j, (c0, c1) in enumerate(((1, 0), (2**32 - 1, 5))):
        assert tuple(int(x[j]) for x in w) == philox4x32(0x0123456789ABCDEF, c0, c1, 77, ref.RNG_POLICY | 3)
