"""Grounds tests/optim_ref.py and the oracle's optimiser entry points before tests/test_optim_edges_gpu.py leans on them
(CPU only): adam_f32 against the oracle bit for bit, adam_f64 against the torch.optim.Adam golden, orc_sqnorm against an
exact sum past every grid cap, and the rule for gradients that are not finite against torch itself."""
import numpy as np
import pytest

from conftest import load_golden, rel_close
from optim_ref import BETAS, adam_f32, adam_f64, clip_scale_f32, host_scalars, mixed_grad, sqnorm_fsum

TOL = 1e-5                                   # tests/test_hip_parity.py's
B1, B2 = BETAS
THIRD = float(np.float32(1.0 / 3.0))


@pytest.mark.parametrize("max_norm,clamp,gs", [(0.5, 0.0, 1.0), (0.0, 1.0, 1.0), (10.0, 1.0, THIRD)])
@pytest.mark.parametrize("n", [1, 3, 5, 1003, 4097])
def test_adam_f32_equals_oracle(oracle, n, max_norm, clamp, gs):
    rng = np.random.default_rng(n)
    p = rng.normal(size=n).astype(np.float32)
    m = (0.01 * rng.normal(size=n)).astype(np.float32)
    v = (0.01 * np.abs(rng.normal(size=n))).astype(np.float32)
    po, mo, vo = p, m, v
    lr, eps = 1e-3, 1e-8
    for step in range(1, 6):
        g = mixed_grad(rng, n, step)
        ss, _, bc2s = host_scalars(lr, B1, B2, step)
        scale = clip_scale_f32(oracle.sqnorm(g, gs)[0], max_norm) if max_norm > 0 else 1.0
        p, g1, m, v = adam_f32(p, g, m, v, B1, B2, eps, ss, bc2s, scale, grad_scale=gs, clamp_abs=clamp)
        po, go, mo, vo = oracle.adam_step(po, g, mo, vo, lr, B1, B2, eps, step, grad_scale=gs, max_grad_norm=max_norm,
                                          clamp_abs=clamp, zero_grad=True)
        for a, b in ((p, po), (m, mo), (v, vo), (g1, go)):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), step


def test_adam_f64_reproduces_golden():
    a = load_golden("adam")
    for k in range(int(a["n_cases"])):
        lr, b1, b2, eps, max_norm, clamp = (float(x) for x in a[f"c{k}_hp"])
        p = a[f"c{k}_p0"]
        m = v = np.zeros_like(p)
        for step, g in enumerate(a[f"c{k}_grads"], 1):
            p, _, m, v, _ = adam_f64(p, g, m, v, lr, b1, b2, eps, step, max_norm=max_norm, clamp_abs=clamp)
        assert np.max(np.abs(p - a[f"c{k}_p5"])) <= 2e-6
        assert rel_close(m, a[f"c{k}_m5"]) <= TOL and rel_close(v, a[f"c{k}_v5"]) <= TOL


@pytest.mark.parametrize("gs", [0.5, THIRD])
@pytest.mark.parametrize("n", [1, 3, 5, 4097, 1048577, 4198403])
def test_oracle_sqnorm_against_exact_sum(oracle, n, gs):
    """4097: two partials; 1 048 577: 257 partials, a second round of the final pass; 4 198 403: the cap of 1024
    workgroups, a partly filled second trip of the grid-stride loop and a tail of 3.  A reference that squared before it
    scaled would miss by about 1e-8 at gs = 1/3 (one float32 rounding of every product)."""
    g = mixed_grad(np.random.default_rng(n), n)
    want = sqnorm_fsum(g, gs)
    got = float(oracle.sqnorm(g, gs)[0])
    assert abs(got - want) <= 1e-13 * want, (got, want)


def _torch_nonfinite(bad, mode):
    import torch
    p = torch.nn.Parameter(torch.ones(8))
    opt = torch.optim.Adam([p], lr=1e-3)
    g = torch.full((8,), 0.25)
    g[3] = bad
    p.grad = g
    if mode == "clip":
        torch.nn.utils.clip_grad_norm_([p], 0.5)
    else:
        p.grad.clamp_(-1.0, 1.0)
    opt.step()
    return ~np.isfinite(p.detach().numpy())


@pytest.mark.parametrize("impl", ["oracle", "adam_f32", "adam_f64"])
@pytest.mark.parametrize("mode", ["clip", "clamp"])
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan], ids=["posinf", "neginf", "nan"])
def test_nonfinite_gradient_as_torch(oracle, bad, mode, impl):
    """clip_grad_norm_ + Adam (ppo_lunarlander.py:302-307) and grad.clamp_ + Adam (dqn_cartpole.py:163-166) on 8
    parameters with one bad gradient element: the same parameters stop being finite.  A NaN norm poisons every
    parameter; an infinite one gives coefficient 0, and 0 * inf is NaN at that element only; clamp_ turns +-inf into
    +-1 and keeps NaN."""
    want = _torch_nonfinite(bad, mode)
    p, z = np.ones(8, np.float32), np.zeros(8, np.float32)
    g = np.full(8, 0.25, np.float32)
    g[3] = bad
    max_norm, clamp = (0.5, 0.0) if mode == "clip" else (0.0, 1.0)
    if impl == "oracle":
        got = oracle.adam_step(p, g, z, z, 1e-3, B1, B2, 1e-8, 1, max_grad_norm=max_norm, clamp_abs=clamp)[0]
    elif impl == "adam_f32":
        ss, _, bc2s = host_scalars(1e-3, B1, B2, 1)
        scale = clip_scale_f32(oracle.sqnorm(g)[0], max_norm) if max_norm > 0 else 1.0
        got = adam_f32(p, g, z, z, B1, B2, 1e-8, ss, bc2s, scale, clamp_abs=clamp)[0]
    else:
        got = adam_f64(p, g, z, z, 1e-3, B1, B2, 1e-8, 1, max_norm=max_norm, clamp_abs=clamp)[0]
    assert np.array_equal(~np.isfinite(got), want), (got, want)
    assert want[3] == (not (mode == "clamp" and np.isinf(bad))) and want.sum() == (8 if (mode == "clip" and np.isnan(bad)) else int(want[3]))
