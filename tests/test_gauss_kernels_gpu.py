"""gymrl_gaussian_sample and gymrl_ppo_gauss_loss_fwd_bwd on an MI355X against tests/gauss_policy_ref.py: the sampling side bit for
bit (torch.equal), the loss side within the recorded bound (profiles/ppo_gauss_tolerances.json: 4 x the float32 restatement's own
deviation from float64), dlog_std bit-identical from run to run and from grid to grid."""
import numpy as np
import pytest

import gauss_policy_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED, COUNTER, ID0 = 0x5EED5EED5, (3 << 32) | 41, (1 << 33) + 5         # keys that use the high words


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from gymrl_amd import ops
    assert ops.device_ok(), "libgymrl_hip.so did not find a gfx950 device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bounds():
    return {k: v["bound"] for k, v in ref.tolerances().items()}


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("N", [1, 17, 64, 4099])
def test_sample_equals_the_restatement(dev, N, A):
    from gymrl_amd import ops
    rng = np.random.default_rng(N * 10 + A)
    mu = (2.0 * rng.normal(size=(N, A))).astype(np.float32)
    ls = np.linspace(-3.0, 1.0, A).astype(np.float32) if A > 1 else np.array([0.3], np.float32)
    value = rng.normal(size=N).astype(np.float32)
    noise = rng.normal(size=(N, A)).astype(np.float32)
    drawn = ref.draw_eps(SEED, ID0 + np.arange(N), COUNTER, A)
    for what, eps, kw in (("drawn", drawn, {}), ("explicit", noise, dict(noise_normal=_t(noise, dev))),
                          ("deterministic", None, dict(deterministic=True))):
        want = ref.sample(mu, ls, eps, deterministic=eps is None)
        act, lp, H, v = ops.gaussian_sample(_t(mu, dev), _t(ls, dev), value=_t(value, dev), seed=SEED, counter=COUNTER, env_id0=ID0, **kw)
        for name, g, w in zip(("action", "logp", "entropy"), (act, lp, H), want):
            assert torch.equal(g.cpu(), torch.from_numpy(w)), (what, name)
        assert torch.equal(v.cpu(), torch.from_numpy(value)), what
    assert not np.array_equal(drawn, ref.draw_eps(SEED, ID0 + np.arange(N), COUNTER + 1, A))


def test_online_gae_composition_equals_the_categorical_samplers(dev):
    """The producer side of GAE over T = 35 steps (two whole chunks of 16 and a ragged one) of N = 20 envs: the chunk maps and the
    running pair carry the bits gymrl_categorical_sample leaves on the same rewards, values and dones."""
    from gymrl_amd import ops
    T, N = 35, 20
    rng = np.random.default_rng(3)
    rew, val = _t(rng.normal(size=(T, N)).astype(np.float32), dev), _t(rng.normal(size=(T + 1, N)).astype(np.float32), dev)
    done = _t((rng.random((T, N)) < 0.1).astype(np.uint8), dev)
    mu, ls = torch.zeros(N, 1, device=dev), torch.zeros(1, device=dev)
    logits = torch.zeros(N, 2, device=dev)
    out = []
    for sampler in ("gauss", "cat"):
        running = torch.zeros(2, N, dtype=torch.float64, device=dev)
        ws = ops.gae_workspace(T, N, dev)
        ws.zero_()
        for t in range(1, T):
            on = ops.gae_online(rew[t - 1], done[t - 1], val[t - 1], running, ws, t - 1, T, 0.99, 0.95)
            if sampler == "gauss":
                ops.gaussian_sample(mu, ls, value=val[t], seed=1, counter=t, online=on)
            else:
                ops.categorical_sample(logits, value=val[t], seed=1, counter=t, online=on)
        ops.gae_online_flush(ops.gae_online(rew[T - 1], done[T - 1], val[T - 1], running, ws, T - 1, T, 0.99, 0.95), val[T])
        adv, ret = ops.gae(rew, val[:T].contiguous(), done, val[T], 0.99, 0.95, variant=2, workspace=ws)
        out.append((ws.clone(), running.clone(), adv, ret))
    for g, c in zip(*out):
        assert torch.equal(g, c)
    want_adv, _ = ops.gae(rew, val[:T].contiguous(), done, val[T], 0.99, 0.95, variant=0)
    assert float((out[0][2] - want_adv).abs().max()) < 1e-5


def _loss_case(B, A, dev, M=None, seed=0):
    """ref.case at (B, A); with M the stored rows live in a slab of M rows and idx picks them (a permutation prefix)."""
    c = ref.case(B, A, 0.0 if A == 1 else -0.5, seed=seed)
    idx = None
    slab = {k: c[k] for k in ("act", "logp_old", "adv", "ret")}
    if M is not None:
        rng = np.random.default_rng(B + 7)
        idx = rng.permutation(M)[:B].astype(np.int32)
        filler = ref.case(M, A, 0.0, seed=99)
        slab = {k: filler[k].copy() for k in slab}
        for k in slab:
            slab[k][idx] = c[k]
    return c, slab, idx


@pytest.mark.parametrize("gather,norm", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("B,A", [(1, 1), (63, 1), (64, 3), (65, 1), (4099, 3)])
def test_loss_within_the_recorded_bound_of_float64(dev, bounds, B, A, gather, norm):
    from gymrl_amd import ops
    c, slab, idx = _loss_case(B, A, dev, M=B + 37 if gather else None)
    moments = None
    if norm:                                             # the moments of ANOTHER population: the rows are shifted and scaled
        moments = (100.0, 25.0, 150.0)
    want = ref.loss_f64(**c, moments=moments)
    met = torch.zeros(5, dtype=torch.float64, device=dev)
    dmu, dv, dls = ops.ppo_gauss_loss_fwd_bwd(
        _t(c["mu"], dev), _t(c["log_std"], dev), _t(c["value"], dev), _t(slab["act"], dev), _t(slab["logp_old"], dev),
        _t(slab["adv"], dev), _t(slab["ret"], dev), ref.CFG, idx=None if idx is None else _t(idx, dev),
        adv_moments=None if moments is None else torch.tensor(moments, dtype=torch.float64, device=dev), metrics_sum=met)
    got = dict(dmu=dmu.cpu().numpy(), dvalue=dv.cpu().numpy(), dlog_std=dls.cpu().numpy(), metrics=met.cpu().numpy())
    for name, err in ref.deviations(got, want, B).items():
        print(f"{name} B={B} A={A} gather={gather} norm={norm}: {err:.3e} (bound {bounds[name]:.3e})")
        assert err <= bounds[name], (name, err, bounds[name])
    # the kernel and the restatement share every float32 line: the per-row outputs are the restatement's bits
    host = ref.loss(**c, moments=moments)
    assert np.array_equal(got["dmu"], host["dmu"]) and np.array_equal(got["dvalue"], host["dvalue"])


@pytest.mark.parametrize("B,A", [(65, 1), (4099, 3), (70001, 2)])
def test_dlog_std_is_the_same_bits_from_run_to_run_and_from_grid_to_grid(dev, B, A):
    """B = 70001: 274 segments, so the finalising pass's lanes add two segments each; grids of 1, 3 and 1024 workgroups"""
    from gymrl_amd import ops
    c, slab, _ = _loss_case(B, A, dev)
    args = [_t(c[k], dev) for k in ("mu", "log_std", "value")] + [_t(slab[k], dev) for k in ("act", "logp_old", "adv", "ret")]
    runs = []
    for grid in (0, 0, 1, 3):
        met = torch.zeros(5, dtype=torch.float64, device=dev)
        dmu, dv, dls = ops.ppo_gauss_loss_fwd_bwd(*args, ref.CFG, metrics_sum=met, grid_blocks=grid)
        runs.append((dls.clone(), dmu.clone(), dv.clone(), met))
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1]) and torch.equal(r[2], runs[0][2])
    assert torch.equal(runs[1][3], runs[0][3])                               # the metrics: run to run under one grid
    host = ref.loss(**c)
    assert np.max(np.abs(runs[0][0].cpu().numpy() - host["dlog_std"]) / np.maximum(1.0, np.abs(host["dlog_std"]))) < 1e-6


def test_nan_advantage_reaches_the_loss(dev):
    from gymrl_amd import ops
    c, slab, _ = _loss_case(65, 1, dev)
    slab["adv"][40] = np.nan
    met = torch.zeros(5, dtype=torch.float64, device=dev)
    dmu, dv, dls = ops.ppo_gauss_loss_fwd_bwd(*[_t(c[k], dev) for k in ("mu", "log_std", "value")],
                                              *[_t(slab[k], dev) for k in ("act", "logp_old", "adv", "ret")], ref.CFG, metrics_sum=met)
    assert torch.isnan(met[0]) and torch.isfinite(met[1:]).all()
    assert torch.isnan(dmu[40]).all() and torch.isfinite(dmu[:40]).all() and torch.isfinite(dmu[41:]).all()
    assert torch.isnan(dls).all() and torch.isfinite(dv).all()


def test_loss_is_capturable_in_a_graph(dev):
    from gymrl_amd import ops
    c, slab, _ = _loss_case(257, 3, dev)
    args = [_t(c[k], dev) for k in ("mu", "log_std", "value")] + [_t(slab[k], dev) for k in ("act", "logp_old", "adv", "ret")]
    out = (torch.empty(257, 3, device=dev), torch.empty(257, device=dev), torch.empty(3, device=dev))
    ws = ops.ppo_gauss_loss_workspace(257, 3, dev)
    parts = torch.zeros(ops.loss_blocks(257), 5, dtype=torch.float64, device=dev)
    call = lambda: ops.ppo_gauss_loss_fwd_bwd(*args, ref.CFG, dmu_out=out[0], dvalue_out=out[1], dlog_std_out=out[2],   # noqa: E731
                                              workspace=parts, dls_workspace=ws)
    call()
    eager = [t.clone() for t in out] + [parts.clone()]
    for t in out:
        t.zero_()
    parts.zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for got, want in zip(list(out) + [parts], eager):
        assert torch.equal(got, want)
