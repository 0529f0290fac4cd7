"""GPU sweep of the reproducible f32 math over the structured input set of tests/det_math_ref.py.

The device functions are reached through entry points whose surrounding arithmetic is exact (det_math_ref.*_inputs state why),
and held to their host twins BIT FOR BIT: the contract is equality, no tolerance is fitted to device output, and the accuracy
the twins have against float64 (tests/test_det_math_ref.py, tools/check_det_f32.c) carries over.  train_tanhf has no twin:
it is held to its header's absolute bound against float64 tanh, on the set and over all 2^32 patterns.  Then the consumers
(GRU / LSTM cell backward, softmax rows) run saturated, against their restatements."""
import time

import numpy as np
import pytest

import det_math_ref as dm
import lstm_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
# train_device.hpp: "absolute error <= 2.22e-7 everywhere".  The header used to say "< 2e-7"; the exhaustive pass below measured
# 2.216e-7 at x = 0xbfe86f11 (1.959e-7 on the structured set), and the claim was corrected to the measured figure.
TRAIN_TANH_ABS = 2.22e-7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pts(oracle):
    return dm.points()


@pytest.fixture(scope="module")
def xrows(pts, dev):
    x = dm.rows(pts)
    return x, torch.from_numpy(x).to(dev)


def _td(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _same(name, x, got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    rep = dm.mismatch_report(name, x, got, want)
    assert not rep, rep


def test_sigmoid_and_exp_through_the_gru_cell_carry_the_twins_bits(dev, xrows):
    from gymrl_amd import ops
    x, _ = xrows
    got = ops.gru_cell_fwd(*_td(dev, *dm.gru_sigmoid_inputs(x)))
    _same("det_sigmoidf via gymrl_gru_cell_fwd", x, got, dm.sigmoidf(x))
    got = got.cpu().numpy()
    assert np.all(got[np.isneginf(x)] == 0) and np.all(got[np.isposinf(x)] == 1) and np.all(np.isnan(got[np.isnan(x)]))
    # exp(-x) = +inf beyond 88.72283 and +0 from 87.33654 on: 1 / (1 + inf) = +0, 1 / (1 + 0) = 1
    assert np.all(dm.bits(got[-x > dm.EXP_HI]) == 0) and np.all(got[-x <= dm.EXP_LO] == 1)


def test_tanh_sel_through_gru_lstm_and_mlp_carries_the_twins_bits(dev, xrows):
    from gymrl_amd import ops
    x, _ = xrows
    want = dm.tanhf_sel(x)
    got = ops.gru_cell_fwd(*_td(dev, *dm.gru_tanh_inputs(x)))
    _same("det_tanhf_sel via gymrl_gru_cell_fwd", x, got, want)
    got = got.cpu().numpy()
    big = np.abs(x) > dm.TANH_BIG
    assert np.array_equal(got[big], np.sign(x[big])) and np.all(np.isnan(got[np.isnan(x)]))
    zero = x == 0
    assert np.array_equal(dm.bits(got[zero]), dm.bits(x[zero]))                       # +-0 -> +-0
    h_new, c_new = ops.lstm_cell_fwd(*_td(dev, *dm.lstm_tanh_inputs(x)))
    _same("det_tanhf_sel via gymrl_lstm_cell_fwd c'", x, c_new, want)
    _same("det_tanhf_sel twice via gymrl_lstm_cell_fwd h'", x, h_new, dm.tanhf_sel(want))
    # one 1 x 1 stage, W = [[1]], no bias: fmaf(x, 1, +0), zeros for the padded k, + 0 -> x but for -0 -> +0
    flat = x.reshape(-1, 1)
    W, xin = _td(dev, np.ones((1, 1), F32), flat)
    out = torch.empty(flat.shape[0], 1, device=dev)
    stages = [dict(W=ops.mlp_pack(W), shape=(1, 1), b=None, act=ops.ACT_TANH, src=-1, dst=-1, out=out)]
    ops.mlp_forward(xin, ops.mlp_desc(stages))
    _same("det_tanhf_sel via gymrl_mlp_forward", flat, out, dm.tanhf_sel(flat + F32(0.0)))


def test_branchy_tanh_through_the_sac_squash_is_the_select_form(dev, xrows):
    """gymrl_sac_sample_fwd with log_std = 0, eps = -0, bound = 1 (det_math_ref.sac_tanh_inputs): std = exp(0) = 1,
    x = mean + 1 * (-0) = mean for every mean, -0 included; action = det_tanhf(x) * 1."""
    from gymrl_amd import ops
    x, _ = xrows
    action, _ = ops.sac_sample_fwd(*_td(dev, *dm.sac_tanh_inputs(x)), 1.0)
    action = action.cpu().numpy()
    _same("det_tanhf via gymrl_sac_sample_fwd", x, action, dm.tanhf(x))
    _same("det_tanhf vs det_tanhf_sel, every x", x, action, dm.tanhf_sel(x))
    zero = x == 0
    assert np.signbit(x[zero]).any() and np.array_equal(dm.bits(action[zero]), dm.bits(x[zero]))       # +-0 -> +-0
    big = np.abs(x) > dm.TANH_BIG
    assert np.array_equal(action[big], np.sign(x[big])) and np.all(np.isnan(action[np.isnan(x)]))


@pytest.mark.parametrize("alpha,eps", [(1.0, 0.0), (0.6, 1e-6)])
def test_exp_of_log_through_per_priorities_carries_the_twins_bits(dev, pts, alpha, eps):
    from gymrl_amd import ops
    pos = pts[(pts > 0) & np.isfinite(pts)]
    got = ops.per_priorities(_td(dev, pos)[0], alpha, eps).cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, got.astype(F32).astype(np.float64))   # an exact float32 value
    _same(f"exp(alpha log) via gymrl_per_priorities alpha={alpha}", pos, got.astype(F32), dm.per_priority(pos, alpha, eps))
    if alpha == 1.0 and eps == 0.0:          # det_expf's special values on the device itself: the priority is exp(log(e))
        lg = dm.logf(pos)
        assert lg[pos == 1][0] == 0 and np.all(got[pos == 1] == 1.0)                                     # exp(+0) = 1
        flushed = lg <= dm.EXP_LO
        assert flushed.sum() > 4000 and np.all(got[flushed] == 0) and not np.signbit(got[flushed]).any()  # exp(x <= -87.33654f) = +0
        assert np.all(got[~flushed] > 0) and np.all(np.isposinf(got[lg > dm.EXP_HI]))


def _train_tanh(ops, xd):
    return ops.tanh_inplace(xd.clone())


def test_train_tanh_meets_its_header_on_the_set_and_is_one_function(dev, xrows):
    from gymrl_amd import ops
    x, xd = xrows
    y = _train_tanh(ops, xd)
    flat = xd.reshape(-1, 1)
    y_lin = ops.lin_fwd(flat, torch.ones(1, 1, device=dev), None, act=ops.LIN_ACT["tanh"])
    _same("train_tanhf: gymrl_lin_fwd (K = 1, W = 1) vs gymrl_tanh_inplace", x.reshape(-1, 1), y_lin, y.reshape(-1, 1).cpu().numpy())
    ref = torch.tanh(xd.double())
    nan = torch.isnan(xd)
    assert bool(torch.isnan(y[nan]).all()) and not bool(torch.isnan(y[~nan]).any())
    assert bool((y[torch.isposinf(xd)] == 1).all()) and bool((y[torch.isneginf(xd)] == -1).all())
    ov = float(dm.train_tanh_overflow())
    assert bool((y[xd >= ov] == 1).all()) and bool((y[xd <= -ov] == -1).all())
    err = torch.where(nan, torch.zeros_like(ref), (y.double() - ref).abs())
    at = int(err.argmax())
    print(f"train_tanhf on the set: max abs err {float(err.max()):.4g} at x = 0x{dm.bits(x.ravel()[at:at + 1])[0]:08x}")
    assert float(err.max()) <= TRAIN_TANH_ABS, (float(err.max()), float(x.ravel()[at]))


def test_train_tanh_meets_its_header_on_every_float(dev):
    from gymrl_amd import ops
    worst, worst_at = 0.0, 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for c in range(64):
        u = torch.arange(c << 26, (c + 1) << 26, dtype=torch.int64, device=dev)
        xd = (u - ((u >> 31) << 32)).to(torch.int32).view(torch.float32)      # the pattern as a two's-complement int32
        y = ops.tanh_inplace(xd.clone())
        err = (y.double() - torch.tanh(xd.double())).abs()
        err = torch.where(torch.isnan(xd), torch.zeros_like(err), err)         # NaN patterns excluded (NaN out: the set's test)
        m, at = err.max(0)
        if float(m) > worst:
            worst, worst_at = float(m), (c << 26) + int(at)
    torch.cuda.synchronize()
    print(f"train_tanhf over 2^32 patterns: max abs err {worst:.4g} at x = 0x{worst_at:08x}, {time.perf_counter() - t0:.2f} s")
    assert worst <= TRAIN_TANH_ABS, (worst, hex(worst_at))


def _gru_bwd_ref(gi, gh, h, go):
    """gru_point_bwd in numpy float32 -> (dgi, dgh, dh) and the gate derivatives"""
    n_h = h.shape[1]
    _, (r, z, n) = dm.gru_cell_fwd(gi, gh, h)
    one = F32(1.0)
    hn = gh[:, 2 * n_h:]
    dn, dz = go * (one - z), go * (h - n)
    dnp = dn * (one - n * n)
    dr, dzz = r * (one - r), z * (one - z)
    dir_, diz = (dnp * hn) * dr, dz * dzz
    return (np.concatenate([dir_, diz, dnp], 1), np.concatenate([dir_, diz, dnp * r], 1), go * z), (dr, dzz, one - n * n)


def _nan_pattern_or_finite(name, got, want):
    got = got.cpu().numpy()
    assert np.all(dm.same_bits(got, want)), name
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), name
    return got


def test_saturated_gru_cell_backward_is_the_restatement_with_exact_zeros(dev, oracle):
    from gymrl_amd import ops
    B, n_h = 33, 64
    gi, gh, h, go = dm.saturated_gru_case(B, n_h)
    assert np.abs(gi + gh).max() > 200 and np.isinf(gi[1]).sum() == 6
    with np.errstate(invalid="ignore", over="ignore"):
        want, (dr, dz, dn) = _gru_bwd_ref(gi, gh, h, go)
        assert all(np.all(dm.same_bits(a, b)) for a, b in zip(want, oracle.gru_cell_bwd(gi, gh, h, go)))
        out = ops.gru_cell_fwd(*_td(dev, gi, gh, h))
        _nan_pattern_or_finite("h'", out, dm.gru_cell_fwd(gi, gh, h)[0])
    got = [_nan_pattern_or_finite(k, a, w) for k, a, w in zip(("dgi", "dgh", "dh"), ops.gru_cell_bwd(*_td(dev, gi, gh, h, go)), want)]
    assert all(np.all(np.isfinite(w)) for w in want)          # r (1 - r), 1 - n^2 are exactly 0 when saturated: no inf * 0
    dgi = got[0]
    for k, d in enumerate((dr, dz, dn)):
        assert (d == 0).mean() > 0.5
        assert np.all(dgi[:, k * n_h:(k + 1) * n_h][d == 0] == 0), k


@pytest.mark.parametrize("B,n_h", [(7, 16), (33, 64)])
def test_saturated_lstm_cell_backward_is_the_restatement_with_exact_zeros(dev, oracle, B, n_h):
    from gymrl_amd import ops
    gi, gh, c, dh, dc = dm.saturated_lstm_case(B, n_h)
    assert np.abs(gi + gh).max() > 200 and np.isinf(gi[1]).sum() == 8
    with np.errstate(invalid="ignore", over="ignore"):
        i, f, g, o = lstm_ref.gates(gi, gh)
        r_h, r_c = lstm_ref.cell_fwd(gi, gh, c)
        h_new, c_new = ops.lstm_cell_fwd(*_td(dev, gi, gh, c))
        _nan_pattern_or_finite("h'", h_new, r_h)
        _nan_pattern_or_finite("c'", c_new, r_c)
        one = F32(1.0)
        tc = lstm_ref.tanhf(r_c)
        for dcn in (None, dc):
            r_dg, r_dcp = lstm_ref.cell_bwd(gi, gh, c, dh, dcn)
            dgates, dcp = ops.lstm_cell_bwd(*_td(dev, gi, gh, c, dh), None if dcn is None else _td(dev, dcn)[0])
            dgates = _nan_pattern_or_finite("dgates", dgates, r_dg)
            _nan_pattern_or_finite("dc", dcp, r_dcp)
            assert np.all(np.isfinite(r_dg)) and np.all(np.isfinite(r_dcp))
            for k, d in enumerate((i * (one - i), f * (one - f), one - g * g, o * (one - o))):
                assert (d == 0).mean() > 0.5
                assert np.all(dgates[:, k * n_h:(k + 1) * n_h][d == 0] == 0), k
            if dcn is None:                                  # dc = (dh o)(1 - tc^2) alone: 0 where tanh(c') is +-1
                assert np.all(dcp.cpu().numpy()[(one - tc * tc) == 0] == 0)


@pytest.mark.parametrize("A", [2, 8])
def test_softmax_rows_past_the_flush_threshold(dev, oracle, A):
    from gymrl_amd import ops
    z, top, low, gap = dm.softmax_case(A)
    B = z.shape[0]
    assert B == 257
    want = dm.softmax_fwd(z)
    zd = _td(dev, z)[0].requires_grad_(True)
    p_dev = ops.softmax_rows(zd)
    _same("gymrl_softmax_rows_fwd", z, p_dev.detach(), want)
    p = p_dev.detach().cpu().numpy()
    b = np.arange(B - 1)
    past = -gap[b] <= dm.EXP_LO
    pl = p[b, low[b]]
    assert np.all(dm.bits(pl[past]) == 0) and np.all((pl[~past] > 0) & (pl[~past] < 2 * np.finfo(F32).tiny))
    assert np.all(np.abs(p.astype(np.float64).sum(1) - 1.0) <= 2 * 2.0 ** -23)
    assert np.all(p[-1] == F32(1.0) / F32(A))
    g = np.random.default_rng(A).normal(size=z.shape).astype(F32)
    p_dev.backward(_td(dev, g)[0])
    _same("gymrl_softmax_rows_bwd", z, zd.grad, dm.softmax_bwd(want, g))
    assert np.all(zd.grad.cpu().numpy()[b, low[b]][past] == 0)
