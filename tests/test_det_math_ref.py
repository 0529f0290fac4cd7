"""CPU checks of the reproducible f32 math's host twins on the structured input set (tests/det_math_ref.py): accuracy against
float64 within the exhaustive maxima of tools/check_det_f32.c, the special-value table, the identity of the two tanh forms,
and the exactness identities through which tests/test_det_math_gpu.py reaches the device functions, evaluated on the
restatements of the cells.  The device results inherit all of it through that file's bit-equality tests."""
import math

import numpy as np
import pytest

import det_math_ref as dm
import lstm_ref

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)


@pytest.fixture(scope="module")
def pts(oracle):
    return dm.points()


def _ulps(y, d):
    """|y - d| in ulps of float32(d), the correctly rounded result: tools/check_det_f32.c's score()"""
    with np.errstate(over="ignore", invalid="ignore"):
        rf = d.astype(F32)
        a = np.abs(rf)
        ulp = np.nextafter(a, INF).astype(np.float64) - a.astype(np.float64)
        err = np.abs(y.astype(np.float64) - d) / ulp
    inf = np.isinf(rf) | np.isinf(y)
    return np.where(inf, np.where(rf == y, 0.0, np.inf), err)


def _half_ulp_up(fig):
    """the printed exhaustive maximum, rounded up to the next half ulp: only the rounding of the figure needs covering"""
    return math.floor(fig * 2.0) / 2.0 + 0.5


def test_the_set_is_fixed_and_reaches_every_seam(pts):
    u = dm.bits(pts)
    assert 2_000_000 <= u.size <= 2_500_000 and np.all(np.diff(u.astype(np.int64)) > 0)
    have = set(u[np.isin(u, [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FFFFFFF, 0x7FFFFFFE, 0x7FC002A5, 0x00000001,
                             0x807FFFFF, 0x00800000, 0x7F7FFFFF])].tolist())
    assert len(have) == 11
    for c in (dm.TANH_SMALL, -dm.TANH_BIG, dm.EXP_LO, dm.EXP_HI, dm.LOG_SPLIT, dm.train_tanh_overflow(), *dm.exp_ties()[[0, 127, 255]]):
        w = dm.window(c)
        assert w.size == 2 * dm.WINDOW + 1 and np.isin(w, u).all(), float(c)
    ov = dm.train_tanh_overflow()
    assert F32(ov * dm.TRAIN_SCALE) >= 128 and F32(np.nextafter(ov, -INF) * dm.TRAIN_SCALE) < 128
    for k, c in zip(range(-127, 129), dm.exp_ties()):          # rintf goes both ways inside every tie window
        n = np.rint(dm.from_bits(dm.window(c)) * dm.LOG2E)
        assert n.min() == k and n.max() == k + 1, k
    s = dm.sincos_points()
    assert np.all(np.abs(s) < 8000) and s.size > 10_000_000
    assert dm.rows(pts).shape == (-(-pts.size // 64), 64) and np.array_equal(dm.bits(dm.rows(pts).ravel()[:pts.size]), u)


def test_twins_stay_within_the_exhaustive_maxima(pts):
    x = pts[~np.isnan(pts)]
    x64 = x.astype(np.float64)
    m = (x > dm.EXP_LO) & (x <= dm.EXP_HI)
    worst = {"exp": _ulps(dm.expf(x[m]), np.exp(x64[m])).max()}
    m = (x > 0) & np.isfinite(x)
    worst["log"] = _ulps(dm.logf(x[m]), np.log(x64[m])).max()
    worst["tanh"] = _ulps(dm.tanhf(x), np.tanh(x64)).max()
    t = np.concatenate([dm.sincos_points(), x[np.abs(x) < 8000]])
    s, c = dm.sincosf(t)
    ds, dc = np.sin(t.astype(np.float64)), np.cos(t.astype(np.float64))
    worst["sin"], worst["cos"] = _ulps(s, ds).max(), _ulps(c, dc).max()
    worst_abs = max(np.abs(s - ds).max(), np.abs(c - dc).max())
    print("measured on the structured set:", {k: round(float(v), 4) for k, v in worst.items()}, "sincos abs", float(worst_abs))
    for k, v in worst.items():
        assert v <= _half_ulp_up(dm.MAX_ULP[k]), (k, v, dm.MAX_ULP[k])
    assert worst_abs <= 9.3e-8, worst_abs          # MAX_ABS_SINCOS = 9.296e-8, its printed digits rounded up


def test_special_values_are_what_the_code_states(pts):
    x = pts[~np.isnan(pts)]
    nans = pts[np.isnan(pts)]
    assert nans.size > 8000
    e = dm.expf(x)
    assert np.all(dm.bits(e[x <= dm.EXP_LO]) == 0) and np.all(e[x > dm.EXP_HI] == INF)
    assert np.all(e[(x > dm.EXP_LO) & (x <= dm.EXP_HI)] > 0) and np.all(np.isfinite(e[x <= dm.EXP_HI]))
    assert np.all(dm.bits(dm.expf(np.array([0.0, -0.0], F32))) == dm.bits(F32(1.0)))
    sg = dm.sigmoidf(np.array([-np.inf, np.inf, 0.0, -0.0, -200.0, 200.0], F32))
    assert np.array_equal(dm.bits(sg), dm.bits(np.array([0.0, 1.0, 0.5, 0.5, 0.0, 1.0], F32)))
    for tanh in (dm.tanhf, dm.tanhf_sel):
        t = tanh(x)
        big = np.abs(x) > dm.TANH_BIG
        assert np.array_equal(t[big], np.sign(x[big])) and np.all(np.abs(t[~big]) <= 1)
        assert np.array_equal(dm.bits(tanh(np.array([0.0, -0.0, np.inf, -np.inf], F32))), dm.bits(np.array([0.0, -0.0, 1.0, -1.0], F32)))
        assert np.all(np.signbit(t) == np.signbit(x))
    for name, fn in (("exp", dm.expf), ("tanh", dm.tanhf), ("tanh_sel", dm.tanhf_sel), ("sigmoid", dm.sigmoidf)):
        assert np.all(np.isnan(fn(nans))), name
    assert dm.logf(np.array([1.0], F32))[0] == 0 and np.all(np.isfinite(dm.logf(x[(x > 0) & np.isfinite(x)])))


def test_the_two_tanh_forms_carry_the_same_bits(pts):
    rep = dm.mismatch_report("orc_tanhf vs orc_tanhf_sel", pts, dm.tanhf_sel(pts), dm.tanhf(pts))
    assert not rep, rep


def test_array_entry_point_is_the_scalar_functions(oracle, pts):
    import ctypes as C
    L = oracle.lib()
    x = pts[:: pts.size // 3000]
    x = x[~np.isnan(x)]
    for name, fn in (("orc_expf", dm.expf), ("orc_logf", dm.logf), ("orc_tanhf", dm.tanhf)):
        f = getattr(L, name)
        f.restype, f.argtypes = C.c_float, [C.c_float]
        xs = x[x > 0] if name == "orc_logf" else x
        want = np.array([f(float(v)) for v in xs], F32)
        assert np.array_equal(dm.bits(fn(xs)), dm.bits(want)), name
    xs = x[np.abs(x) < 8000]
    s, c = C.c_float(), C.c_float()
    want = []
    for v in xs:
        L.orc_sincosf(C.c_float(float(v)), C.byref(s), C.byref(c))
        want.append((s.value, c.value))
    want = np.array(want, F32)
    got_s, got_c = dm.sincosf(xs)
    assert np.array_equal(dm.bits(got_s), dm.bits(want[:, 0])) and np.array_equal(dm.bits(got_c), dm.bits(want[:, 1]))
    assert np.all(np.isnan(oracle.map_f32(6, xs)))                             # an op the entry point does not know: NaN


def test_exactness_identities_hold_on_the_restatements(oracle, pts):
    """every construction of det_math_ref.*_inputs returns exactly f(x) when evaluated with the host restatement of its kernel"""
    x = dm.rows(pts)
    gi, gh, h = dm.gru_sigmoid_inputs(x)
    for name, got in (("numpy", dm.gru_cell_fwd(gi, gh, h)[0]), ("oracle", oracle.gru_cell_fwd(gi, gh, h))):
        rep = dm.mismatch_report(f"GRU cell ({name}) as sigmoid", x, got, dm.sigmoidf(x))
        assert not rep, rep
    gi, gh, h = dm.gru_tanh_inputs(x)
    for name, got in (("numpy", dm.gru_cell_fwd(gi, gh, h)[0]), ("oracle", oracle.gru_cell_fwd(gi, gh, h))):
        rep = dm.mismatch_report(f"GRU cell ({name}) as tanh", x, got, dm.tanhf_sel(x))
        assert not rep, rep
    h_new, c_new = lstm_ref.cell_fwd(*dm.lstm_tanh_inputs(x))
    rep = dm.mismatch_report("LSTM cell c' as tanh", x, c_new, dm.tanhf_sel(x)) or \
        dm.mismatch_report("LSTM cell h' as tanh(tanh)", x, h_new, dm.tanhf_sel(dm.tanhf_sel(x)))
    assert not rep, rep
    # gymrl_mlp_forward, one 1 x 1 stage W = [[1]], no bias, tanh: the chain is fmaf(x, 1, +0) then fmaf(0, 0, acc) for the padded
    # k, and acc + 0: x itself but for -0 -> +0 (there is no other pre-scale)
    flat = x.reshape(-1, 1)
    got = oracle.linear_act(flat, np.ones((1, 1), F32), None, act=1)
    rep = dm.mismatch_report("MLP stage as tanh", flat, got, dm.tanhf_sel(flat + F32(0.0)))
    assert not rep, rep
    # gymrl_sac_sample_fwd, log_std = 0, eps = -0, bound = 1: the branchy tanh of x itself, -0 included
    action, _ = oracle.sac_sample_fwd(*dm.sac_tanh_inputs(x), 1.0)
    rep = dm.mismatch_report("SAC squash as tanh", x, action, dm.tanhf(x)) or \
        dm.mismatch_report("SAC squash (branchy) vs the select form", x, action, dm.tanhf_sel(x))
    assert not rep, rep
    assert np.array_equal(dm.bits(action[x == 0]), dm.bits(x[x == 0])) and np.signbit(x[x == 0]).any()
    # gymrl_per_priorities, alpha = 1, eps = 0, no clip: (float)1 * log(e) is log(e)
    pos = pts[(pts > 0) & np.isfinite(pts)]
    assert (pos < np.finfo(F32).tiny).sum() > 4000
    for alpha, eps in ((1.0, 0.0), (0.6, 1e-6)):
        got = oracle.per_priorities(pos, alpha, eps)
        want = dm.per_priority(pos, alpha, eps)
        assert got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64)), (alpha, eps)
    assert np.array_equal(dm.per_priority(pos, 1.0, 0.0), dm.expf(dm.logf(pos)))


def test_saturated_softmax_rows_on_the_restatement():
    for A in (2, 8):
        z, top, low, gap = dm.softmax_case(A)
        p = dm.softmax_fwd(z)
        b = np.arange(z.shape[0] - 1)
        past = -gap[b] <= dm.EXP_LO
        assert past.any() and (~past).any()
        pl = p[b, low[b]]
        assert np.all(dm.bits(pl[past]) == 0) and np.all((pl[~past] > 0) & (pl[~past] < 2 * np.finfo(F32).tiny))
        assert np.all(np.abs(p.astype(np.float64).sum(1) - 1.0) <= 2 * 2.0 ** -23)
        assert np.all(p[-1] == F32(1.0) / F32(A))
