"""GPU edge checks of the one-launch GRU and LSTM sequence kernels (gymrl_gru_seq_fwd/_bwd, gymrl_lstm_seq_fwd/_bwd)
against the float64 loop of tests/rnn_seq_ref.py: every output element written (NaN-filled caller-owned outputs), absent
operands, every hidden size, row placement bit for bit, saturated gates and signed zeros, degenerate shapes, run to run.
The bounds are test_gru_seq_gpu.py's and test_lstm_seq_gpu.py's: rel_close <= 1e-5 forward, <= 1e-4 for the gradients."""
import functools

import numpy as np
import pytest

import rnn_seq_ref as R
from conftest import rel_close

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL_FWD, TOL_BWD = 1e-5, 1e-4
KINDS = ("gru", "lstm")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(kind, dev, c, absent=(), need_d0=True, zeros=False, poison=True):
    """Both directions of one family on case c -> {name: numpy}.  absent: operands passed as None (zeros=True: as explicit
    zero tensors instead).  poison: every output is a caller-owned buffer filled with NaN before the call."""
    from gymrl_amd import ops
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    T, B, HG = c["gi"].shape
    H = HG // R.GATES[kind]
    op = {k: ((td(np.zeros_like(c[k])) if zeros else None) if k in absent else td(c[k])) for k in R.OPERANDS[kind]}
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev) if poison else None  # noqa: E731
    gi, W, b, lens = td(c["gi"]), td(c["W"]), td(c["b"]), c["lens"]
    if kind == "gru":
        h_seq, h_last = ops.gru_seq_fwd(gi, W, b, lens, h0=op["h0"], h_seq=nan(T, B, H), h_last=nan(B, H))
        bwd = ops.gru_seq_bwd(gi, W, b, h_seq, lens, d_hseq=op["d_hseq"], d_hlast=op["d_hlast"], h0=op["h0"], need_dh0=need_d0,
                              dgi=nan(T, B, HG), dgh=nan(T, B, HG), dh0=nan(B, H) if need_d0 else None)
        out = (h_seq, h_last) + bwd
    else:
        fwd = ops.lstm_seq_fwd(gi, W, b, lens, h0=op["h0"], c0=op["c0"], h_seq=nan(T, B, H), c_seq=nan(T, B, H),
                               h_last=nan(B, H), c_last=nan(B, H))
        bwd = ops.lstm_seq_bwd(gi, W, b, fwd[0], fwd[1], lens, d_hseq=op["d_hseq"], d_hlast=op["d_hlast"], d_clast=op["d_clast"],
                               h0=op["h0"], c0=op["c0"], need_d0=need_d0, dgates=nan(T, B, HG),
                               dh0=nan(B, H) if need_d0 else None, dc0=nan(B, H) if need_d0 else None)
        out = fwd + bwd
    return {name: (None if t is None else t.cpu().numpy()) for name, t in zip(R.NAMES[kind], out)}


def _errors(kind, got, ref, c, absent=()):
    """{name: rel_close} of every output, plus the weight gradients formed from dgh / dgates as the caller's GEMMs do."""
    errs = {name: rel_close(got[name], ref[name]) for name in R.NAMES[kind] if got[name] is not None}
    d = "dgh" if kind == "gru" else "dgates"
    h0 = None if "h0" in absent else c["h0"]
    for name, a, w in zip(("dW_hh", "db_hh"), R.weight_grads(got[d], got["h_seq"], h0), R.weight_grads(ref[d], ref["h_seq"], h0)):
        errs[name] = rel_close(a, w)
    return errs


def _check(kind, what, got, ref, c, absent=()):
    """No NaN anywhere, exact zeros past each length, the project's bounds inside, and for a length-0 row the state and
    the gradient handed through bit for bit."""
    for name, a in got.items():
        assert a is None or (a.dtype == np.float32 and a.shape == ref[name].shape and not np.isnan(a).any()), (what, name)
    errs = _errors(kind, got, ref, c, absent)
    print(f"{kind}_seq {what}: " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    for name, e in errs.items():
        assert e <= (TOL_BWD if name.startswith("d") else TOL_FWD), (what, name, e)
    zero = np.zeros(got["h_last"].shape[1], np.float32)
    through = (("h_last", "h0"), ("dh0", "d_hlast")) + ((("c_last", "c0"), ("dc0", "d_clast")) if kind == "lstm" else ())
    for e, n in enumerate(c["lens"]):
        for name in R.NAMES[kind]:
            if got[name] is not None and got[name].ndim == 3:
                assert not got[name][n:, e].any(), (what, name, e)
        if n == 0:
            for out, src in through:
                if got[out] is not None:
                    assert np.array_equal(got[out][e], zero if src in absent else c[src][e]), (what, out, e)
        else:
            assert np.array_equal(got["h_last"][e], got["h_seq"][n - 1, e]), (what, e)
            if kind == "lstm":
                assert np.array_equal(got["c_last"][e], got["c_seq"][n - 1, e]), (what, e)
    return errs


@functools.lru_cache(maxsize=None)
def _pattern_case(kind, H, B, pattern):
    T = 6
    c = R.case(kind, 1000 * H + B, B, T, H, lens=R.length_pattern(pattern, B, T, seed=B))
    return c, R.reference(kind, c)


@functools.lru_cache(maxsize=None)
def _saturated(kind, H):
    c = R.saturated_case(kind, 50 + H, 17, 8, H)
    return c, R.reference(kind, c)


@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("H", [16, 32, 48, 64])
def test_every_output_element_is_written(dev, H, B):
    for kind in KINDS:
        for pattern in R.PATTERNS:
            c, ref = _pattern_case(kind, H, B, pattern)
            _check(kind, f"H={H} B={B} {pattern}", _run(kind, dev, c), ref, c)


@pytest.mark.parametrize("absent", list(R.ABSENT))
@pytest.mark.parametrize("H", [32, 64])
def test_absent_operands(dev, H, absent):
    B, T = 19, 8
    names = R.ABSENT[absent]
    need_d0 = absent != "ppg_rnn"                                     # PPG-RNN's call asks for no dh0
    for kind in KINDS:
        c = R.case(kind, 7 * H, B, T, H)
        assert 0 in c["lens"] and T in c["lens"]
        ref = R.reference(kind, c, names)
        got = _run(kind, dev, c, names, need_d0=need_d0)
        _check(kind, f"H={H} absent={absent}", got, ref, c, names)
        same = _run(kind, dev, c, names, need_d0=need_d0, zeros=True)  # None is zeros, to the bit
        for name in R.NAMES[kind]:
            assert (got[name] is None and same[name] is None) or np.array_equal(got[name], same[name]), (kind, name)
        other = _run(kind, dev, c, names, need_d0=not need_d0)        # asking for dh0 / dc0 or not changes no other bit
        for name in R.NAMES[kind]:
            if got[name] is not None and other[name] is not None:
                assert np.array_equal(got[name], other[name]), (kind, name)
        for name in ("dh0", "dc0")[:R.GATES[kind] - 2]:
            assert (got[name] is None) == (not need_d0) and (other[name] is None) == need_d0, (kind, name)


@pytest.mark.parametrize("B,T", [(17, 24), (1, 40)])
@pytest.mark.parametrize("H", [16, 32, 48, 64])
def test_every_hidden_size_matches_float64(dev, H, B, T):
    for kind in KINDS:
        c = R.case(kind, 31 * H + B, B, T, H)
        errs = _check(kind, f"H={H} B={B} T={T}", _run(kind, dev, c), R.reference(kind, c), c)
        assert {"dW_hh", "db_hh"} <= set(errs)


def _rows_equal(kind, a, rows_a, b, rows_b, what):
    for name in R.NAMES[kind]:
        x = a[name][:, rows_a] if a[name].ndim == 3 else a[name][rows_a]
        y = b[name][:, rows_b] if b[name].ndim == 3 else b[name][rows_b]
        assert np.array_equal(x, y), (kind, what, name)


@pytest.mark.parametrize("H", [32, 64])
def test_rows_do_not_depend_on_their_placement(dev, H):
    every = list(range(R.PERM_B))
    for kind in KINDS:
        c = R.placement_case(kind, 3 * H, H)
        got = _run(kind, dev, c)
        _check(kind, f"H={H} placement", got, R.reference(kind, c), c)
        _rows_equal(kind, _run(kind, dev, R.take_rows(kind, c, R.PERM)), every, got, list(R.PERM), "permuted")
        for row in R.SOLO:                                            # alone, a row has no neighbour to be frozen beside
            _rows_equal(kind, _run(kind, dev, R.take_rows(kind, c, [row])), [0], got, [row], f"row {row} alone")


def test_rows_do_not_depend_on_their_launch(dev):
    """B = 770 is one launch of 768 rows and one of 2: rows 766..769 as their own batch of four, and the batch rolled by
    one row (old row 767, the first launch's last, becomes the second launch's first)."""
    B, T, H = 770, 3, 16
    seam = [766, 767, 768, 769]
    for kind in KINDS:
        c = R.case(kind, 77, B, T, H, lens=np.random.default_rng(77).integers(0, T + 1, size=B))
        for row, n in zip(seam, (T, 2, T, 1)):
            c["lens"][row] = n
        got = _run(kind, dev, c)
        _check(kind, "B=770", got, R.reference(kind, c), c)
        _rows_equal(kind, _run(kind, dev, R.take_rows(kind, c, seam)), [0, 1, 2, 3], got, seam, "seam rows alone")
        rolled = [(i - 1) % B for i in range(B)]
        _rows_equal(kind, _run(kind, dev, R.take_rows(kind, c, rolled)), [768, 0, 1], got, [767, 769, 0], "rolled by one")


@pytest.mark.parametrize("H", [16, 64])
def test_saturated_gates_and_signed_zeros(dev, H):
    for kind in KINDS:
        c, ref = _saturated(kind, H)
        got = _run(kind, dev, c)
        for name, a in got.items():
            assert np.isfinite(a).all(), (kind, name)
        _check(kind, f"H={H} saturated", got, ref, c)
        for name in R.BWD[kind]:                                      # an exactly zero gradient comes out as zero
            dead = ref[name] == 0.0
            assert dead.any() or got[name].ndim == 2
            worst = float(np.abs(got[name][dead]).max()) if dead.any() else 0.0
            print(f"{kind}_seq H={H} saturated {name}: {int(dead.sum())} exact zeros in float64, largest |kernel| there {worst:.3e}")
            assert worst <= 1e-30, (kind, name, worst)


@pytest.mark.parametrize("H", [16, 64])
def test_degenerate_shapes(dev, H):
    for kind in KINDS:
        G = R.GATES[kind]
        c = R.case(kind, 5, 5, 0, H, lens=[0] * 5)                    # T = 0: the state and its gradient pass through
        got = _run(kind, dev, c)
        assert got["h_seq"].shape == (0, 5, H) and got[R.BWD[kind][0]].shape == (0, 5, G * H)
        assert np.array_equal(got["h_last"], c["h0"]) and np.array_equal(got["dh0"], c["d_hlast"])
        if kind == "lstm":
            assert got["c_seq"].shape == (0, 5, H)
            assert np.array_equal(got["c_last"], c["c0"]) and np.array_equal(got["dc0"], c["d_clast"])
        got = _run(kind, dev, c, R.ABSENT["all"])
        assert all(not a.any() and not np.isnan(a).any() for a in got.values())
        c = R.case(kind, 5, 0, 4, H, lens=[])                         # B = 0: nothing to do, and no error
        for poison in (True, False):
            got = _run(kind, dev, c, poison=poison)
            assert got["h_seq"].shape == (4, 0, H) and got["h_last"].shape == (0, H) and got["dh0"].shape == (0, H)
            assert got[R.BWD[kind][0]].shape == (4, 0, G * H)


def test_run_to_run_bit_identical(dev):
    cases = [(kind, _pattern_case(kind, H, 33, "random")[0]) for kind in KINDS for H in (16, 32, 48, 64)]
    cases += [(kind, _saturated(kind, H)[0]) for kind in KINDS for H in (16, 64)]
    for kind, c in cases:
        a, b = _run(kind, dev, c), _run(kind, dev, c)
        for name in R.NAMES[kind]:
            assert np.array_equal(a[name], b[name], equal_nan=True), (kind, name)
