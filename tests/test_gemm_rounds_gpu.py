"""The row-streaming GEMMs (gemm.hip: gemm_ws_kernel / gemm_ns_kernel behind gymrl_linear_fwd / _bwd_input /
_bwd_input_add) PAST one row tile per wave, and the weight gradient past 64 rows per slice.

The kernels are persistent: a wave takes row tile bt * 4 + wave and steps bt by the number of row groups.  Up to
row_groups * rows_per_round rows every wave runs its loop once (tests/test_gemm_gpu.py's bit-exact cases); beyond that
gemm_ws_kernel runs tile t's epilogue inside tile t + 1's MFMA stream, through the previous tile's descriptors, and
gemm_ns_kernel reuses a wave's LDS tile for A rows, output rows and the next A rows.  Every row count here comes from
ops.linear_geometry (the launchers' own arithmetic) and every case asserts that its call runs more than one round.

Each case checks: a row subset bit for bit against the oracle's fmaf chain; EVERY row bit for bit against the same entry
run over single-round chunks (the path the neighbouring file ties to the oracle); the tanh epilogue; the guard rows."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FWD, BWD_INPUT, BWD_INPUT_ADD = 0, 1, 2
GUARD = 3                       # NaN rows behind the output: nothing may be written past B


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from gymrl_amd import ops
    assert ops.device_ok()
    return torch.device("cuda:0")


def _ceil(a, b):
    return -(-a // b)


def _plan(kind, K, N, rounds):
    """B of a case and its geometry.  R = the most rows one round covers (row groups of a huge batch x rows per round).
      'ragged': R + 3 rounds-of-one-group + 2 full row tiles + a partial one: two rounds, the last one partial — some workgroups
                run two tiles and others one, and in the last workgroup one wave has a partial tile and one has no rows;
      'three':  2 R + 95: a tile's epilogue rides on a tile that itself leaves a pending epilogue;
      'full':   2 R: no ragged tile, every wave ends in the tail epilogue with a full `pend`."""
    from gymrl_amd import ops
    rg_max, rpr = ops.linear_geometry(kind, 1 << 40, K, N)
    rows = rpr // 4                                      # one wave's row tile (64 wide kernels, 32 narrow)
    R = rg_max * rpr
    full, tail = {"ragged": (1, 3 * rpr + 2 * rows + rows // 2 + 5), "three": (2, 95), "full": (2, 0)}[rounds]
    B = full * R + tail
    rg, rpr_b = ops.linear_geometry(kind, B, K, N)
    assert (rg, rpr_b) == (rg_max, rpr)
    assert _ceil(B, rpr) > rg                            # more than one round: what this file exists for
    assert _ceil(_ceil(B, rpr), rg) == {"ragged": 2, "three": 3, "full": 2}[rounds]
    if rounds == "ragged":                               # 37 rows of a 64-row tile / 21 of a 32-row one, then an empty wave
        assert 0 < (B % rpr) % rows and _ceil(B % rpr, rows) == 3
    return B, R, rpr


def _oracle_rows(B, R, rpr, seed):
    """The rows compared with the oracle: the first 64, 64 on either side of every round boundary, the last round, 512 at
    random from the rest.  A last round longer than 1024 rows (the exactly-full case: R rows) is represented by its first
    64 rows and its last rows_per_round + 64, the last workgroup's final iteration — the chunked comparison covers the rest."""
    pick = np.zeros(B, bool)
    pick[:64] = True
    rounds = _ceil(B, R)
    for j in range(1, rounds):
        pick[j * R - 64:j * R + 64] = True
    start = (rounds - 1) * R
    if B - start <= 1024:
        pick[start:] = True
    else:
        pick[start:start + 64] = True
        pick[B - rpr - 64:] = True
    rest = np.flatnonzero(~pick)
    pick[np.random.default_rng(seed).choice(rest, size=512, replace=False)] = True
    rows = np.flatnonzero(pick)
    assert rows.size <= 2100
    return rows


def _guarded(B, cols, dev):
    return torch.full((B + GUARD, cols), float("nan"), device=dev)


def _check_guard(out, B):
    assert bool(torch.isnan(out[B:]).all()), "rows past B were written"
    assert not bool(torch.isnan(out[:B]).any()), "a row inside B was left unwritten (or is NaN)"


def _chunked(kind, K, N, B, chunk, call, cols, dev):
    """`call(a, b, out_rows)` over consecutive chunks of `chunk` rows, each a single round by the geometry query."""
    from gymrl_amd import ops
    out = _guarded(B, cols, dev)
    for n in {chunk, B % chunk} - {0}:
        rg, rpr = ops.linear_geometry(kind, n, K, N)
        assert _ceil(n, rpr) <= rg, "a chunk must stay on the one-tile-per-wave path"
    for a in range(0, B, chunk):
        b = min(a + chunk, B)
        call(a, b, out[a:b])
    return out


def _equal_to_single_round_calls(kind, K, N, B, R, rpr, call, got, dev):
    """Every output of the one call against the same entry over single-round chunks: of rows_per_round rows (one workgroup
    per column slice) and of R rows (the whole grid, one tile per wave)."""
    for chunk in (rpr, R):
        want = _chunked(kind, K, N, B, chunk, call, got.shape[1], dev)
        _check_guard(want, B)
        assert torch.equal(got[:B], want[:B]), f"differs from the calls over chunks of {chunk} rows"


FWD_SHAPES = [(256, 256), (256, 512), (128, 128), (128, 256), (64, 64), (64, 128)]
FWD_CASES = ([(K, N, r, True) for (K, N) in FWD_SHAPES for r in ("ragged", "full")] + [(256, 256, "three", True)] +
             [(256, 256, "ragged", False), (128, 128, "ragged", False)])


@pytest.mark.parametrize("K,N,rounds,bias", FWD_CASES)
def test_linear_fwd_past_one_round(dev, oracle, K, N, rounds, bias):
    from gymrl_amd import ops
    B, R, rpr = _plan(FWD, K, N, rounds)
    print(f"fwd K={K} N={N} {rounds}: B={B} R={R} rows_per_round={rpr}")
    g = torch.Generator(device=dev).manual_seed(1000 * K + N + len(rounds))
    x = torch.randn(B, K, device=dev, generator=g)
    W = torch.randn(N, K, device=dev, generator=g) / (16 if K == 256 else 8)     # asymmetric: transposes cannot hide
    b = torch.randn(N, device=dev, generator=g) if bias else None
    rows = _oracle_rows(B, R, rpr, B + N)
    want = oracle.linear_fwd(x[rows].cpu().numpy(), W.cpu().numpy(), None if b is None else b.cpu().numpy())
    for act in (False, True):
        y = _guarded(B, N, dev)
        ops.linear_fwd(x, W, b, y[:B], act=act)
        _check_guard(y, B)
        got = y[rows].cpu().numpy()
        if not act:
            assert np.array_equal(got, want)
        else:   # 1 - 2 / (exp2(x * 2 log2 e) + 1) on the hardware exp2 / rcp units: absolute error, the neighbouring file's bound
            assert np.max(np.abs(got.astype(np.float64) - np.tanh(want.astype(np.float64)))) <= 4e-7
        _equal_to_single_round_calls(FWD, K, N, B, R, rpr, lambda a, e, o: ops.linear_fwd(x[a:e], W, b, o, act=act), y, dev)


BWD_SHAPES = [(256, 256), (512, 256), (256, 128), (128, 128), (128, 64), (64, 64)]          # (N, K)
BWD_CASES = [(N, K, r) for (N, K) in BWD_SHAPES for r in ("ragged", "full")] + [(256, 256, "three")]


@pytest.mark.parametrize("with_h", [True, False])
@pytest.mark.parametrize("N,K,rounds", BWD_CASES)
def test_linear_bwd_input_past_one_round(dev, oracle, N, K, rounds, with_h):
    from gymrl_amd import ops
    B, R, rpr = _plan(BWD_INPUT, K, N, rounds)
    print(f"bwd_input N={N} K={K} {rounds}: B={B} R={R} rows_per_round={rpr}")
    g = torch.Generator(device=dev).manual_seed(77 * N + K + len(rounds))
    dy = torch.randn(B, N, device=dev, generator=g)
    W = torch.randn(N, K, device=dev, generator=g) / (16 if N >= 256 else 8)
    H = torch.tanh(torch.randn(B, K, device=dev, generator=g)) if with_h else None
    rows = _oracle_rows(B, R, rpr, B + K)
    dx = _guarded(B, K, dev)
    ops.linear_bwd_input(dy, W, H, dx[:B])
    _check_guard(dx, B)
    want = oracle.linear_bwd_input(dy[rows].cpu().numpy(), W.cpu().numpy(), None if H is None else H[rows].cpu().numpy())
    assert np.array_equal(dx[rows].cpu().numpy(), want)
    _equal_to_single_round_calls(BWD_INPUT, K, N, B, R, rpr,
                                 lambda a, e, o: ops.linear_bwd_input(dy[a:e], W, None if H is None else H[a:e], o), dx, dev)


@pytest.mark.parametrize("rounds", ["ragged", "full"])
def test_linear_bwd_input_add_past_one_round(dev, oracle, rounds):
    from gymrl_amd import ops
    N, K = 256, 128
    B, R, rpr = _plan(BWD_INPUT_ADD, K, N, rounds)
    print(f"bwd_input_add N={N} K={K} {rounds}: B={B} R={R} rows_per_round={rpr}")
    g = torch.Generator(device=dev).manual_seed(31 + len(rounds))
    dy = torch.randn(B, N, device=dev, generator=g)
    W = torch.randn(N, K, device=dev, generator=g) / 16
    G = torch.randn(B, K, device=dev, generator=g)
    rows = _oracle_rows(B, R, rpr, B)
    dx = _guarded(B, K, dev)
    ops.linear_bwd_input_add(dy, W, G, dx[:B])
    _check_guard(dx, B)
    want = oracle.linear_bwd_input(dy[rows].cpu().numpy(), W.cpu().numpy(), None) + G[rows].cpu().numpy()       # float32 add
    assert want.dtype == np.float32 and np.array_equal(dx[rows].cpu().numpy(), want)
    _equal_to_single_round_calls(BWD_INPUT_ADD, K, N, B, R, rpr, lambda a, e, o: ops.linear_bwd_input_add(dy[a:e], W, G[a:e], o), dx, dev)


# ------------------------------------------------------------------ weight gradient, more than 64 rows per slice ------
def _weight_columns(N):
    """About 32 columns of dy that together hit every position of gemm_tn_kernel's store map
    n = 256 ntile + 128 wn + 4 ip + t, ip = (r & 3) + 8 (r >> 2) + 4 h: both 256-column tiles (N = 512), both wn halves,
    all four t, both h halves, with the accumulator register r varied along the way."""
    cols = []
    combos = itertools.product(range(N // 256), range(2), range(4), range(2))
    for idx, (tile, wn, t, h) in enumerate(combos):
        for r in ({(5 * idx + 3) % 16, (5 * idx + 11) % 16} if N == 256 else {(5 * idx + 3) % 16}):
            cols.append(256 * tile + 128 * wn + 4 * ((r & 3) + 8 * (r >> 2) + 4 * h) + t)
    cols = sorted(set(cols))
    assert len(cols) == 32
    for tile, wn, t, h in itertools.product(range(N // 256), range(2), range(4), range(2)):
        assert any(c // 256 == tile and (c % 256) // 128 == wn and c % 4 == t and ((c % 128) // 4 // 4) % 2 == h for c in cols)
    return cols


# B: 16385 -> 249 slices of 66 rows (not a multiple of 8: the plain block mapping), the last one 17 rows (odd);
#    18943 -> 256 slices of 74 rows, the last one 73 (odd);  11520 at N = 512 -> 128 slices of 90 rows, 2 x 128 partial tiles
@pytest.mark.parametrize("B,N,what", [(16385, 256, "slices % 8"), (18943, 256, "256 slices"), (11520, 512, "workspace full")])
def test_linear_bwd_weight_past_64_rows_per_slice(dev, oracle, B, N, what):
    from gymrl_amd import ops
    slices, rps = ops.linear_bwd_weight_geometry(B, N)
    print(f"bwd_weight B={B} N={N}: slices={slices} rows_per_slice={rps}")
    assert slices * rps >= B and (slices - 1) * rps < B and rps % 2 == 0
    assert rps > 64
    last = B - (slices - 1) * rps
    if what == "slices % 8":
        assert slices % 8 != 0 and last % 2 == 1
    elif what == "256 slices":
        assert slices == 256 and last % 2 == 1
    else:
        assert slices * (N // 256) == 256
    g = torch.Generator(device=dev).manual_seed(13 * B + N)
    x = torch.randn(B, 256, device=dev, generator=g)
    dy = torch.randn(B, N, device=dev, generator=g)
    dW = torch.full((N, 256), float("nan"), device=dev)
    db = torch.full((N,), float("nan"), device=dev)
    ops.linear_bwd_weight(dy, x, dW, ops.gemm_workspace(dev), db)
    # dW[n][:] and db[n] depend on column n of dy alone: the oracle's chains for a column subset
    cols = _weight_columns(N)
    dyc, xc = dy[:, cols].cpu().numpy(), x.cpu().numpy()
    assert np.array_equal(dW[cols].cpu().numpy(), oracle.linear_bwd_weight(dyc, xc, slices, rps))
    assert np.array_equal(db[cols].cpu().numpy(), oracle.linear_bwd_bias(dyc, slices, rps))
    # every other row: fp64 on the device, the bound tests/test_gemm_gpu.py's minibatch test applies to this kernel
    want = dy.double().t() @ x.double()

    def err(got):
        return float((got.double() - want).abs().max() / want.abs().max())

    e_hip, e_lib = err(dW), err(dy.t() @ x)
    print(f"  dW error relative to the largest entry: kernel {e_hip:.3e}, library f32 GEMM {e_lib:.3e}")
    assert e_hip <= 4 * e_lib + 1e-6, (e_hip, e_lib)
    assert float((db.double() - dy.double().sum(0)).abs().max()) <= 1e-5 * float(dy.double().abs().sum(0).max())
