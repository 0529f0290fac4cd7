"""gymrl_lin_fwd / _bwd_input / _bwd_weight (csrc/lin.hip) bit for bit against the oracle's restatement of the documented
accumulation order, at the launchers' tile and dispatch seams.

Every output is a window of a NaN-filled buffer (3 guard rows, and guard columns where the kernel takes a row stride):
after the call everything outside the window is still NaN and nothing inside is.  Every comparison with the oracle is
np.array_equal on all rows (the 4 M-row skinny case and the 128 x 128 LDS case name their subsets).  Every case asserts,
through tests/lin_ref.py's restatement of the launchers' rules, the kernel, tile width, slice count and last-slice length
it means to reach; the slice count is also read back from gymrl_lin_workspace_bytes.

Two epilogues cannot be restated on the host and are held to float64 of the bit-pinned pre-activation instead: tanh
(train_tanhf: hardware exp2 and rcp; bound derived in lin_ref.tanh_bound) and SiLU (device expf; yardstick torch's silu).
Their outputs are still required to be the same bits on every sibling path (vector / scalar, NT 1 / 4, batched / single).
"""
import functools
import math

import numpy as np
import pytest
import torch

import lin_ref as L
from lin_ref import ACT, F32

pytestmark = pytest.mark.gpu

D = "cuda"
LO, HI = -0.7, 0.9
ACTS = ["none", "relu", "tanh", "clamp"]
NAN = float("nan")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


# ---- data -------------------------------------------------------------------------------------------------------------
def _weight(rng, N, K, fan):
    """Asymmetric (a ramp over the columns on top of the noise), scaled 1 / sqrt(fan)."""
    return (rng.standard_normal((N, K)) * (0.5 + np.arange(K) / K) / math.sqrt(fan)).astype(F32)


def _saved(rng, shape, act):
    """A saved activation output from the activation itself: exact 0 (relu) and exact lo / hi (clamp) occur."""
    z = rng.standard_normal(shape).astype(F32)
    if act == "relu":
        return np.maximum(z, F32(0))
    if act == "tanh":
        return np.tanh(z).astype(F32)
    if act == "clamp":
        return np.minimum(np.maximum(z, F32(LO)), F32(HI))
    return z


def _place(a, mode="aligned"):
    """The array on the device as a view with the given layout, NaN around it.  aligned: its own tensor; ld4 / ld1: the
    first columns of a buffer 4 / 1 wider; off1: one float into a flat buffer (16-byte misaligned, compact rows); col1: a
    column slice starting one float into a wider buffer."""
    t = torch.from_numpy(np.array(a, copy=True))       # (a copy: the shared big cases are read-only)
    if mode == "aligned":
        return t.to(D)
    if t.dim() == 1 or mode == "off1":
        flat = torch.full((t.numel() + 5,), NAN, dtype=t.dtype, device=D)
        v = flat[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        return v
    extra = {"ld4": 4, "ld1": 1, "col1": 3}[mode]
    c0 = 1 if mode == "col1" else 0
    buf = torch.full((t.shape[0], t.shape[1] + extra), NAN, dtype=t.dtype, device=D)
    v = buf[:, c0:c0 + t.shape[1]]
    v.copy_(t)
    return v


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _al(*ts):
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


def _np(t):
    return t.detach().cpu().numpy().copy()


# ---- runners: launch into guarded windows, assert the path, check the guards ------------------------------------------
def run_fwd(xs, Ws, bs, acts, x2s=None, x_mode="aligned", w_mode="aligned", expect=None):
    """One gymrl_lin_fwd launch of len(Ws) items (numpy in, numpy out).  expect: (NT, VEC) the launch must take."""
    from gymrl_amd import ops
    n = len(Ws)
    x2s = x2s or [None] * n
    B, K1 = xs[0].shape
    N, K = Ws[0].shape
    tx = [_place(x, x_mode) for x in xs]
    tx2 = [None if x2 is None else _place(x2, x_mode) for x2 in x2s]
    tw = [_place(w, w_mode) for w in Ws]
    tb = [None if b is None else _place(b, w_mode) for b in bs]
    assert L.fwd_path(B, K, K1, N, _ld(tx[0]), _al(*tx, *tw)) == expect, (L.fwd_path(B, K, K1, N, _ld(tx[0]), _al(*tx, *tw)), expect)
    outs = [L.guarded(torch, B, N, D) for _ in range(n)]
    ops.lin_fwd(tx if n > 1 else tx[0], tw if n > 1 else tw[0], tb if n > 1 else tb[0],
                [ACT[a] for a in acts] if n > 1 else ACT[acts[0]], x2=tx2 if n > 1 else tx2[0],
                out=[v for _, v in outs] if n > 1 else outs[0][1], lo=LO, hi=HI)
    for buf, _ in outs:
        assert L.guards_intact(torch, buf, (B, N))
    return [_np(v) for _, v in outs]


def check_fwd(orc, got, x, W, b, act, x2=None):
    """none / relu / clamp: the oracle's bits.  tanh: the derived bound around float64 tanh of the oracle's z."""
    if act == "tanh":
        z = L.fwd(orc, x, W, b, ACT["none"], x2=x2)
        err = np.abs(got.astype(np.float64) - np.tanh(z.astype(np.float64)))
        assert (err <= L.tanh_bound(z)).all(), float((err / L.tanh_bound(z)).max())
    else:
        assert np.array_equal(got, L.fwd(orc, x, W, b, ACT[act], LO, HI, x2=x2))


def run_bwd_input(dys, ys, Ws, acts, K1=None, want=(True, True), old=None, sum_items=False, mode="aligned", w_mode="aligned",
                  compact=False, expect=None):
    """One gymrl_lin_bwd_input launch.  old: [B, K] float32 the destinations start from (accumulate), else NaN.
    compact: exact-width destinations (guard rows only).  Returns the list of [B, K] results, NaN where not wanted."""
    from gymrl_amd import ops
    n = len(Ws)
    B, N = dys[0].shape
    K = Ws[0].shape[1]
    K1 = K if K1 is None else K1
    tdy = [_place(a, mode) for a in dys]
    ty = [None if a is None else _place(a, mode) for a in ys]
    tw = [_place(w, w_mode) for w in Ws]
    n_out = 1 if sum_items else n
    w1, w2 = want[0] and K1 > 0, want[1] and K1 < K
    g1 = [L.guarded(torch, B, K1, D, None if old is None else torch.from_numpy(old[:, :K1]), col_guard=not compact)
          if w1 else None for _ in range(n_out)]
    g2 = [L.guarded(torch, B, K - K1, D, None if old is None else torch.from_numpy(old[:, K1:]), col_guard=not compact)
          if w2 else None for _ in range(n_out)]
    dx = [g[1] if g else None for g in g1] + [None] * (n - n_out)
    dx2 = [g[1] if g else None for g in g2] + [None] * (n - n_out)
    if sum_items:
        dx, dx2 = [dx[0]] * n, [dx2[0]] * n
    lddx = _ld(dx[0]) if w1 else K
    path = L.bwd_input_path(B, N, K, K1, _ld(tdy[0]), lddx, sum_items, n, _al(*tdy, *[t for t, a in zip(ty, acts) if a != "none"]),
                            w1 and _al(*[d for d in dx if d is not None], *tw))
    assert path == expect, (path, expect)
    multi = n > 1
    ops.lin_bwd_input(tdy if multi else tdy[0], ty if multi else ty[0], tw if multi else tw[0],
                      [ACT[a] for a in acts] if multi else ACT[acts[0]], K1=K1,
                      dx=(dx if multi else dx[0]) if w1 else None, dx2=(dx2 if multi else dx2[0]) if w2 else None,
                      want=want, lo=LO, hi=HI, accumulate=old is not None, sum_items=sum_items)
    res = []
    for i in range(n_out):
        full = np.full((B, K), np.nan, F32)
        if w1:
            assert L.guards_intact(torch, g1[i][0], (B, K1), col_guard=not compact)
            full[:, :K1] = _np(g1[i][1])
        if w2:
            assert L.guards_intact(torch, g2[i][0], (B, K - K1), col_guard=not compact)
            full[:, K1:] = _np(g2[i][1])
        res.append(full)
    return res


def _wanted(a, K1, want):
    a = a.copy()
    if not want[0]:
        a[:, :K1] = np.nan
    if not want[1]:
        a[:, K1:] = np.nan
    return a


def run_bwd_weight(dys, ys, xs, acts, x2s=None, with_db=True, old=None, dy_mode="aligned", expect=None):
    """One gymrl_lin_bwd_weight launch into row-guarded dW [N, K] and guarded db [N].  old: (dW, db) to accumulate onto.
    expect: (kernel, nt, slices, rows_per_slice, last-slice rows).  Returns [(dW, db | None)] per item."""
    from gymrl_amd import _lib, ops
    n = len(dys)
    x2s = x2s or [None] * n
    B, N = dys[0].shape
    K1 = xs[0].shape[1]
    K = K1 + (0 if x2s[0] is None else x2s[0].shape[1])
    tdy = [_place(a, dy_mode) for a in dys]
    ty = [None if a is None else _place(a, dy_mode) for a in ys]
    tx = [_place(a) for a in xs]
    tx2 = [None if a is None else _place(a) for a in x2s]
    gw = [L.guarded(torch, N, K, D, None if old is None else torch.from_numpy(old[0]), col_guard=False) for _ in range(n)]
    gb = [L.guarded_vec(torch, N, D, None if old is None else torch.from_numpy(old[1])) if with_db else None for _ in range(n)]
    ld_ok = _ld(tdy[0]) % 4 == 0 and _ld(tx[0]) % 4 == 0
    path = L.bwd_weight_path(B, N, K, K1, max(ACT[a] for a in acts), ld_ok, _al(*tdy, *tx, *[g[1] for g in gw]))
    assert path == expect, (path, expect)
    assert L.slices_from_workspace(_lib.lib().gymrl_lin_workspace_bytes(B, N, K, n), n, N, K) == path[2]
    multi = n > 1
    dbs = [g[1] if g else None for g in gb]
    ops.lin_bwd_weight(tdy if multi else tdy[0], ty if multi else ty[0], tx if multi else tx[0],
                       [g[1] for g in gw] if multi else gw[0][1], dbs if multi else dbs[0],
                       [ACT[a] for a in acts] if multi else ACT[acts[0]], x2=tx2 if multi else tx2[0], lo=LO, hi=HI,
                       accumulate=old is not None)
    res = []
    for i in range(n):
        assert L.guards_intact(torch, gw[i][0], (N, K), col_guard=False)
        if with_db:
            assert L.guards_intact(torch, gb[i][0], (N,))
        res.append((_np(gw[i][1]), _np(gb[i][1]) if with_db else None))
    return res


def check_bwd_weight_variants(orc, dy, y, x, act, expect, x2=None, ref=None, dy_mode="aligned"):
    """db present / None x accumulate off / on against ONE oracle evaluation (accumulate is one float32 add on top)."""
    B, N = dy.shape
    xc = x if x2 is None else np.concatenate([x, x2], 1)
    if ref is None:
        ref = orc.lin_bwd_weight(dy, y, xc, expect[2], expect[3], ACT[act], LO, HI)
    rng = np.random.default_rng(B + N)
    old = (rng.standard_normal(ref[0].shape).astype(F32), rng.standard_normal(N).astype(F32))
    outs = {}
    for with_db in (True, False):
        for acc in (False, True):
            (dW, db), = run_bwd_weight([dy], [y], [x], [act], [x2], with_db, old if acc else None, dy_mode, expect)
            assert np.array_equal(dW, old[0] + ref[0] if acc else ref[0]), (act, with_db, acc)
            if with_db:
                assert np.array_equal(db, old[1] + ref[1] if acc else ref[1]), (act, with_db, acc)
            outs[with_db, acc] = (dW, db)
    return ref, outs


# ---- forward and input gradient: tile edges, NT = 1 --------------------------------------------------------------------
EDGE_SHAPES = [(1, 0, 1), (3, 0, 17), (20, 0, 33), (125, 5, 70)]          # K1, K2, N


@pytest.mark.parametrize("K1,K2,N", EDGE_SHAPES)
@pytest.mark.parametrize("B", [1, 15, 16, 17])
def test_fwd_tile_edges(orc, B, K1, K2, N):
    rng = np.random.default_rng(B * 1000 + N)
    K = K1 + K2
    x, x2 = rng.standard_normal((B, K1)).astype(F32), (rng.standard_normal((B, K2)).astype(F32) if K2 else None)
    W, b = _weight(rng, N, K, K), rng.standard_normal(N).astype(F32)
    for act in ACTS:
        got, = run_fwd([x], [W], [b], [act], [x2], expect=(1, K2 == 0 and K % 4 == 0))
        check_fwd(orc, got, x, W, b, act, x2)
    got, = run_fwd([x], [W], [None], ["none"], [x2], expect=(1, K2 == 0 and K % 4 == 0))      # no bias
    check_fwd(orc, got, x, W, None, "none", x2)


@pytest.mark.parametrize("K1,K2,N", EDGE_SHAPES)
@pytest.mark.parametrize("B", [1, 15, 16, 17])
def test_bwd_input_tile_edges(orc, B, K1, K2, N):
    """Two blocks: both, the first only (the second present: its stores must not happen), the second only."""
    rng = np.random.default_rng(B * 1000 + N + 1)
    K = K1 + K2
    dy, W = rng.standard_normal((B, N)).astype(F32), _weight(rng, N, K, K)
    for act in ACTS:
        y = _saved(rng, (B, N), act)
        ref = orc.lin_bwd_input(dy, y, W, ACT[act], LO, HI)
        for want in ([(True, True), (True, False), (False, True)] if K2 else [(True, True)]):
            got, = run_bwd_input([dy], [y], [W], [act], K1, want, expect=("mfma", 1, False))
            assert np.array_equal(got, _wanted(ref, K1, want), equal_nan=True), (act, want)


# ---- NT = 4 with a ragged last column group -----------------------------------------------------------------------------
B4 = 6555                 # 410 row tiles, the last of 11 rows; x 5 column tiles = 2050 > 2048 waves


def test_fwd_nt4_ragged_group(orc):
    K, N = 20, 70
    assert L.cdiv(B4, 16) == 410 and B4 % 16 == 11 and L.cdiv(N, 64) == 2 and N % 64 == 6
    rng = np.random.default_rng(40)
    x, W, b = rng.standard_normal((B4, K)).astype(F32), _weight(rng, N, K, K), rng.standard_normal(N).astype(F32)
    for act in ACTS:
        vec, = run_fwd([x], [W], [b], [act], expect=(4, True))
        sca, = run_fwd([x], [W], [b], [act], x_mode="col1", w_mode="off1", expect=(4, False))
        assert np.array_equal(vec, sca), act
        check_fwd(orc, vec, x, W, b, act)


def test_bwd_input_nt4_ragged_group(orc):
    N, K = 20, 70
    rng = np.random.default_rng(41)
    dy, W = rng.standard_normal((B4, N)).astype(F32), _weight(rng, N, K, K)
    for act in ACTS:
        y = _saved(rng, (B4, N), act)
        vec, = run_bwd_input([dy], [y], [W], [act], expect=("mfma", 4, True))
        sca, = run_bwd_input([dy], [y], [W], [act], mode="col1", w_mode="off1", expect=("mfma", 4, False))
        assert np.array_equal(vec, sca), act
        assert np.array_equal(vec, orc.lin_bwd_input(dy, y, W, ACT[act], LO, HI)), act


# ---- vector against scalar loads at one shape -----------------------------------------------------------------------------
VS = (37, 64, 48)         # B, K, N
LAYOUTS = [("aligned", True), ("ld4", True), ("ld1", False), ("off1", False)]


def test_fwd_vector_and_scalar_loads_same_bits(orc):
    B, K, N = VS
    rng = np.random.default_rng(50)
    x, W, b = rng.standard_normal((B, K)).astype(F32), _weight(rng, N, K, K), rng.standard_normal(N).astype(F32)
    for act in ACTS:
        runs = [run_fwd([x], [W], [b], [act], x_mode=m, expect=(1, v))[0] for m, v in LAYOUTS]
        runs.append(run_fwd([x], [W], [b], [act], w_mode="off1", expect=(1, False))[0])
        for r in runs[1:]:
            assert np.array_equal(r, runs[0]), act
        check_fwd(orc, runs[0], x, W, b, act)


def test_bwd_input_vector_and_scalar_loads_same_bits(orc):
    B, K, N = VS
    rng = np.random.default_rng(51)
    dy, W = rng.standard_normal((B, N)).astype(F32), _weight(rng, N, K, K)
    for act in ACTS:
        y = _saved(rng, (B, N), act)
        runs = [run_bwd_input([dy], [y], [W], [act], mode=m, expect=("mfma", 1, v))[0] for m, v in LAYOUTS]
        for r in runs[1:]:
            assert np.array_equal(r, runs[0]), act
        assert np.array_equal(runs[0], orc.lin_bwd_input(dy, y, W, ACT[act], LO, HI)), act


# ---- items per launch -------------------------------------------------------------------------------------------------
ITEM_ACTS = ["relu", "none", "clamp", "tanh"]


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_items_per_launch(orc, n):
    """1 .. GYMRL_LIN_MAX_ITEMS layers in one launch (the argument blocks are padded from item 0): each item is its own
    single-item launch and the oracle, in all three directions."""
    B, K, N = 33, 12, 20
    rng = np.random.default_rng(60 + n)
    acts = ITEM_ACTS[:n]
    xs = [rng.standard_normal((B, K)).astype(F32) for _ in acts]
    Ws = [_weight(rng, N, K, K) for _ in acts]
    bs = [rng.standard_normal(N).astype(F32) for _ in acts]
    dys = [rng.standard_normal((B, N)).astype(F32) for _ in acts]
    ys = [_saved(rng, (B, N), a) for a in acts]
    fw = run_fwd(xs, Ws, bs, acts, expect=(1, True))
    bi = run_bwd_input(dys, ys, Ws, acts, expect=("mfma", 1, True))
    path = ("tile", 1, 1, 64, 33)
    bw = run_bwd_weight(dys, ys, xs, acts, expect=path)
    for i, a in enumerate(acts):
        assert np.array_equal(fw[i], run_fwd([xs[i]], [Ws[i]], [bs[i]], [a], expect=(1, True))[0])
        check_fwd(orc, fw[i], xs[i], Ws[i], bs[i], a)
        assert np.array_equal(bi[i], run_bwd_input([dys[i]], [ys[i]], [Ws[i]], [a], expect=("mfma", 1, True))[0])
        assert np.array_equal(bi[i], orc.lin_bwd_input(dys[i], ys[i], Ws[i], ACT[a], LO, HI))
        (dW, db), = run_bwd_weight([dys[i]], [ys[i]], [xs[i]], [a], expect=path)
        assert np.array_equal(bw[i][0], dW) and np.array_equal(bw[i][1], db)
        rW, rb = orc.lin_bwd_weight(dys[i], ys[i], xs[i], 1, 64, ACT[a], LO, HI)
        assert np.array_equal(dW, rW) and np.array_equal(db, rb)


@pytest.mark.parametrize("B,N,K,nt", [(33, 64, 48, 1), (B4, 20, 70, 4)])
@pytest.mark.parametrize("n", [2, 4])
def test_bwd_input_summed_items(orc, B, N, K, nt, n):
    """sum_items: the items' chains run on into one another, on the vector path, mixed activations, ragged B."""
    rng = np.random.default_rng(70 + n + B)
    acts = ITEM_ACTS[:n]
    dys = [rng.standard_normal((B, N)).astype(F32) for _ in acts]
    ys = [_saved(rng, (B, N), a) for a in acts]
    Ws = [_weight(rng, N, K, K) for _ in acts]
    ref = orc.lin_bwd_input(dys, ys, Ws, [ACT[a] for a in acts], LO, HI)
    got, = run_bwd_input(dys, ys, Ws, acts, sum_items=True, expect=("mfma", nt, True))
    assert np.array_equal(got, ref)
    old = rng.standard_normal((B, K)).astype(F32)
    got, = run_bwd_input(dys, ys, Ws, acts, sum_items=True, old=old, expect=("mfma", nt, True))
    assert np.array_equal(got, old + ref)


# ---- accumulate into dx and dx2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K1,K2,nt", [(37, 48, 60, 4, 1), (B4, 20, 65, 5, 4)])
def test_bwd_input_accumulates_into_both_blocks(orc, B, N, K1, K2, nt):
    rng = np.random.default_rng(80 + B)
    K = K1 + K2
    dy, W = rng.standard_normal((B, N)).astype(F32), _weight(rng, N, K, K)
    old = rng.standard_normal((B, K)).astype(F32)
    for act in ACTS:
        y = _saved(rng, (B, N), act)
        ref = old + orc.lin_bwd_input(dy, y, W, ACT[act], LO, HI)
        assert np.array_equal(ref, orc.lin_bwd_input(dy, y, W, ACT[act], LO, HI, old=old))
        for want in ((True, True), (True, False), (False, True)):
            got, = run_bwd_input([dy], [y], [W], [act], K1, want, old=old, expect=("mfma", nt, True))
            assert np.array_equal(got, _wanted(ref, K1, want), equal_nan=True), (act, want)


# ---- the skinny VALU kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 4, 16, 17])
@pytest.mark.parametrize("B", [8192, 8193])
def test_bwd_input_skinny_threshold(orc, B, N):
    """B = 8192: the MFMA kernel; B = 8193 and N <= 16: the VALU kernel — each its own restatement (they differ in the last
    bits by design); N = 17 stays on the MFMA kernel.  Plain and accumulating."""
    K = 12
    rng = np.random.default_rng(90 + N)
    skinny = B > 8192 and N <= 16
    expect = ("skinny", None, None) if skinny else ("mfma", 1, N % 4 == 0)
    dy, W = rng.standard_normal((B, N)).astype(F32), _weight(rng, N, K, K)
    old = rng.standard_normal((B, K)).astype(F32)
    for act in ACTS:
        y = _saved(rng, (B, N), act)
        ref = orc.lin_bwd_input(dy, y, W, ACT[act], LO, HI, skinny=skinny)
        got, = run_bwd_input([dy], [y], [W], [act], compact=True, expect=expect)
        assert np.array_equal(got, ref), act
        got, = run_bwd_input([dy], [y], [W], [act], compact=True, old=old, expect=expect)
        assert np.array_equal(got, old + ref), act


def test_bwd_input_skinny_past_the_grid_cap(orc):
    """B * K / 4 threads are 20 more than 16384 blocks of 256: the last rows are written by the grid-stride loop's second
    trip.  2048 rows against the oracle (the first and last 64, those around the wrap, the rest at random), all for NaN."""
    from gymrl_amd import ops
    N, K = 4, 12
    B = 16384 * 256 // 3 + 7
    assert L.skinny_blocks(B, K) == (16384, 16385) and L.bwd_input_path(B, N, K, K, N)[0] == "skinny"
    wrap = 16384 * 256 // 3                                # the row the first thread of the second trip writes
    rng = np.random.default_rng(95)
    rows = np.unique(np.concatenate([np.arange(64), np.arange(B - 64, B), np.arange(wrap - 40, min(B, wrap + 8))]))
    rest = rng.choice(np.setdiff1d(np.arange(B), rows), 2048 - rows.size, replace=False)
    rows = np.sort(np.concatenate([rows, rest]))
    assert rows.size == 2048
    g = torch.Generator(device=D).manual_seed(95)
    dy = torch.randn(B, N, device=D, generator=g)
    z = torch.randn(B, N, device=D, generator=g)
    W = _weight(rng, N, K, K)
    tw = torch.from_numpy(W).to(D)
    buf, dx = L.guarded(torch, B, K, D, col_guard=False)
    ridx = torch.from_numpy(rows).to(D)
    for act in ACTS:
        y = {"none": z, "relu": torch.relu(z), "tanh": torch.tanh(z), "clamp": z.clamp(LO, HI)}[act]
        buf.fill_(NAN)
        assert _al(dx, tw, dy, y) and _ld(dx) % 4 == 0
        ops.lin_bwd_input(dy, y, tw, ACT[act], dx=dx, lo=LO, hi=HI)
        assert L.guards_intact(torch, buf, (B, K), col_guard=False), act
        ref = orc.lin_bwd_input(_np(dy[ridx]), _np(y[ridx]), W, ACT[act], LO, HI, skinny=True)
        assert np.array_equal(_np(dx[ridx]), ref), act


# ---- the DUELING epilogue ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 64])
@pytest.mark.parametrize("B", [1, 17, 100])
@pytest.mark.parametrize("A", [1, 2, 3, 15])
def test_dueling_epilogue(orc, A, B, K):
    """q and the greedy action bit for bit against lin_ref.dueling on the oracle's z; two and all advantages tied (copied
    weight rows and biases): the first index wins.  The argmax buffer is guarded too."""
    from gymrl_amd import ops
    rng = np.random.default_rng(A * 100 + B + K)
    x = rng.standard_normal((B, K)).astype(F32)
    for tie in ("none", "two", "all"):
        if tie != "none" and A == 1:
            continue
        W, b = _weight(rng, A + 1, K, K), rng.standard_normal(A + 1).astype(F32)
        if tie == "two":
            W[A - 1], b[A - 1] = W[0], b[0]
        if tie == "all":
            W[:A], b[:A] = W[0], b[0]
        q_ref, am_ref = L.dueling(orc.linear_act(x, W, b, 0), A)
        if tie == "all":
            assert (am_ref == 0).all()
        tx, tw, tb = _place(x), _place(W), _place(b)
        assert L.fwd_path(B, K, K, A + 1, _ld(tx), _al(tx, tw)) == (1, K % 4 == 0)
        qb, q = L.guarded(torch, B, A, D)
        ab, am = L.guarded_vec(torch, B, D, dtype=torch.int32, sentinel=-7)
        ops.lin_fwd(tx, tw, tb, ACT["dueling"], out=q, argmax=am)
        assert L.guards_intact(torch, qb, (B, A)) and L.guards_intact(torch, ab, (B,), sentinel=-7)
        assert np.array_equal(_np(q), q_ref), tie
        assert np.array_equal(_np(am), am_ref), tie
        qb2, q2 = L.guarded(torch, B, A, D)                         # without an argmax buffer: the same q
        ops.lin_fwd(tx, tw, tb, ACT["dueling"], out=q2)
        assert L.guards_intact(torch, qb2, (B, A)) and np.array_equal(_np(q2), q_ref)


# ---- SiLU -------------------------------------------------------------------------------------------------------------
def test_fwd_silu(orc, capsys):
    """y against float64 z / (1 + exp(-z)) of the bit-pinned float32 pre-activation z.  The yardstick is the reference, not
    the kernel: at most twice the largest error of torch's silu on the same z on the device, plus one float32 ulp of the
    largest output."""
    from gymrl_amd import ops
    B, K, N = VS
    rng = np.random.default_rng(110)
    x, W, b = rng.standard_normal((B, K)).astype(F32), _weight(rng, N, K, K), (2 * rng.standard_normal(N)).astype(F32)
    z, = run_fwd([x], [W], [b], ["none"], expect=(1, True))
    assert np.array_equal(z, L.fwd(orc, x, W, b, ACT["none"]))
    buf, y = L.guarded(torch, B, N, D)
    ops.lin_fwd(_place(x), _place(W), _place(b), ACT["silu"], out=y)
    assert L.guards_intact(torch, buf, (B, N))
    z64 = z.astype(np.float64)
    exact = z64 / (1.0 + np.exp(-z64))
    err_kernel = float(np.abs(_np(y).astype(np.float64) - exact).max())
    err_torch = float(np.abs(_np(torch.nn.functional.silu(torch.from_numpy(z).to(D))).astype(np.float64) - exact).max())
    ulp = float(np.spacing(F32(np.abs(exact).max())))
    with capsys.disabled():
        print(f"\nsilu: kernel max error {err_kernel:.3e}, torch max error {err_torch:.3e}, ulp of the largest output {ulp:.3e}")
    assert err_kernel <= 2 * err_torch + ulp, (err_kernel, err_torch, ulp)


# ---- weight gradient: one slice ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K1,K2", [(1, 1, 0), (17, 3, 0), (70, 125, 5)])
@pytest.mark.parametrize("B", [1, 16, 17, 127, 128, 129, 512])
def test_bwd_weight_one_slice(orc, B, N, K1, K2):
    rng = np.random.default_rng(B * 100 + N)
    K = K1 + K2
    expect = ("tile", 1, 1, L.cdiv(B, 32) * 32, B)
    dy = rng.standard_normal((B, N)).astype(F32)
    x, x2 = rng.standard_normal((B, K1)).astype(F32), (rng.standard_normal((B, K2)).astype(F32) if K2 else None)
    for act in ACTS:
        check_bwd_weight_variants(orc, dy, _saved(rng, (B, N), act), x, act, expect, x2)


# ---- weight gradient: slice seams of the 16 x 16 kernel and the reduce ------------------------------------------------------
@pytest.mark.parametrize("B,N,K,slices,rps,last,groups", [
    (513, 16, 16, 3, 192, 129, [1, 1, 1, 0, 0, 0, 0, 0]),            # the last slice: eight full 16-row steps and one row
    (2305, 16, 16, 10, 256, 1, [2, 2, 2, 2, 2, 0, 0, 0]),            # empty reduce groups, a last slice of one row
    (4097, 3, 5, 17, 256, 1, [3, 3, 3, 3, 3, 2, 0, 0]),              # a short group
])
def test_bwd_weight_slice_seams(orc, B, N, K, slices, rps, last, groups):
    assert L.reduce_groups(slices) == groups and last == B - (slices - 1) * rps
    rng = np.random.default_rng(B)
    dy, x = rng.standard_normal((B, N)).astype(F32), rng.standard_normal((B, K)).astype(F32)
    for act in ACTS:
        check_bwd_weight_variants(orc, dy, _saved(rng, (B, N), act), x, act, ("tile", 1, slices, rps, last))


@pytest.mark.parametrize("shape", ["smallest", "two_row_tiles"])
def test_bwd_weight_tile_kernel_nt4(orc, shape):
    """tiles x slices > 4096 with K no multiple of 64: 16 x 64 tiles per wave with a ragged last column group.  The smallest
    such shape has one row of dW; the second has two row tiles, the last of one row."""
    B, N, K = L.smallest_weight_nt4() if shape == "smallest" else (3841, 17, 2049)
    assert B <= 8192 and K % 64 != 0
    expect = ("tile", 4, 16, 256, 1)
    assert L.bwd_weight_path(B - 1, N, K)[1] == 1
    rng = np.random.default_rng(B + N)
    dy, x = rng.standard_normal((B, N)).astype(F32), rng.standard_normal((B, K)).astype(F32)
    for act in ("none", "relu"):
        check_bwd_weight_variants(orc, dy, _saved(rng, (B, N), act), x, act, expect)


# ---- weight gradient: the 64 x 64-block kernels -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _big_case(B, N, K):
    """Data and the oracle's dW, db of a big shape, shared by the tests that launch it (the oracle walks B N K fmaf)."""
    from oracle import oracle
    rng = np.random.default_rng(B + N + K)
    dy, x = rng.standard_normal((B, N)).astype(F32), rng.standard_normal((B, K)).astype(F32)
    _, _, slices, rps, _ = L.bwd_weight_path(B, N, K)
    ref = oracle.lin_bwd_weight(dy, None, x, slices, rps)
    for a in (dy, x, *ref):
        a.setflags(write=False)
    return dy, x, ref


@pytest.mark.parametrize("B,slices,last,batches,partial", [
    (16384, 64, 256, 16, False),         # every slice an even count of 16-row batches: the loop's second exit
    (16385, 65, 1, 1, True),             # a last slice of one row: the first exit, a partial batch
    (16400, 65, 16, 1, False),           # odd, the batch full
    (16404, 65, 20, 2, True),            # even, the last batch partial
])
def test_bwd_weight_big_kernel(orc, B, slices, last, batches, partial):
    N, K = 64, 192
    assert not L.bwd_weight_lds(N, K) and L.slice_batches(last) == (batches, partial) and L.slice_batches(256) == (16, False)
    dy, x, ref = _big_case(B, N, K)
    check_bwd_weight_variants(orc, dy, None, x, "none", ("big", None, slices, 256, last), ref=ref)


def test_bwd_weight_big_kernel_fallback(orc):
    """The big shape's data with dy a column slice one float off alignment, and again aligned with relu: both take the
    16 x 16 kernel with the big shape's slice count.  The no-activation fallback is the big kernel's output bit for bit."""
    B, N, K = 16385, 64, 192
    dy, x, ref = _big_case(B, N, K)
    (bW, bb), = run_bwd_weight([dy], [None], [x], ["none"], expect=("big", None, 65, 256, 1))
    _, outs = check_bwd_weight_variants(orc, dy, None, x, "none", ("tile", 1, 65, 256, 1), ref=ref, dy_mode="col1")
    assert np.array_equal(outs[True, False][0], bW) and np.array_equal(outs[True, False][1], bb)
    rng = np.random.default_rng(7)
    y = _saved(rng, (B, N), "relu")
    (dW, db), = run_bwd_weight([dy], [y], [x], ["relu"], expect=("tile", 1, 65, 256, 1))
    rW, rb = orc.lin_bwd_weight(dy, y, x, 65, 256, ACT["relu"])
    assert np.array_equal(dW, rW) and np.array_equal(db, rb)


@pytest.mark.parametrize("N,K,kernel", [(64, 192, "big"), (128, 128, "big_lds")])
@pytest.mark.parametrize("n", [2, 4])
def test_bwd_weight_big_kernel_items(n, N, K, kernel):
    B = 16385
    rng = np.random.default_rng(n + N)
    expect = (kernel, None, 65, 256, 1)
    dys = [rng.standard_normal((B, N)).astype(F32) for _ in range(n)]
    xs = [rng.standard_normal((B, K)).astype(F32) for _ in range(n)]
    both = run_bwd_weight(dys, [None] * n, xs, ["none"] * n, expect=expect)
    for i in range(n):
        (dW, db), = run_bwd_weight([dys[i]], [None], [xs[i]], ["none"], expect=expect)
        assert np.array_equal(both[i][0], dW) and np.array_equal(both[i][1], db)


def _store_map_rows():
    """32 rows of a 128-row dW covering both 64-row halves, every i (0..3) and every 4q + g (0..15) of the store map
    n0 + 4 (4q + g) + i."""
    rows = [64 * (j % 2) + 4 * (j % 16) + (j // 8) % 4 for j in range(32)]
    assert len(set(rows)) == 32 and {r // 64 for r in rows} == {0, 1}
    assert {r % 4 for r in rows} == {0, 1, 2, 3} and {(r % 64) // 4 for r in rows} == set(range(16))
    return np.array(sorted(rows))


@pytest.mark.parametrize("B,last,batches,partial", [(16385, 1, 1, True), (16404, 20, 2, True), (16640, 256, 16, False)])
def test_bwd_weight_lds_kernel(orc, B, last, batches, partial):
    """N = K = 128: the oracle on all of db and on 32 rows of dW chosen over the store map; every other row to float64 with
    the derived bound gamma_n sum |terms|, n = the slice's rows + the reduce's adds (+ the accumulate) + 1."""
    N = K = 128
    slices = 65
    expect = ("big_lds", None, slices, 256, last)
    assert L.slice_batches(last) == (batches, partial)
    rng = np.random.default_rng(B)
    dy, x = rng.standard_normal((B, N)).astype(F32), rng.standard_normal((B, K)).astype(F32)
    rows = _store_map_rows()
    rW, _ = orc.lin_bwd_weight(dy[:, rows], None, x, slices, 256, want_db=False)
    _, rb = orc.lin_bwd_weight(dy, None, x[:, :1], slices, 256)
    exact = dy.astype(np.float64).T @ x.astype(np.float64)
    mag = np.abs(dy.astype(np.float64)).T @ np.abs(x.astype(np.float64))
    old = (rng.standard_normal((N, K)).astype(F32), rng.standard_normal(N).astype(F32))
    for with_db in (True, False):
        for acc in (False, True):
            (dW, db), = run_bwd_weight([dy], [None], [x], ["none"], with_db=with_db, old=old if acc else None, expect=expect)
            assert np.array_equal(dW[rows], old[0][rows] + rW if acc else rW), (with_db, acc)
            if with_db:
                assert np.array_equal(db, old[1] + rb if acc else rb), (with_db, acc)
            n = 256 + L.cdiv(slices, 8) + 7 + int(acc) + 1
            want = exact + old[0] if acc else exact
            bound = L.gamma(n) * (mag + np.abs(old[0]) if acc else mag)
            assert (np.abs(dW - want) <= bound).all(), (with_db, acc)
