"""The oracle's restatement of lin.hip's backward launches (orc_lin_bwd_input, _skinny, orc_lin_bwd_weight) and
tests/lin_ref.py's geometry, on the CPU.

The new chains are held to float64 at the seam shapes of tests/test_lin_seams_gpu.py with a derived per-element bound:
|got - exact| <= gamma_n * sum |terms|, gamma_n = n u / (1 - n u), u = 2^-24, n = the float32 roundings on the
element's path (chain length + reduce adds + accumulate + one for dz; dz itself is formed in float32 by lin_ref's
restatement of act_bwd, which one test pins to the oracle bit for bit).  Structure is checked exactly: a lone slice is a
plain ascending fmaf chain, slices commute only inside a reduce group, summed items are one chain.
"""
import math

import numpy as np
import pytest

import lin_ref as L
from lin_ref import ACT, F32

LO, HI = -0.7, 0.9
ACTS = ["none", "relu", "tanh", "clamp"]


def _saved(rng, shape, act):
    z = rng.standard_normal(shape).astype(F32)
    if act == "relu":
        return np.maximum(z, F32(0))
    if act == "tanh":
        return np.tanh(z).astype(F32)
    if act == "clamp":
        return np.minimum(np.maximum(z, F32(LO)), F32(HI))
    return z


def _fma_chain(terms_a, terms_b):
    """acc = fmaf(a_i, b_i, acc) from +0 over axis 0 in float32, each step evaluated exactly in rationals and rounded once
    (float64 arithmetic would round twice)."""
    from fractions import Fraction
    acc = np.zeros(terms_a.shape[1:], F32)
    flat = acc.reshape(-1)
    A, Bm = terms_a.reshape(terms_a.shape[0], -1), terms_b.reshape(terms_b.shape[0], -1)
    for j in range(flat.size):
        v = F32(0)
        for i in range(A.shape[0]):
            exact = Fraction(float(A[i, j])) * Fraction(float(Bm[i, j])) + Fraction(float(v))
            v = _round_f32(exact)
        flat[j] = v
    return acc


def _round_f32(fr):
    """Round a Fraction to the nearest float32 (ties to even)."""
    d = float(fr)                     # correctly rounded to float64
    f = F32(d)
    from fractions import Fraction
    if Fraction(float(f)) == fr:
        return f
    # candidates: f and its neighbour on the other side of fr
    other = np.nextafter(f, F32(np.inf) if Fraction(float(f)) < fr else F32(-np.inf))
    ef, eo = abs(Fraction(float(f)) - fr), abs(Fraction(float(other)) - fr)
    if ef < eo:
        return f
    if eo < ef:
        return other
    return f if (f.view(np.uint32) & 1) == 0 else other


def test_act_bwd_restatement_is_the_oracles(oracle):
    """N = 1, W = 1: dX = fmaf(dz, 1, +0) = dz, so the oracle's dz is lin_ref.dz_f32's bit for bit — relu's exact zeros at
    y = 0, clamp's strict bounds at y = lo and y = hi, tanh as 1 - y * y with two roundings."""
    rng = np.random.default_rng(0)
    for act in ACTS:
        y = _saved(rng, (4096, 1), act)
        dy = rng.standard_normal((4096, 1)).astype(F32)
        if act == "clamp":
            assert (y == F32(LO)).any() and (y == F32(HI)).any()
        if act == "relu":
            assert (y == 0).any()
        want = L.dz_f32(dy, y, ACT[act], LO, HI)
        one = np.ones((1, 1), F32)
        assert np.array_equal(oracle.lin_bwd_input(dy, y, one, ACT[act], LO, HI), want)
        assert np.array_equal(oracle.lin_bwd_input(dy, y, one, ACT[act], LO, HI, skinny=True), want)
        dW, db = oracle.lin_bwd_weight(dy[:1], y[:1], np.ones((1, 1), F32), 1, 32, ACT[act], LO, HI)
        assert np.array_equal(dW, want[:1]) and np.array_equal(db, want[0])


def test_bwd_input_order_is_the_documented_one(oracle):
    """n0 = 0, 16, ...; e; q: n = n0 + 4q + e, against an exactly rounded chain in that order — and NOT the ascending one
    (the data make the two differ); the skinny restatement is ascending multiply-then-add."""
    rng = np.random.default_rng(1)
    N, K = 21, 3
    dy = (rng.standard_normal((2, N)) * 10.0 ** rng.integers(-3, 4, (2, N))).astype(F32)
    W = rng.standard_normal((N, K)).astype(F32)
    order = [n0 + 4 * q + e for n0 in range(0, N, 16) for e in range(4) for q in range(4) if n0 + 4 * q + e < N]
    assert sorted(order) == list(range(N))
    got = oracle.lin_bwd_input(dy, None, W)
    want = _fma_chain(dy.T[order][:, :, None].repeat(K, 2), W[order][:, None, :].repeat(2, 1))
    assert np.array_equal(got, want)
    asc = _fma_chain(dy.T[:, :, None].repeat(K, 2), W[:, None, :].repeat(2, 1))
    assert not np.array_equal(asc, want)
    sk = np.zeros((2, K), F32)
    for n in range(N):
        sk = sk + dy[:, n:n + 1] * W[n:n + 1]
    assert np.array_equal(oracle.lin_bwd_input(dy, None, W, skinny=True), sk)
    assert not np.array_equal(sk, want)


def test_one_slice_is_a_plain_ascending_chain(oracle):
    rng = np.random.default_rng(2)
    B, N, K = 37, 3, 2
    dy = (rng.standard_normal((B, N)) * 10.0 ** rng.integers(-3, 4, (B, N))).astype(F32)
    x = rng.standard_normal((B, K)).astype(F32)
    dW, db = oracle.lin_bwd_weight(dy, None, x, 1, L.bwd_weight_rows_per_slice(B, 1))
    want = _fma_chain(dy[:, :, None].repeat(K, 2), x[:, None, :].repeat(N, 1))
    assert np.array_equal(dW, want)
    c = [np.zeros(N, F32) for _ in range(4)]
    for m in range(B):
        c[m & 3] = c[m & 3] + dy[m]
    assert np.array_equal(db, (c[0] + c[1]) + (c[2] + c[3]))


@pytest.mark.parametrize("B,N,K,slices,rps", [(513, 16, 16, 3, 192), (2305, 16, 16, 10, 256), (4097, 3, 5, 17, 256)])
def test_slices_commute_only_inside_a_reduce_group(oracle, B, N, K, slices, rps):
    """Swapping the two slices of one reduce group of two leaves dW and db unchanged (a + b = b + a from 0); swapping slices
    of different groups changes the order of the group sums."""
    assert L.bwd_weight_path(B, N, K)[2:4] == (slices, rps)
    rng = np.random.default_rng(B)
    Bf = slices * rps                              # whole slices only, so that rows can be permuted slice-wise
    dy = (rng.standard_normal((Bf, N)) * 10.0 ** rng.integers(-2, 3, (Bf, N))).astype(F32)
    x = rng.standard_normal((Bf, K)).astype(F32)
    base = oracle.lin_bwd_weight(dy, None, x, slices, rps)
    groups = L.reduce_groups(slices)
    each = L.cdiv(slices, 8)

    def swapped(a, b):
        idx = np.arange(Bf).reshape(slices, rps)
        idx[[a, b]] = idx[[b, a]]
        idx = idx.reshape(-1)
        return oracle.lin_bwd_weight(dy[idx], None, x[idx], slices, rps)

    if each == 2:
        for g, n in enumerate(groups):
            if n == 2:
                got = swapped(2 * g, 2 * g + 1)
                assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
    if each <= 2:                                    # across groups: the sum is reordered, some element must move
        got = swapped(0, slices - 1)
        assert not np.array_equal(got[0], base[0])
    # and the stated order itself: groups of `each` consecutive slices from 0, then the groups in turn
    parts = [oracle.lin_bwd_weight(dy[s * rps:(s + 1) * rps], None, x[s * rps:(s + 1) * rps], 1, rps) for s in range(slices)]
    for j in (0, 1):
        tot = None
        for g in range(8):
            s = np.zeros_like(parts[0][j])
            for k in range(g * each, min(slices, (g + 1) * each)):
                s = s + parts[k][j]
            tot = s if tot is None else tot + s
        assert np.array_equal(tot, base[j])


def test_summed_items_are_one_chain(oracle):
    rng = np.random.default_rng(3)
    B, N, K = 33, 20, 7
    acts = ["none", "clamp", "relu", "tanh"]
    dys = [rng.standard_normal((B, N)).astype(F32) for _ in acts]
    ys = [_saved(rng, (B, N), a) for a in acts]
    Ws = [rng.standard_normal((N, K)).astype(F32) for _ in acts]
    got = oracle.lin_bwd_input(dys, ys, Ws, [ACT[a] for a in acts], LO, HI)
    # one item whose reduction is the items' reductions one after another, each padded to whole 16-steps so that the
    # (n0, e, q) walk of the concatenation visits the items' terms in the items' own order
    pad = L.cdiv(N, 16) * 16
    dz = np.zeros((B, pad * len(acts)), F32)
    Wc = np.zeros((pad * len(acts), K), F32)
    for i, a in enumerate(acts):
        dz[:, i * pad:i * pad + N] = L.dz_f32(dys[i], ys[i], ACT[a], LO, HI)
        Wc[i * pad:i * pad + N] = Ws[i]
    assert np.array_equal(got, oracle.lin_bwd_input(dz, None, Wc))
    old = rng.standard_normal((B, K)).astype(F32)
    assert np.array_equal(oracle.lin_bwd_input(dys, ys, Ws, [ACT[a] for a in acts], LO, HI, old=old), old + got)


INPUT_SEAMS = [(1, 1, 1), (15, 17, 3), (16, 33, 20), (17, 70, 130), (37, 48, 64), (33, 64, 48), (257, 20, 70), (300, 16, 12)]


@pytest.mark.parametrize("B,N,K", INPUT_SEAMS)
@pytest.mark.parametrize("act", ACTS)
def test_bwd_input_against_float64(oracle, B, N, K, act):
    rng = np.random.default_rng(B * 131 + N)
    dy = rng.standard_normal((B, N)).astype(F32)
    y = _saved(rng, (B, N), act)
    W = (rng.standard_normal((N, K)) / math.sqrt(N) * (1 + np.arange(K) / K)).astype(F32)
    old = rng.standard_normal((B, K)).astype(F32)
    dz = L.dz_f32(dy, y, ACT[act], LO, HI).astype(np.float64)
    exact = dz @ W.astype(np.float64)
    mag = np.abs(dz) @ np.abs(W.astype(np.float64))
    for skinny in (False, True):
        if skinny and N > L.SKINNY_N:
            continue
        n = (2 * N if skinny else N) + 1           # the skinny chain rounds the product and the sum
        got = oracle.lin_bwd_input(dy, y, W, ACT[act], LO, HI, skinny=skinny)
        assert (np.abs(got - exact) <= L.gamma(n) * mag).all()
        acc = oracle.lin_bwd_input(dy, y, W, ACT[act], LO, HI, old=old, skinny=skinny)
        assert np.array_equal(acc, old + got)
    two = oracle.lin_bwd_input([dy, dy[::-1].copy()], [y, y[::-1].copy()], [W, W[::-1].copy()], ACT[act], LO, HI)
    dz2 = dz[::-1]
    exact2 = exact + dz2 @ W[::-1].astype(np.float64)
    mag2 = mag + np.abs(dz2) @ np.abs(W[::-1].astype(np.float64))
    assert (np.abs(two - exact2) <= L.gamma(2 * N + 1) * mag2).all()


WEIGHT_SEAMS = [(1, 1, 1), (17, 17, 3), (129, 70, 130), (512, 17, 3), (513, 16, 16), (2305, 16, 16), (4097, 3, 5),
                (16385, 64, 4), (16400, 64, 4), (16404, 64, 4)]


@pytest.mark.parametrize("B,N,K", WEIGHT_SEAMS)
@pytest.mark.parametrize("act", ["none", "tanh", "clamp"])
def test_bwd_weight_against_float64(oracle, B, N, K, act):
    """The last three shapes run the big kernels' cut (N = 64, K = 192) on four columns of X: the cut depends on the
    launch's shape, the chain on the rows only."""
    rng = np.random.default_rng(B * 17 + N)
    cut_K = 192 if B >= 16384 else K
    _, _, slices, rps, last = L.bwd_weight_path(B, N, cut_K)
    assert 1 <= last <= rps
    dy = rng.standard_normal((B, N)).astype(F32)
    y = _saved(rng, (B, N), act)
    x = (rng.standard_normal((B, K)) + 0.25).astype(F32)
    dz = L.dz_f32(dy, y, ACT[act], LO, HI).astype(np.float64)
    x64 = x.astype(np.float64)
    reduce_adds = 0 if slices == 1 else L.cdiv(slices, 8) + 7
    n = min(B, rps) + reduce_adds + 1
    dW, db = oracle.lin_bwd_weight(dy, y, x, slices, rps, ACT[act], LO, HI)
    assert (np.abs(dW - dz.T @ x64) <= L.gamma(n) * (np.abs(dz).T @ np.abs(x64))).all()
    # db: a serial sum of a quarter of the slice's rows, two pairwise adds, the reduce
    n_db = L.cdiv(min(B, rps), 4) + 2 + reduce_adds + 1
    assert (np.abs(db - dz.sum(0)) <= L.gamma(n_db) * np.abs(dz).sum(0)).all()
    old_w, old_b = rng.standard_normal((N, K)).astype(F32), rng.standard_normal(N).astype(F32)
    aW, ab = oracle.lin_bwd_weight(dy, y, x, slices, rps, ACT[act], LO, HI, old_dw=old_w, old_db=old_b)
    assert np.array_equal(aW, old_w + dW) and np.array_equal(ab, old_b + db)
    nW, nb = oracle.lin_bwd_weight(dy, y, x, slices, rps, ACT[act], LO, HI, want_db=False)
    assert nb is None and np.array_equal(nW, dW)


def test_dueling_restatement():
    """lin_ref.dueling against float64 (the mean of A float32 numbers in a 4-level tree, a division, two adds: 7 roundings)
    and its structure: the tree is NOT the serial sum, ties go to the first index, A = 1 gives q = v + (z - z)."""
    rng = np.random.default_rng(5)
    for A in (1, 2, 3, 15):
        z = (rng.standard_normal((200, A + 1)) * 3).astype(F32)
        z[:50, 1:A] = z[:50, :1]                       # all advantages tied
        q, am = L.dueling(z, A)
        z64 = z.astype(np.float64)
        exact = z64[:, A:] + z64[:, :A] - z64[:, :A].mean(1, keepdims=True)
        mag = np.abs(z64[:, A:]) + np.abs(z64[:, :A]) + np.abs(z64[:, :A]).mean(1, keepdims=True)
        assert (np.abs(q - exact) <= L.gamma(7) * mag).all()
        assert (am[:50] == 0).all()
        assert (q[np.arange(200), am] == q.max(1)).all()
        if A == 1:
            assert np.array_equal(q, z[:, 1:])
    z = np.array([[1e8, 1.0, -1e8, 1.0, 1.0, 0.0]], F32)      # ((a + b) + (c + d)) + e, not (((a + b) + c) + d) + e
    q, _ = L.dueling(z, 5)
    tree = ((F32(1e8) + F32(1)) + (F32(-1e8) + F32(1))) + ((F32(1) + F32(0)) + F32(0))
    assert q[0, 0] == F32(0) + (F32(1e8) - tree / F32(5))


def test_geometry_figures_of_the_seam_cases():
    assert L.pick_nt(L.cdiv(6555, 16), 70) == 4 and L.cdiv(6555, 16) == 410 and 6555 - 409 * 16 == 11
    assert L.pick_nt(L.cdiv(6555, 16), 20) == 1 and L.pick_nt(410, 64) == 1 and L.pick_nt(1000, 16) == 1
    assert L.fwd_path(37, 64, 64, 48, 64) == (1, True) and L.fwd_path(37, 64, 64, 48, 65) == (1, False)
    assert L.fwd_path(37, 64, 64, 48, 68) == (1, True) and L.fwd_path(37, 64, 64, 48, 64, aligned=False) == (1, False)
    assert L.fwd_path(17, 130, 125, 70, 125) == (1, False)
    assert L.bwd_input_path(8192, 4, 12, 12, 4) == ("mfma", 1, True)
    assert L.bwd_input_path(8193, 4, 12, 12, 4)[0] == "skinny" and L.bwd_input_path(8193, 1, 12, 12, 1)[0] == "skinny"
    assert L.bwd_input_path(8193, 17, 12, 12, 17) == ("mfma", 1, False)
    assert L.bwd_input_path(8193, 4, 12, 12, 4, sum_items=True, n_items=2)[0] == "mfma"
    B = 16384 * 256 // 3 + 7
    assert L.skinny_blocks(B, 12) == (16384, 16385)
    assert L.bwd_weight_path(512, 70, 130) == ("tile", 1, 1, 512, 512)
    assert L.bwd_weight_path(513, 16, 16) == ("tile", 1, 3, 192, 129)
    assert L.bwd_weight_path(2305, 16, 16) == ("tile", 1, 10, 256, 1) and L.reduce_groups(10) == [2, 2, 2, 2, 2, 0, 0, 0]
    assert L.bwd_weight_path(4097, 3, 5) == ("tile", 1, 17, 256, 1) and L.reduce_groups(17) == [3, 3, 3, 3, 3, 2, 0, 0]
    assert L.bwd_weight_path(16384, 64, 192) == ("big", None, 64, 256, 256)
    assert L.bwd_weight_path(16385, 64, 192) == ("big", None, 65, 256, 1)
    assert L.bwd_weight_path(16385, 128, 128) == ("big_lds", None, 65, 256, 1)
    assert L.bwd_weight_path(16385, 64, 192, aligned=False) == ("tile", 1, 65, 256, 1)
    assert L.bwd_weight_path(16385, 64, 192, act=2) == ("tile", 1, 65, 256, 1)
    assert L.bwd_weight_path(16383, 64, 192)[0] == "tile"
    assert L.slice_batches(256) == (16, False) and L.slice_batches(1) == (1, True)
    assert L.slice_batches(16) == (1, False) and L.slice_batches(20) == (2, True)
    B, N, K = L.smallest_weight_nt4()
    kernel, nt, slices, _, _ = L.bwd_weight_path(B, N, K)
    assert (kernel, nt) == ("tile", 4) and K % 64 != 0 and B <= 8192 and L.cdiv(N, 16) * L.cdiv(K, 16) * slices > 4096
    assert L.bwd_weight_path(B - 1, N, K)[1] == 1


def test_geometry_agrees_with_the_library():
    """lin_ref's slice count against gymrl_lin_workspace_bytes (a host function: no GPU needed) over a sweep of shapes."""
    from gymrl_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(7)
    shapes = [(b, n, k) for b in (1, 512, 513, 600, 2305, 4097, 4200, 8192, 16383, 16384, 16385, 40013, 262144)
              for n, k in ((1, 1), (3, 5), (16, 16), (17, 3), (70, 130), (64, 192), (128, 128), (256, 256), (1, 4097), (64, 64))]
    shapes += [tuple(int(v) for v in rng.integers(1, (70000, 300, 300))) for _ in range(300)]
    for B, N, K in shapes:
        for items in (1, 4):
            nbytes = lib.gymrl_lin_workspace_bytes(B, N, K, items)
            assert L.slices_from_workspace(nbytes, items, N, K) == L.bwd_weight_slices(B, N, K), (B, N, K)
        s = L.bwd_weight_slices(B, N, K)
        rps = L.bwd_weight_rows_per_slice(B, s)
        assert rps % 32 == 0 and s * rps >= B
