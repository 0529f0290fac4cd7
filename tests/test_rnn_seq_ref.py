"""CPU checks of tests/rnn_seq_ref.py: the explicit float64 loops against float64 torch.nn.GRU / nn.LSTM under autograd
(one row at a time, W_ih = I so that the input projection IS gi), and every input generator of
tests/test_rnn_seq_edges_gpu.py against the property it states."""
import numpy as np
import pytest

import rnn_seq_ref as R
from conftest import rel_close

torch = pytest.importorskip("torch")


def _nn_ref(kind, c, absent):
    """float64 nn.GRU / nn.LSTM, one unbatched row per call; a length-0 row runs nothing: its state and gradient pass."""
    T, B, HG = c["gi"].shape
    G = R.GATES[kind]
    H = HG // G
    net = (torch.nn.GRU if kind == "gru" else torch.nn.LSTM)(HG, H).double()
    with torch.no_grad():
        net.weight_ih_l0.copy_(torch.eye(HG, dtype=torch.float64))
        net.bias_ih_l0.zero_()
        net.weight_hh_l0.copy_(torch.from_numpy(c["W"]).double())
        net.bias_hh_l0.copy_(torch.from_numpy(c["b"]).double())
    net.weight_ih_l0.requires_grad_(False)
    net.bias_ih_l0.requires_grad_(False)
    op = {k: (np.zeros_like(c[k]) if k in absent else c[k]).astype(np.float64) for k in R.OPERANDS[kind]}
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))  # noqa: E731
    r = {"h_seq": np.zeros((T, B, H)), "h_last": op["h0"].copy(), "dh0": op["d_hlast"].copy()}
    if kind == "gru":
        r["dgi"] = np.zeros((T, B, HG))
    else:
        r.update(c_seq=np.zeros((T, B, H)), c_last=op["c0"].copy(), dgates=np.zeros((T, B, HG)), dc0=op["d_clast"].copy())
    for e, n in enumerate(c["lens"]):
        if n == 0:
            continue
        x = f64(c["gi"][:n, e]).requires_grad_(True)
        hh = f64(op["h0"][e:e + 1]).requires_grad_(True)
        if kind == "gru":
            out, hl = net(x, hh)
            loss = (out * f64(op["d_hseq"][:n, e])).sum() + (hl[0] * f64(op["d_hlast"][e])).sum()
        else:
            cc = f64(op["c0"][e:e + 1]).requires_grad_(True)
            out, (hl, cl) = net(x, (hh, cc))
            loss = (out * f64(op["d_hseq"][:n, e])).sum() + (hl[0] * f64(op["d_hlast"][e])).sum() + \
                (cl[0] * f64(op["d_clast"][e])).sum()
        loss.backward()
        r["h_seq"][:n, e], r["h_last"][e], r["dh0"][e] = out.detach().numpy(), hl[0].detach().numpy(), hh.grad[0].numpy()
        if kind == "gru":
            r["dgi"][:n, e] = x.grad.numpy()
        else:
            r["dgates"][:n, e], r["c_last"][e], r["dc0"][e] = x.grad.numpy(), cl[0].detach().numpy(), cc.grad[0].numpy()
            with torch.no_grad():                                         # nn.LSTM returns only the last c: step it for c_seq
                st = (hh.detach(), cc.detach())
                for t in range(n):
                    _, st = net(x[t:t + 1].detach(), st)
                    r["c_seq"][t, e] = st[1][0].numpy()
    g_w, g_b = net.weight_hh_l0.grad, net.bias_hh_l0.grad
    r["dW"] = np.zeros((HG, H)) if g_w is None else g_w.numpy()
    r["db"] = np.zeros(HG) if g_b is None else g_b.numpy()
    return r


@pytest.mark.parametrize("absent", list(R.ABSENT) + ["none"])
@pytest.mark.parametrize("H", [16, 32, 48, 64])
@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_loop_matches_float64_torch_nn(kind, H, absent):
    B, T = 6, 7
    c = R.case(kind, 100 + H, B, T, H, lens=[T, 0, 1, 4, T, 3])
    absent = R.ABSENT.get(absent, ())
    got = R.reference(kind, c, absent)
    want = _nn_ref(kind, c, absent)
    h0 = None if "h0" in absent else c["h0"]
    got["dW"], got["db"] = R.weight_grads(got["dgh" if kind == "gru" else "dgates"], got["h_seq"], h0)
    # nn.GRU exposes dgi (the gradient of its input) but not dgh: dgh enters through dW, db and dh0, and differs from
    # dgi only in the n block, by the factor r
    for name, w in want.items():
        assert got[name].shape == w.shape and got[name].dtype == np.float64, name
        assert rel_close(got[name], w) <= 1e-12, (name, rel_close(got[name], w))
    if kind == "gru":
        assert np.array_equal(got["dgh"][:, :, :2 * H], got["dgi"][:, :, :2 * H])


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_frozen_rows_and_absent_operands(kind):
    B, T, H = 5, 6, 16
    c = R.case(kind, 7, B, T, H, lens=[0, T, 2, 0, 1])
    r = R.reference(kind, c)
    for e, n in enumerate(c["lens"]):
        for name in R.NAMES[kind]:
            if r[name].ndim == 3:
                assert not r[name][n:, e].any() and (n == 0 or r[name][:n, e].any()), name
        if n == 0:
            assert np.array_equal(r["h_last"][e], c["h0"][e]) and np.array_equal(r["dh0"][e], c["d_hlast"][e])
            if kind == "lstm":
                assert np.array_equal(r["c_last"][e], c["c0"][e]) and np.array_equal(r["dc0"][e], c["d_clast"][e])
        else:
            assert np.array_equal(r["h_last"][e], r["h_seq"][n - 1, e])
    for absent in R.ABSENT.values():                                  # None means zeros, exactly
        zeros = dict(c, **{k: np.zeros_like(c[k]) for k in absent if k in c})
        a, z = R.reference(kind, c, absent), R.reference(kind, zeros)
        for name in R.NAMES[kind]:
            assert np.array_equal(a[name], z[name]), (absent, name)


def test_degenerate_shapes():
    for kind in ("gru", "lstm"):
        c = R.case(kind, 1, 5, 0, 16, lens=[0] * 5)
        r = R.reference(kind, c)
        assert r["h_seq"].shape == (0, 5, 16) and np.array_equal(r["h_last"], c["h0"]) and np.array_equal(r["dh0"], c["d_hlast"])
        r = R.reference(kind, R.case(kind, 1, 0, 4, 16, lens=[]))
        assert all(r[name].size == 0 for name in R.NAMES[kind])


@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_length_patterns_hold_what_they_state(B):
    T = 6
    p = {name: np.asarray(R.length_pattern(name, B, T, seed=B)) for name in R.PATTERNS}
    assert all(len(v) == B and v.min() >= 0 and v.max() <= T for v in p.values())
    assert not p["zeros"].any() and (p["full"] == T).all() and (p["ones"] == 1).all()
    tiles = lambda v: [v[k:k + R.TILE] for k in range(0, B, R.TILE)]  # noqa: E731
    assert not tiles(p["tile0_zero_tile1_full"])[0].any() and (tiles(p["tile0_full_tile1_zero"])[0] == T).all()
    if B > R.TILE:
        assert len(tiles(p["tile0_zero_tile1_full"])[0]) == R.TILE    # sixteen zero lengths next to a full tile
        assert (tiles(p["tile0_zero_tile1_full"])[1] == T).all() and not tiles(p["tile0_full_tile1_zero"])[1].any()
    if B == 33:
        assert len(tiles(p["tile0_zero_tile1_full"])[1]) == R.TILE and not tiles(p["tile0_zero_tile1_full"])[2].any()
    assert p["one_full_slot0"][0] == T and p["one_full_slot0"].sum() == T
    assert p["one_full_slot15"][min(15, B - 1)] == T and p["one_full_slot15"].sum() == T
    assert all(t.max() == 3 for t in tiles(p["tmax3"])) and 3 < T
    if B > 2:
        assert {0, 1, T} <= set(p["random"].tolist())


@pytest.mark.parametrize("H", [16, 64])
@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_saturated_case_is_saturated_and_finite(kind, H):
    B, T = 17, 8
    c = R.saturated_case(kind, 50 + H, B, T, H)
    G = R.GATES[kind]
    assert np.abs(c["W"]).max() < 0.3 * 6 and c["lens"][0] == c["lens"][1] == T
    for k in range(G):                                                # the four planted values of every gate, signs included
        col = c["gi"][:, :, k * H + 4 * k:k * H + 4 * k + 4]
        rows = slice(2, None)                                         # rows 0 and 1 are overridden in whole gates
        assert (col[:, rows, 0] == 100).all() and (col[:, rows, 1] == -100).all()
        assert (col[:, rows, 2] == 0).all() and not np.signbit(col[:, rows, 2]).any()
        assert (col[:, rows, 3] == 0).all() and np.signbit(col[:, rows, 3]).all()
    pre = {}
    r = R.reference(kind, c, pre=pre)
    m = R.planted_mask(kind, B, T, H)
    assert m.any() and (c["gi"][m] != 0).all() and (np.abs(c["gi"][m]) == 100).all()
    live = np.asarray(c["lens"]).reshape(1, B, 1) > np.arange(T).reshape(T, 1, 1)
    sat = m & live
    assert sat.sum() > T * G * 2 and (np.abs(pre["a"][sat]) > 50).all()
    assert (np.sign(pre["a"][sat]) == np.sign(c["gi"][sat])).all()
    for name, v in r.items():
        assert np.isfinite(v).all(), name
    if kind == "lstm":                                                # c integrates: +1 a step in row 0, -1 in row 1
        step = np.diff(np.concatenate([c["c0"][None, :2].astype(np.float64), r["c_seq"][:, :2]], 0), axis=0)
        assert np.allclose(step[:, 0], 1.0, atol=1e-12) and np.allclose(step[:, 1], -1.0, atol=1e-12)
        assert np.abs(r["c_last"][0] - c["c0"][0] - T).max() < 1e-12
    else:
        assert np.array_equal(r["h_last"][0], c["h0"][0].astype(np.float64))       # z = 1 exactly: h never moves
        assert np.abs(r["h_seq"][:, 1] - 1.0).max() < 1e-12
    grads = [r[n] for n in R.BWD[kind] if r[n].ndim == 3]
    assert any(((g == 0) & np.broadcast_to(live, g.shape)).any() for g in grads)   # exact-zero gradients at live steps exist


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_every_gpu_input_has_a_finite_reference(kind):
    cases = [R.case(kind, 11, B, 6, H, lens=R.length_pattern(p, B, 6, seed=B)) for H in (16, 48) for B in (1, 33) for p in R.PATTERNS]
    cases += [R.case(kind, 12, 19, 8, 32), R.case(kind, 13, 17, 24, 48), R.case(kind, 14, 1, 40, 64), R.placement_case(kind, 15, 32),
              R.case(kind, 16, 770, 3, 16)]
    for c in cases:
        for name, v in R.reference(kind, c).items():
            assert np.isfinite(v).all(), name


def test_placement_case_and_permutation():
    c = R.placement_case("lstm", 3, 32)
    T = 8
    assert [c["lens"][i] for i in R.SOLO] == [0, 1, 3, T, T] and len(c["lens"]) == R.PERM_B
    assert sorted(R.PERM) == list(range(R.PERM_B))
    moved_tile = sum(i // R.TILE != p // R.TILE for i, p in enumerate(R.PERM))
    moved_slot = sum(i % R.TILE != p % R.TILE for i, p in enumerate(R.PERM))
    assert moved_tile >= R.PERM_B // 2 and moved_slot >= R.PERM_B - 3
    p = R.take_rows("lstm", c, R.PERM)
    assert p["lens"] == [c["lens"][i] for i in R.PERM] and np.array_equal(p["gi"][:, 4], c["gi"][:, R.PERM[4]])
    assert np.array_equal(p["c0"][9], c["c0"][R.PERM[9]]) and p["gi"].flags.c_contiguous
    # the reference itself is placement-free: the permuted batch gives the permuted rows
    a, b = R.reference("lstm", c), R.reference("lstm", p)
    for name in R.NAMES["lstm"]:
        rows = a[name][:, list(R.PERM)] if a[name].ndim == 3 else a[name][list(R.PERM)]
        assert rel_close(b[name], rows) <= 1e-13, name
