"""GPU checks of the one-launch LSTM sequence kernels (gymrl_lstm_seq_fwd / _bwd) on ragged batches (lengths 0, 1 and T
included): against a CPU float64 nn.LSTM run one episode at a time, against the per-step composition (F.linear +
gymrl_lstm_cell_*), bit for bit against the cell kernels when W_hh = 0, and run to run.  The bounds are gru_seq's:
rel_close <= 1e-5 forward, <= 1e-4 for the gradients."""
import numpy as np
import pytest

from conftest import rel_close

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL_FWD, TOL_BWD = 1e-5, 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _case(rng, G, T, H, lens=None, scale=0.3):
    if lens is None:
        lens = rng.integers(1, T + 1, size=G)
        lens[0] = T
        if G > 1:
            lens[-1] = 1
        if G > 2:
            lens[1] = 0
    gi = (rng.normal(size=(T, G, 4 * H)) * 1.5).astype(np.float32)
    W = (rng.normal(size=(4 * H, H)) * scale).astype(np.float32)
    b = (rng.normal(size=4 * H) * 0.5).astype(np.float32)
    h0, c0 = ((rng.normal(size=(G, H)) * 0.5).astype(np.float32) for _ in range(2))
    return [int(x) for x in lens], gi, W, b, h0, c0


def _grads(rng, G, T, H):
    return (rng.normal(size=(T, G, H)).astype(np.float32), rng.normal(size=(G, H)).astype(np.float32),
            rng.normal(size=(G, H)).astype(np.float32))


def _ref64(lens, gi, W, b, h0, c0, d_hseq, d_hlast, d_clast):
    """float64 nn.LSTM with W_ih = I, b_ih = 0 (so its input projection IS gi), one unbatched episode per call."""
    T, G, H4 = gi.shape
    H = H4 // 4
    lstm = torch.nn.LSTM(H4, H).double()
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(torch.eye(H4, dtype=torch.float64))
        lstm.bias_ih_l0.zero_()
        lstm.weight_hh_l0.copy_(torch.from_numpy(W).double())
        lstm.bias_hh_l0.copy_(torch.from_numpy(b).double())
    lstm.bias_ih_l0.requires_grad_(False)
    lstm.weight_ih_l0.requires_grad_(False)
    r = dict(h_seq=np.zeros((T, G, H)), c_last=c0.astype(np.float64), h_last=h0.astype(np.float64),
             dgates=np.zeros((T, G, H4)), dh0=d_hlast.astype(np.float64), dc0=d_clast.astype(np.float64))
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.float64))  # noqa: E731
    for e in range(G):
        n = lens[e]
        if n == 0:                                                        # nothing runs: the state and its gradient pass through
            continue
        x = f64(gi[:n, e]).requires_grad_(True)
        hh, cc = f64(h0[e:e + 1]).requires_grad_(True), f64(c0[e:e + 1]).requires_grad_(True)
        out, (hl, cl) = lstm(x, (hh, cc))
        ((out * f64(d_hseq[:n, e])).sum() + (hl[0] * f64(d_hlast[e])).sum() + (cl[0] * f64(d_clast[e])).sum()).backward()
        r["h_seq"][:n, e], r["h_last"][e], r["c_last"][e] = out.detach().numpy(), hl[0].detach().numpy(), cl[0].detach().numpy()
        r["dgates"][:n, e], r["dh0"][e], r["dc0"][e] = x.grad.numpy(), hh.grad[0].numpy(), cc.grad[0].numpy()
    g_w, g_b = lstm.weight_hh_l0.grad, lstm.bias_hh_l0.grad
    r["dW"] = np.zeros((H4, H)) if g_w is None else g_w.numpy()
    r["db"] = np.zeros(H4) if g_b is None else g_b.numpy()
    return r


def _weight_grads(dgates, h_seq, h0):
    """dW_hh = sum_t dgates_t^T h_{t-1}, db_hh = sum_t dgates_t — the caller's GEMMs over the flattened rows (frozen rows
    contribute nothing: their dgates are zero)."""
    hprev = torch.cat([h0.unsqueeze(0), h_seq[:-1]], 0)
    T, G, H4 = dgates.shape
    dW = dgates.reshape(T * G, H4).double().t() @ hprev.reshape(T * G, -1).double()
    return dW.cpu().numpy(), dgates.double().sum((0, 1)).cpu().numpy()


def _run(ops, td, lens, gi, W, b, h0, c0, d_hseq, d_hlast, d_clast):
    h_seq, c_seq, h_last, c_last = ops.lstm_seq_fwd(td(gi), td(W), td(b), lens, h0=td(h0), c0=td(c0))
    dgates, dh0, dc0 = ops.lstm_seq_bwd(td(gi), td(W), td(b), h_seq, c_seq, lens, d_hseq=td(d_hseq), d_hlast=td(d_hlast),
                                        d_clast=td(d_clast), h0=td(h0), c0=td(c0))
    return h_seq, c_seq, h_last, c_last, dgates, dh0, dc0


@pytest.mark.parametrize("G,T,H", [(1, 300, 64), (5, 60, 64), (16, 40, 64), (17, 40, 64), (33, 24, 48), (5, 8, 16)])
def test_fused_matches_float64_nn_lstm(dev, G, T, H):
    from gymrl_amd import ops
    rng = np.random.default_rng(G * 1000 + T + H)
    lens, gi, W, b, h0, c0 = _case(rng, G, T, H)
    d_hseq, d_hlast, d_clast = _grads(rng, G, T, H)
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    h_seq, c_seq, h_last, c_last, dgates, dh0, dc0 = _run(ops, td, lens, gi, W, b, h0, c0, d_hseq, d_hlast, d_clast)
    r = _ref64(lens, gi, W, b, h0, c0, d_hseq, d_hlast, d_clast)
    hs, cs, dg = h_seq.cpu().numpy(), c_seq.cpu().numpy(), dgates.cpu().numpy()
    dW, db = _weight_grads(dgates, h_seq, td(h0))
    errs = {"h_seq": rel_close(hs, r["h_seq"]), "h_last": rel_close(h_last.cpu().numpy(), r["h_last"]),
            "c_last": rel_close(c_last.cpu().numpy(), r["c_last"]), "dgates": rel_close(dg, r["dgates"]),
            "dh0": rel_close(dh0.cpu().numpy(), r["dh0"]), "dc0": rel_close(dc0.cpu().numpy(), r["dc0"]),
            "dW_hh": rel_close(dW, r["dW"]), "db_hh": rel_close(db, r["db"])}
    print(f"lstm_seq vs float64 nn.LSTM G={G} T={T} H={H}: " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    for k in ("h_seq", "h_last", "c_last"):
        assert errs[k] <= TOL_FWD, (k, errs[k])
    for k in ("dgates", "dh0", "dc0", "dW_hh", "db_hh"):
        assert errs[k] <= TOL_BWD, (k, errs[k])
    hl, cl = h_last.cpu().numpy(), c_last.cpu().numpy()
    for e, n in enumerate(lens):
        assert not hs[n:, e].any() and not cs[n:, e].any() and not dg[n:, e].any()      # past each length: exact zeros
        if n == 0:
            assert np.array_equal(hl[e], h0[e]) and np.array_equal(cl[e], c0[e])
            assert np.array_equal(dh0.cpu().numpy()[e], d_hlast[e]) and np.array_equal(dc0.cpu().numpy()[e], d_clast[e])
        else:
            assert np.array_equal(hl[e], hs[n - 1, e]) and np.array_equal(cl[e], cs[n - 1, e])


def _per_step(ops, gi, W, b, h0, c0, lens, d_hseq, d_hlast, d_clast, linear=True):
    """The per-step composition: one F.linear + one gymrl_lstm_cell_* launch per step and direction.  linear=False: gh is
    b_hh itself (the W_hh = 0 case, with no GEMM in the way of a bit-for-bit comparison)."""
    T, G, H4 = gi.shape
    ln = torch.tensor(lens, device=gi.device).unsqueeze(1)
    gh_of = (lambda h: torch.nn.functional.linear(h, W, b).contiguous()) if linear else (lambda h: b.expand(G, H4).contiguous())
    h, c, hs, cs = h0.clone(), c0.clone(), [], []
    zero = torch.zeros_like(h0)
    for t in range(T):
        hn, cn = ops.lstm_cell_fwd(gi[t].contiguous(), gh_of(h), c.contiguous())
        act = t < ln
        hs.append(torch.where(act, hn, zero))
        cs.append(torch.where(act, cn, zero))
        h, c = torch.where(act, hn, h), torch.where(act, cn, c)
    h_seq, c_seq = torch.stack(hs), torch.stack(cs)
    dgates = torch.zeros_like(gi)
    dh, dc = d_hlast.clone(), d_clast.clone()
    for t in range(T - 1, -1, -1):
        act = t < ln
        hp, cp = (h0, c0) if t == 0 else (h_seq[t - 1], c_seq[t - 1])
        dg, dcp = ops.lstm_cell_bwd(gi[t].contiguous(), gh_of(hp), cp.contiguous(), (dh + d_hseq[t]).contiguous(), dc.contiguous())
        dgates[t] = torch.where(act, dg, torch.zeros_like(dg))
        dh = torch.where(act, dgates[t] @ W, dh)
        dc = torch.where(act, dcp, dc)
    return h_seq, c_seq, h, c, dgates, dh, dc


def test_fused_matches_per_step_composition(dev):
    from gymrl_amd import ops
    rng = np.random.default_rng(5)
    G, T, H = 5, 60, 64
    lens, gi, W, b, h0, c0 = _case(rng, G, T, H)
    grads = _grads(rng, G, T, H)
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ref = _per_step(ops, td(gi), td(W), td(b), td(h0), td(c0), lens, *(td(a) for a in grads))
    got = _run(ops, td, lens, gi, W, b, h0, c0, *grads)
    names = ("h_seq", "c_seq", "h_last", "c_last", "dgates", "dh0", "dc0")
    for name, a, want in zip(names, got, ref):
        err = rel_close(a.cpu().numpy(), want.cpu().numpy())
        print(f"lstm_seq vs per-step {name}: {err:.3e}")
        assert err <= (TOL_BWD if name.startswith("d") else TOL_FWD), (name, err)


def test_zero_recurrent_weight_is_bit_exact_to_the_cell_kernels(dev):
    """W_hh = 0 makes gh exactly b_hh: the fused kernels must then reproduce gymrl_lstm_cell_fwd / _bwd bit for bit in
    every output, forward and backward."""
    from gymrl_amd import ops
    rng = np.random.default_rng(9)
    G, T, H = 19, 40, 64
    lens, gi, _, b, h0, c0 = _case(rng, G, T, H)
    W = np.zeros((4 * H, H), np.float32)
    grads = _grads(rng, G, T, H)
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ref = _per_step(ops, td(gi), td(W), td(b), td(h0), td(c0), lens, *(td(a) for a in grads), linear=False)
    got = _run(ops, td, lens, gi, W, b, h0, c0, *grads)
    for name, a, want in zip(("h_seq", "c_seq", "h_last", "c_last", "dgates", "dh0", "dc0"), got, ref):
        assert np.array_equal(a.cpu().numpy(), want.cpu().numpy()), name


def test_run_to_run_bit_identical_and_many_tiles(dev):
    from gymrl_amd import ops
    rng = np.random.default_rng(3)
    G, T, H = 800, 8, 32                                              # two launches of 768 + 32 rows
    lens, gi, W, b, h0, c0 = _case(rng, G, T, H, lens=rng.integers(0, T + 1, size=G))
    grads = _grads(rng, G, T, H)
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    outs = [[x.cpu().numpy() for x in _run(ops, td, lens, gi, W, b, h0, c0, *grads)] for _ in range(2)]
    for a, c in zip(*outs):
        assert np.array_equal(a, c)
    h_seq, c_seq, h_last, c_last, dgates, dh0, dc0 = outs[0]
    for e in (0, 767, 768, 799):                                      # either side of the launch split
        n = lens[e]
        assert not h_seq[n:, e].any() and not c_seq[n:, e].any() and not dgates[n:, e].any()
        if n == 0:
            assert np.array_equal(h_last[e], h0[e]) and np.array_equal(c_last[e], c0[e])
            assert np.array_equal(dh0[e], grads[1][e]) and np.array_equal(dc0[e], grads[2][e])
        else:
            assert np.array_equal(h_last[e], h_seq[n - 1, e]) and np.array_equal(c_last[e], c_seq[n - 1, e])
            assert dgates[:n, e].any()
    # rows 767 and 768 sit in different launches: each against the per-step composition of its own row
    sel = [0, 767, 768, 799]
    ref = _per_step(ops, td(gi[:, sel]), td(W), td(b), td(h0[sel]), td(c0[sel]), [lens[e] for e in sel],
                    td(grads[0][:, sel]), td(grads[1][sel]), td(grads[2][sel]))
    assert rel_close(h_seq[:, sel], ref[0].cpu().numpy()) <= TOL_FWD and rel_close(dgates[:, sel], ref[4].cpu().numpy()) <= TOL_BWD
    assert rel_close(dh0[sel], ref[5].cpu().numpy()) <= TOL_BWD and rel_close(dc0[sel], ref[6].cpu().numpy()) <= TOL_BWD
