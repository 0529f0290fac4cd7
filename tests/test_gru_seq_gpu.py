"""GPU checks of the one-launch GRU sequence kernels (gymrl_gru_seq_fwd / _bwd) on ragged batches of episodes:
against a CPU float64 nn.GRU run one episode at a time, against the per-step composition (F.linear + gymrl_gru_cell_*),
bit for bit against the cell kernels when W_hh = 0, and run to run."""
import numpy as np
import pytest

from conftest import rel_close

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


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
    gi = (rng.normal(size=(T, G, 3 * H)) * 1.5).astype(np.float32)
    W = (rng.normal(size=(3 * H, H)) * scale).astype(np.float32)
    b = (rng.normal(size=3 * H) * 0.5).astype(np.float32)
    h0 = (rng.normal(size=(G, H)) * 0.5).astype(np.float32)
    return [int(x) for x in lens], gi, W, b, h0


def _ref64(lens, gi, W, b, h0, d_hseq, d_hlast):
    """float64 nn.GRU with W_ih = I, b_ih = 0 (so its input projection IS gi), one unbatched episode per call."""
    T, G, H3 = gi.shape
    H = H3 // 3
    gru = torch.nn.GRU(H3, H).double()
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.eye(H3, dtype=torch.float64))
        gru.bias_ih_l0.zero_()
        gru.weight_hh_l0.copy_(torch.from_numpy(W).double())
        gru.bias_hh_l0.copy_(torch.from_numpy(b).double())
    gru.bias_ih_l0.requires_grad_(False)
    gru.weight_ih_l0.requires_grad_(False)
    h_seq, h_last = np.zeros((T, G, H)), np.zeros((G, H))
    dgi, dh0 = np.zeros((T, G, H3)), np.zeros((G, H))
    for e in range(G):
        n = lens[e]
        x = torch.from_numpy(gi[:n, e].astype(np.float64)).requires_grad_(True)
        hh = torch.from_numpy(h0[e:e + 1].astype(np.float64)).requires_grad_(True)
        out, hl = gru(x, hh)
        loss = (out * torch.from_numpy(d_hseq[:n, e].astype(np.float64))).sum() + \
            (hl[0] * torch.from_numpy(d_hlast[e].astype(np.float64))).sum()
        loss.backward()
        h_seq[:n, e], h_last[e] = out.detach().numpy(), hl[0].detach().numpy()
        dgi[:n, e], dh0[e] = x.grad.numpy(), hh.grad[0].numpy()
    return h_seq, h_last, dgi, dh0, gru.weight_hh_l0.grad.numpy(), gru.bias_hh_l0.grad.numpy()


def _weight_grads(dgh, h_seq, h0, lens):
    """dW_hh = sum_t dgh_t^T h_{t-1}, db_hh = sum_t dgh_t — the caller's GEMMs over the flattened rows."""
    hprev = torch.cat([h0.unsqueeze(0), h_seq[:-1]], 0)
    T, G, H3 = dgh.shape
    dW = dgh.reshape(T * G, H3).double().t() @ hprev.reshape(T * G, -1).double()
    return dW.cpu().numpy(), dgh.double().sum((0, 1)).cpu().numpy()


@pytest.mark.parametrize("G,T,H", [(1, 1000, 64), (5, 300, 64), (16, 200, 64), (33, 120, 64), (5, 60, 16), (7, 50, 48)])
def test_fused_matches_float64_nn_gru(dev, G, T, H):
    from gymrl_amd import ops
    rng = np.random.default_rng(G * 1000 + T + H)
    lens, gi, W, b, h0 = _case(rng, G, T, H)
    d_hseq = rng.normal(size=(T, G, H)).astype(np.float32)
    d_hlast = rng.normal(size=(G, H)).astype(np.float32)
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    h_seq, h_last = ops.gru_seq_fwd(td(gi), td(W), td(b), lens, h0=td(h0))
    dgi, dgh, dh0 = ops.gru_seq_bwd(td(gi), td(W), td(b), h_seq, lens, d_hseq=td(d_hseq), d_hlast=td(d_hlast), h0=td(h0))
    r_hseq, r_hlast, r_dgi, r_dh0, r_dW, r_db = _ref64(lens, gi, W, b, h0, d_hseq, d_hlast)
    hs = h_seq.cpu().numpy()
    assert rel_close(hs, r_hseq) <= 1e-5 and rel_close(h_last.cpu().numpy(), r_hlast) <= 1e-5
    for e, n in enumerate(lens):                                       # past each length: exact zeros
        assert not hs[n:, e].any() and not dgi.cpu().numpy()[n:, e].any() and not dgh.cpu().numpy()[n:, e].any()
    assert rel_close(dgi.cpu().numpy(), r_dgi) <= 1e-4 and rel_close(dh0.cpu().numpy(), r_dh0) <= 1e-4
    dW, db = _weight_grads(dgh, h_seq, td(h0), lens)
    assert rel_close(dW, r_dW) <= 1e-4 and rel_close(db, r_db) <= 1e-4


def _per_step(ops, gi, W, b, h0, lens, d_hseq, d_hlast):
    """The per-step composition: one F.linear + one gymrl_gru_cell_* launch per step and direction."""
    T, G, H3 = gi.shape
    H = H3 // 3
    ln = torch.tensor(lens, device=gi.device)
    h, hs = h0.clone(), []
    for t in range(T):
        gh = torch.nn.functional.linear(h, W, b)
        hn = ops.gru_cell_fwd(gi[t].contiguous(), gh.contiguous(), h)
        act = (t < ln).unsqueeze(1)
        hs.append(torch.where(act, hn, torch.zeros_like(hn)))
        h = torch.where(act, hn, h)
    h_seq = torch.stack(hs)
    dgi, dgh = torch.zeros_like(gi), torch.zeros_like(gi)
    dh = d_hlast.clone()
    for t in range(T - 1, -1, -1):
        act = (t < ln).unsqueeze(1)
        hp = h0 if t == 0 else h_seq[t - 1]
        gh = torch.nn.functional.linear(hp, W, b)
        go = dh + d_hseq[t]
        a, c, ddir = ops.gru_cell_bwd(gi[t].contiguous(), gh.contiguous(), hp.contiguous(), go.contiguous())
        dgi[t] = torch.where(act, a, torch.zeros_like(a))
        dgh[t] = torch.where(act, c, torch.zeros_like(c))
        dh = torch.where(act, ddir + dgh[t] @ W, dh)
    return h_seq, h, dgi, dgh, dh


def test_fused_matches_per_step_composition(dev):
    from gymrl_amd import ops
    rng = np.random.default_rng(5)
    G, T, H = 5, 200, 64
    lens, gi, W, b, h0 = _case(rng, G, T, H)
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_hseq, d_hlast = td(rng.normal(size=(T, G, H)).astype(np.float32)), td(rng.normal(size=(G, H)).astype(np.float32))
    ref = _per_step(ops, td(gi), td(W), td(b), td(h0), lens, d_hseq, d_hlast)
    h_seq, h_last = ops.gru_seq_fwd(td(gi), td(W), td(b), lens, h0=td(h0))
    dgi, dgh, dh0 = ops.gru_seq_bwd(td(gi), td(W), td(b), h_seq, lens, d_hseq=d_hseq, d_hlast=d_hlast, h0=td(h0))
    for got, want, tol in ((h_seq, ref[0], 1e-5), (h_last, ref[1], 1e-5), (dgi, ref[2], 1e-4), (dgh, ref[3], 1e-4),
                           (dh0, ref[4], 1e-4)):
        assert rel_close(got.cpu().numpy(), want.cpu().numpy()) <= tol


def test_zero_recurrent_weight_is_bit_exact_to_the_cell_kernels(dev):
    """W_hh = 0 makes gh exactly b_hh: the fused kernels must then reproduce gymrl_gru_cell_fwd / _bwd bit for bit."""
    from gymrl_amd import ops
    rng = np.random.default_rng(9)
    G, T, H = 19, 80, 64
    lens, gi, _, b, h0 = _case(rng, G, T, H)
    W = np.zeros((3 * H, H), np.float32)
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_hseq, d_hlast = td(rng.normal(size=(T, G, H)).astype(np.float32)), td(rng.normal(size=(G, H)).astype(np.float32))
    h_seq, h_last = ops.gru_seq_fwd(td(gi), td(W), td(b), lens, h0=td(h0))
    dgi, dgh, dh0 = ops.gru_seq_bwd(td(gi), td(W), td(b), h_seq, lens, d_hseq=d_hseq, d_hlast=d_hlast, h0=td(h0))
    gh = td(b).expand(G, 3 * H).contiguous()
    ln = torch.tensor(lens, device=dev).unsqueeze(1)
    h, want = td(h0), []
    for t in range(T):
        hn = ops.gru_cell_fwd(td(gi[t]), gh, h)
        want.append(torch.where(t < ln, hn, torch.zeros_like(hn)))
        h = torch.where(t < ln, hn, h)
    assert np.array_equal(h_seq.cpu().numpy(), torch.stack(want).cpu().numpy())
    assert np.array_equal(h_last.cpu().numpy(), h.cpu().numpy())
    dh = d_hlast.clone()
    for t in range(T - 1, -1, -1):
        hp = td(h0) if t == 0 else h_seq[t - 1].contiguous()
        a, c, ddir = ops.gru_cell_bwd(td(gi[t]), gh, hp, (dh + d_hseq[t]).contiguous())
        act = t < ln
        assert np.array_equal(dgi[t].cpu().numpy(), torch.where(act, a, torch.zeros_like(a)).cpu().numpy()), t
        assert np.array_equal(dgh[t].cpu().numpy(), torch.where(act, c, torch.zeros_like(c)).cpu().numpy()), t
        dh = torch.where(act, ddir, dh)
    assert np.array_equal(dh0.cpu().numpy(), dh.cpu().numpy())


def test_run_to_run_bit_identical_and_many_tiles(dev):
    from gymrl_amd import ops
    rng = np.random.default_rng(3)
    G, T, H = 800, 40, 32                                             # two launches of 768 + 32 episodes
    lens, gi, W, b, _ = _case(rng, G, T, H, lens=rng.integers(0, 41, size=800))
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_hseq = td(rng.normal(size=(T, G, H)).astype(np.float32))
    outs = []
    for _ in range(2):
        h_seq, h_last = ops.gru_seq_fwd(td(gi), td(W), td(b), lens)
        outs.append([x.cpu().numpy() for x in (h_seq, h_last) + ops.gru_seq_bwd(td(gi), td(W), td(b), h_seq, lens,
                                                                                 d_hseq=d_hseq)])
    for a, c in zip(*outs):
        assert np.array_equal(a, c)
    h_seq, h_last, dgi, dgh, dh0 = outs[0]
    for e in (0, 767, 768, 799):                                      # either side of the launch split
        n = lens[e]
        assert not h_seq[n:, e].any() and not dgi[n:, e].any()
        if n == 0:
            assert not h_last[e].any() and np.array_equal(dh0[e], np.zeros(H, np.float32))
        else:
            assert np.array_equal(h_last[e], h_seq[n - 1, e])
