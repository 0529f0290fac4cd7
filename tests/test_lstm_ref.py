"""tests/lstm_ref.py (the numpy restatement of lstm_cell_device.hpp that the GPU tests compare bits against) pinned to
torch.nn.LSTM: against a float64 nn.LSTM on CPU and against the reference's own URNN(layer=nn.LSTM) golden window.
Bounds: 2e-6 forward, 1e-5 gradients (the GRU golden test's)."""
import numpy as np
import pytest

import lstm_ref
from conftest import load_golden, rel_close

torch = pytest.importorskip("torch")

PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def _run_ref(x, h0c0, sd, w_out, w_h):
    H = h0c0.shape[1] // 2
    w = [sd[k] for k in PARAMS]
    out, hL, cL, steps = lstm_ref.lstm_forward(x, h0c0[:, :H], h0c0[:, H:], w[0], w[1], w[2], w[3])
    g = lstm_ref.lstm_backward(x, steps, w[0], w[1], w_out, w_h[:, :H], w_h[:, H:])
    return out, np.concatenate([hL, cL], 1), g


def test_restatement_matches_float64_nn_lstm():
    rng = np.random.default_rng(7)
    B, L, D, H = 4, 7, 5, 8
    lstm = torch.nn.LSTM(D, H, batch_first=True).double()
    with torch.no_grad():
        for p in lstm.parameters():
            p.copy_(torch.from_numpy(rng.normal(size=tuple(p.shape)) * 0.6))
    x = (rng.normal(size=(B, L, D)) * 1.5).astype(np.float32)
    x[0, 0] *= 30.0                                                       # saturated gates
    s0 = (rng.normal(size=(B, 2 * H)) * 0.5).astype(np.float32)
    w_out, w_h = rng.normal(size=(B, L, H)).astype(np.float32), rng.normal(size=(B, 2 * H)).astype(np.float32)
    sd = {k: getattr(lstm, k).detach().numpy().astype(np.float32) for k in PARAMS}
    with torch.no_grad():                                                 # the float64 net holds the float32 weights exactly
        for k in PARAMS:
            getattr(lstm, k).copy_(torch.from_numpy(sd[k]).double())
    xt = torch.from_numpy(x).double().requires_grad_(True)
    h0 = torch.from_numpy(s0[:, :H].copy()).double().requires_grad_(True)
    c0 = torch.from_numpy(s0[:, H:].copy()).double().requires_grad_(True)
    out, (hL, cL) = lstm(xt, (h0.unsqueeze(0), c0.unsqueeze(0)))
    ((out * torch.from_numpy(w_out)).sum() + (hL[0] * torch.from_numpy(w_h[:, :H])).sum()
     + (cL[0] * torch.from_numpy(w_h[:, H:])).sum()).backward()
    r_out, r_state, g = _run_ref(x, s0, sd, w_out, w_h)
    assert rel_close(r_out, out.detach().numpy()) <= 2e-6
    assert rel_close(r_state, torch.cat([hL[0], cL[0]], 1).detach().numpy()) <= 2e-6
    assert rel_close(g["dx"], xt.grad.numpy()) <= 1e-5
    assert rel_close(g["dh0"], h0.grad.numpy()) <= 1e-5 and rel_close(g["dc0"], c0.grad.numpy()) <= 1e-5
    for k in PARAMS:
        assert rel_close(g[k], getattr(lstm, k).grad.numpy()) <= 1e-5, k


def test_restatement_matches_reference_urnn_lstm_golden():
    g = load_golden("ppo_lstm_lstm_parts")
    sd = {k: g["lstm_sd_rnn." + k] for k in PARAMS}
    assert sd["weight_ih_l0"].shape == (64, 12) and g["lstm_h0"].shape == (5, 32) and g["lstm_x"].shape == (5, 6, 12)
    assert np.abs(g["lstm_h0"]).min() > 0
    out, state, grads = _run_ref(g["lstm_x"], g["lstm_h0"], sd, g["lstm_w_out"], g["lstm_w_h"])
    assert rel_close(out, g["lstm_out"]) <= 2e-6 and rel_close(state, g["lstm_hn"]) <= 2e-6
    assert rel_close(grads["dx"], g["lstm_dx"]) <= 1e-5
    assert rel_close(np.concatenate([grads["dh0"], grads["dc0"]], 1), g["lstm_dh0"]) <= 1e-5
    for k in PARAMS:
        assert rel_close(grads[k], g["lstm_grad_rnn." + k]) <= 1e-5, k


def test_cell_restatement_saturates_like_the_formulas():
    """Beyond +-9 tanh is exactly +-1 and beyond +-88 the sigmoid is exactly 0 or 1: the cell then copies or drops c."""
    gi = np.array([[100.0, 100.0, 0.5, 100.0], [-100.0, 100.0, 20.0, 100.0], [100.0, -100.0, -20.0, -100.0]], np.float32)
    gh = np.zeros_like(gi)
    c = np.array([[0.25], [0.25], [0.25]], np.float32)
    h, cn = lstm_ref.cell_fwd(gi, gh, c)
    t = lstm_ref.tanhf(np.float32(0.5))
    assert cn[0, 0] == np.float32(0.25) + t and cn[1, 0] == np.float32(0.25) and cn[2, 0] == np.float32(-1.0)
    assert h[2, 0] == 0.0 and h[1, 0] == lstm_ref.tanhf(np.float32(0.25))
    dgates, dcp = lstm_ref.cell_bwd(gi, gh, c, np.ones_like(c))
    assert np.all(np.isfinite(dgates)) and dcp[2, 0] == 0.0
