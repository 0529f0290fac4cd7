"""Plain numpy float32 restatement of gymrl_amd/csrc/lstm_cell_device.hpp, operation by operation (TEST INFRASTRUCTURE).

exp and tanh are the built oracle library's orc_expf / orc_tanhf_sel (the bits of det_expf and det_tanhf_sel), taken through
tests/det_math_ref.py; everything else is IEEE float32 arithmetic, which numpy evaluates exactly as the header writes it (the kernels
are built with -ffp-contract=off and correctly rounded division).  Also a window / episode recurrence with float64 gate
products, like oracle.gru_forward, and its reverse.
"""
import numpy as np

import det_math_ref

_F = np.float32
_ONE = _F(1.0)


def expf(x):
    return det_math_ref.expf(x)


def tanhf(x):
    """det_tanhf_sel"""
    return det_math_ref.tanhf_sel(x)


def sigmoidf(x):
    """det_sigmoidf: 1.0f / (1.0f + det_expf(-x))"""
    return _ONE / (_ONE + expf(-np.asarray(x, _F)))


def _split(g):
    g = np.asarray(g, _F)
    H = g.shape[-1] // 4
    return g[..., :H], g[..., H:2 * H], g[..., 2 * H:3 * H], g[..., 3 * H:]


def gates(gi, gh):
    """lstm_gates: PyTorch's order i, f, g, o on a = gi + gh."""
    (ii, fi, gg, oi), (ih, fh, hg, oh) = _split(gi), _split(gh)
    return sigmoidf(ii + ih), sigmoidf(fi + fh), tanhf(gg + hg), sigmoidf(oi + oh)


def cell_fwd(gi, gh, c):
    """lstm_point_fwd -> (h', c')"""
    c = np.asarray(c, _F)
    i, f, g, o = gates(gi, gh)
    c_new = (f * c) + (i * g)
    h_new = o * tanhf(c_new)
    return h_new, c_new


def cell_bwd(gi, gh, c, dh, dcn=None):
    """lstm_point_bwd -> (dgates [.., 4H] = dgi = dgh, dc_prev)"""
    c, dh = np.asarray(c, _F), np.asarray(dh, _F)
    dcn = np.zeros_like(c) if dcn is None else np.asarray(dcn, _F)
    i, f, g, o = gates(gi, gh)
    cn = (f * c) + (i * g)
    tc = tanhf(cn)
    do = (dh * tc) * (o * (_ONE - o))
    dc = dcn + ((dh * o) * (_ONE - (tc * tc)))
    di = (dc * g) * (i * (_ONE - i))
    df = (dc * c) * (f * (_ONE - f))
    dg = (dc * i) * (_ONE - (g * g))
    dcp = dc * f
    return np.concatenate([di, df, dg, do], -1), dcp


def _mm(a, b):
    return (np.asarray(a, np.float64) @ np.asarray(b, np.float64))


def lstm_forward(x, h0, c0, w_ih, w_hh, b_ih, b_hh):
    """torch.nn.LSTM(batch_first=True, one layer) over x [B, L, D] from (h0, c0) [B, H] -> (out [B, L, H], h_L, c_L,
    and the per-step (gi, gh, c_prev, h_prev) the reverse pass needs)."""
    x, h, c = np.asarray(x, _F), np.asarray(h0, _F), np.asarray(c0, _F)
    outs, steps = [], []
    for l in range(x.shape[1]):
        gi = (_mm(x[:, l], np.asarray(w_ih).T) + b_ih).astype(_F)
        gh = (_mm(h, np.asarray(w_hh).T) + b_hh).astype(_F)
        steps.append((gi, gh, c, h))
        h, c = cell_fwd(gi, gh, c)
        outs.append(h)
    return np.stack(outs, 1), h, c, steps


def lstm_backward(x, steps, w_ih, w_hh, d_out, d_hL, d_cL):
    """Reverse of lstm_forward for loss = sum(out * d_out) + sum(h_L * d_hL) + sum(c_L * d_cL).
    Returns dict(dx, dh0, dc0, weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0); the products are float64."""
    x = np.asarray(x, _F)
    B, L, D = x.shape
    dh, dc = np.asarray(d_hL, _F), np.asarray(d_cL, _F)
    dx = np.zeros((B, L, D), _F)
    dW_ih, dW_hh = np.zeros(np.shape(w_ih), np.float64), np.zeros(np.shape(w_hh), np.float64)
    db = np.zeros(np.shape(w_hh)[0], np.float64)
    for l in range(L - 1, -1, -1):
        gi, gh, c_prev, h_prev = steps[l]
        dgates, dc = cell_bwd(gi, gh, c_prev, dh + np.asarray(d_out, _F)[:, l], dc)
        dW_ih += _mm(dgates.T, x[:, l])
        dW_hh += _mm(dgates.T, h_prev)
        db += dgates.astype(np.float64).sum(0)
        dx[:, l] = _mm(dgates, w_ih).astype(_F)
        dh = _mm(dgates, w_hh).astype(_F)
    return {"dx": dx, "dh0": dh, "dc0": dc, "weight_ih_l0": dW_ih, "weight_hh_l0": dW_hh, "bias_ih_l0": db, "bias_hh_l0": db}
