"""GPU checks of the per-step LSTM cell kernels (gymrl_lstm_cell_fwd / _bwd): bit for bit against tests/lstm_ref.py, the
numpy restatement of lstm_cell_device.hpp, including saturated gates and both forms of dc_out."""
import numpy as np
import pytest

import lstm_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _case(B, H):
    rng = np.random.default_rng(100 * B + H)
    gi, gh = ((rng.normal(size=(B, 4 * H)) * 2).astype(np.float32) for _ in range(2))
    c, dh, dc = (rng.normal(size=(B, H)).astype(np.float32) for _ in range(3))
    # pre-activations beyond +-9 (tanh saturates) and +-88 (exp leaves float32's range), in every gate block
    sat = np.array([-100.0, 100.0, -12.0, 12.0], np.float32)
    for gt in range(4):
        gi[0, gt * H:gt * H + 4] = np.roll(sat, gt)
        gh[0, gt * H:gt * H + 4] = np.roll(sat, gt) * 0.5
    c[0, :4] = (30.0, -30.0, 0.0, -0.0)
    return gi, gh, c, dh, dc


@pytest.mark.parametrize("B,H", [(1, 4), (5, 16), (33, 64), (7, 512)])
def test_cell_kernels_are_the_restatement_bit_for_bit(dev, B, H):
    from gymrl_amd import ops
    gi, gh, c, dh, dc = _case(B, H)
    assert np.abs(gi + gh).max() > 88 and ((np.abs(gi + gh) > 9) & (np.abs(gi + gh) < 88)).any()
    td = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    h_new, c_new = ops.lstm_cell_fwd(td(gi), td(gh), td(c))
    r_h, r_c = lstm_ref.cell_fwd(gi, gh, c)
    assert np.array_equal(h_new.cpu().numpy(), r_h) and np.array_equal(c_new.cpu().numpy(), r_c)
    for dcn in (None, dc):
        dgates, dcp = ops.lstm_cell_bwd(td(gi), td(gh), td(c), td(dh), None if dcn is None else td(dcn))
        r_dg, r_dcp = lstm_ref.cell_bwd(gi, gh, c, dh, dcn)
        assert np.all(np.isfinite(r_dg))
        assert np.array_equal(dgates.cpu().numpy(), r_dg) and np.array_equal(dcp.cpu().numpy(), r_dcp), dcn is None
