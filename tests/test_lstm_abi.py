"""CPU-side checks of the LSTM entry points (cell and one-launch sequence kernels): declared once in the header and in
the binding, and every argument check runs before any HIP call, so bad input is -EINVAL (-22) on a machine with no GPU."""
import ctypes
import os
import re

NAMES = ("gymrl_lstm_cell_fwd", "gymrl_lstm_cell_bwd", "gymrl_lstm_seq_fwd", "gymrl_lstm_seq_bwd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lens(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_symbols_are_declared_once_and_loaded_with_the_header_signature():
    from gymrl_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "gymrl.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        protos = re.findall(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert len(protos) == 1, name
        params = [p.strip() for p in protos[0].split(",")]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for ct, p in zip(argtypes, params):
            if p.startswith("const int32_t*"):
                assert ct is ctypes.POINTER(ctypes.c_int32), (name, p)
            elif "*" in p:
                assert ct is ctypes.c_void_p, (name, p)
            else:
                assert p.startswith("int ") and ct is ctypes.c_int, (name, p)
        assert getattr(L, name).argtypes == argtypes
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define\s+GYMRL_ABI_VERSION\s+4\b", header)


def test_lstm_cell_validates_arguments_without_gpu():
    from gymrl_amd import _lib
    L = _lib.lib()
    null, fake, odd = None, 256, 260          # `fake` is 16-byte aligned and never dereferenced: validation fails first
    assert L.gymrl_lstm_cell_fwd(fake, fake, fake, 0, 16, fake, fake, null) == 0          # no rows: nothing to launch
    for H in (0, -4, 3, 6, 18):
        assert L.gymrl_lstm_cell_fwd(fake, fake, fake, 2, H, fake, fake, null) == -22, H
    assert L.gymrl_lstm_cell_fwd(fake, fake, fake, -1, 16, fake, fake, null) == -22
    for k in range(5):                                                                   # each pointer NULL, then misaligned
        for bad in (null, odd):
            a = [fake] * 5
            a[k] = bad
            assert L.gymrl_lstm_cell_fwd(a[0], a[1], a[2], 2, 16, a[3], a[4], null) == -22, (k, bad)
    assert L.gymrl_lstm_cell_bwd(fake, fake, fake, fake, null, 0, 16, fake, fake, null) == 0
    for k in range(7):
        for bad in (null, odd):
            a = [fake] * 7
            a[k] = bad
            if k == 4 and bad is null:
                continue                                                                 # dc_out = NULL means zeros: legal
            assert L.gymrl_lstm_cell_bwd(a[0], a[1], a[2], a[3], a[4], 2, 16, a[5], a[6], null) == -22, (k, bad)
    for H in (0, 2, 30):
        assert L.gymrl_lstm_cell_bwd(fake, fake, fake, fake, null, 2, H, fake, fake, null) == -22, H


def test_lstm_seq_validates_arguments_without_gpu():
    from gymrl_amd import _lib
    L = _lib.lib()
    null, fake, odd = None, 256, 260
    ok = _lens(3, 1)

    def fwd(gi=fake, W=fake, b=fake, h0=null, c0=null, lens=ok, T=4, B=2, H=64, h_seq=fake, c_seq=fake):
        return L.gymrl_lstm_seq_fwd(gi, W, b, h0, c0, lens, T, B, H, h_seq, c_seq, null, null, null)

    def bwd(gi=fake, W=fake, b=fake, h0=null, h_seq=fake, c_seq=fake, lens=ok, T=4, B=2, H=64, dgates=fake):
        return L.gymrl_lstm_seq_bwd(gi, W, b, h0, null, h_seq, c_seq, null, null, null, lens, T, B, H, dgates, null, null, null)

    assert fwd(B=0) == 0 and bwd(B=0) == 0                                # no rows: nothing to launch
    for H in (0, 8, 20, 63, 80, 128, 512):
        assert fwd(H=H) == -22 and bwd(H=H) == -22, H                     # H not in {16, 32, 48, 64}
    for kw in ({"gi": null}, {"W": null}, {"b": null}, {"lens": None}, {"h_seq": null}, {"c_seq": null}):
        assert fwd(**kw) == -22 and bwd(**kw) == -22, kw                  # NULL required pointers
    assert bwd(dgates=null) == -22
    for kw in ({"W": odd}, {"h_seq": odd}, {"h0": odd}):
        assert fwd(**kw) == -22 and bwd(**kw) == -22, kw                  # misaligned vector-loaded pointers
    for lens in (_lens(3, 5), _lens(-1, 2)):
        assert fwd(lens=lens) == -22 and bwd(lens=lens) == -22            # len out of [0, T]
    assert fwd(T=-1) == -22 and fwd(B=-2) == -22 and bwd(T=-1) == -22 and bwd(B=-2) == -22
    # T = 0 or B = 0: the [T,B,*] arrays have no element, and NULL is what an allocator hands out for them
    assert fwd(gi=null, h_seq=null, c_seq=null, B=0) == 0 and bwd(gi=null, h_seq=null, c_seq=null, dgates=null, B=0) == 0
    assert fwd(W=null, B=0) == -22 and bwd(b=null, B=0) == -22


def test_ops_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    import pytest
    torch = pytest.importorskip("torch")
    from gymrl_amd import ops
    T, B, H = 3, 2, 16
    gi, W, b = torch.zeros(T, B, 4 * H), torch.zeros(4 * H, H), torch.zeros(4 * H)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.lstm_cell_fwd(gi[0], gi[0], torch.zeros(B, H))
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.lstm_seq_fwd(gi, W, b, [T] * B)
    with pytest.raises(ValueError, match="lengths"):
        ops.lstm_seq_fwd(gi, W, b, [T])
    with pytest.raises(ValueError, match="W_hh"):
        ops.lstm_seq_fwd(gi, torch.zeros(3 * H, H), b, [T] * B)
    with pytest.raises(ValueError, match="c0"):
        ops.lstm_seq_fwd(gi, W, b, [T] * B, c0=torch.zeros(B, H + 1))
    with pytest.raises(ValueError, match="c_seq"):
        ops.lstm_seq_bwd(gi, W, b, torch.zeros(T, B, H), torch.zeros(T, B, H + 4), [T] * B)
    with pytest.raises(ValueError, match="gh"):
        ops.lstm_cell_bwd(gi[0], torch.zeros(B, 3 * H), torch.zeros(B, H), torch.zeros(B, H))
    seq, row = torch.zeros(T, B, H), torch.zeros(B, H)                 # caller-owned outputs of the wrong shape
    for name, bad in (("h_seq", torch.zeros(T, B + 1, H)), ("c_seq", torch.zeros(T + 1, B, H)), ("h_last", torch.zeros(B, H + 1)),
                      ("c_last", torch.zeros(B + 1, H))):
        with pytest.raises(ValueError, match=name):
            ops.lstm_seq_fwd(gi, W, b, [T] * B, **{name: bad})
    for name, bad in (("dgates", torch.zeros(T, B, 3 * H)), ("dh0", torch.zeros(B, H + 1)), ("dc0", torch.zeros(H, B))):
        with pytest.raises(ValueError, match=name):
            ops.lstm_seq_bwd(gi, W, b, seq, seq, [T] * B, **{name: bad})
    for kw in ({"dh0": row}, {"dc0": row}, {"dh0": row, "dc0": row}):
        with pytest.raises(ValueError, match="need_d0"):
            ops.lstm_seq_bwd(gi, W, b, seq, seq, [T] * B, need_d0=False, **kw)
    with pytest.raises(RuntimeError, match="MI355X"):                  # well-shaped outputs pass the shape checks
        ops.lstm_seq_bwd(gi, W, b, seq, seq, [T] * B, dgates=torch.zeros_like(gi), dh0=row, dc0=row.clone())


def test_urnn_accepts_gru_and_lstm_only():
    import pytest
    torch = pytest.importorskip("torch")
    from gymrl_amd.ppo_lstm_lunarlander import URNN, Config
    with pytest.raises(NotImplementedError):
        URNN(12, 16, layer=torch.nn.RNN)
    rnn = URNN(12, 16, layer=torch.nn.LSTM)
    assert rnn.chunk_size == 2 and tuple(rnn.rnn.weight_ih_l0.shape) == (64, 12)
    assert set(rnn.state_dict()) == {"rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0"}
    assert URNN(12, 16).chunk_size == 1
    cfg = Config()
    assert cfg.rnn_layer == "gru" and isinstance(cfg.rnn_fused, bool)
