"""CPU-side checks of the whole-episode recurrent entry points (GRU sequence, per-episode GAE, L5 / L6): every argument
check runs before any HIP call, so bad input is -EINVAL (-22) on a machine with no GPU at all."""
import ctypes

import numpy as np


def _lens(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _offs(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_symbols_are_declared_and_loaded():
    from gymrl_amd import _lib
    L = _lib.lib()
    for name in ("gymrl_gru_seq_fwd", "gymrl_gru_seq_bwd", "gymrl_episode_gae", "gymrl_ppg_policy_loss_fwd_bwd",
                 "gymrl_ppg_aux_loss_fwd_bwd"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.gymrl_abi_version() == 4


def test_gru_seq_validates_arguments_without_gpu():
    from gymrl_amd import _lib
    L = _lib.lib()
    null, fake = None, 256                    # `fake` is 16-byte aligned and never dereferenced: validation fails first
    fwd = lambda gi, h0, lens, T, B, H: L.gymrl_gru_seq_fwd(gi, fake, fake, h0, lens, T, B, H, fake, fake, null)  # noqa: E731
    ok = _lens(3, 1)
    for H in (0, 8, 20, 63, 80, 128):
        assert fwd(fake, null, ok, 4, 2, H) == -22, H                    # H not in {16, 32, 48, 64}
    assert fwd(null, null, ok, 4, 2, 64) == -22                          # NULL gi
    assert fwd(fake, null, None, 4, 2, 64) == -22                        # NULL lengths
    assert fwd(fake, null, _lens(3, 5), 4, 2, 64) == -22                 # len[b] > T
    assert fwd(fake, null, _lens(-1, 2), 4, 2, 64) == -22                # len[b] < 0
    assert fwd(fake, 260, ok, 4, 2, 64) == -22                           # h0 not 16-byte aligned
    assert fwd(fake, null, ok, -1, 2, 64) == -22 and fwd(fake, null, ok, 4, -2, 64) == -22
    assert L.gymrl_gru_seq_fwd(fake, 260, fake, null, ok, 4, 2, 64, fake, fake, null) == -22   # W_hh misaligned
    assert L.gymrl_gru_seq_fwd(fake, fake, fake, null, ok, 4, 2, 64, fake, null, null) == -22  # NULL h_last
    assert fwd(fake, null, ok, 4, 0, 64) == 0                            # no episodes: nothing to launch
    bwd = lambda lens, T, H, dgi=fake: L.gymrl_gru_seq_bwd(fake, fake, fake, null, fake, null, null, lens, T, 2, H,  # noqa: E731
                                                           dgi, fake, null, null)
    assert bwd(ok, 4, 40) == -22 and bwd(_lens(3, 9), 4, 64) == -22 and bwd(ok, 4, 64, dgi=null) == -22
    assert L.gymrl_gru_seq_bwd(fake, fake, fake, null, null, null, null, ok, 4, 2, 64, fake, fake, null, null) == -22  # NULL h_seq
    assert L.gymrl_gru_seq_bwd(fake, fake, fake, null, fake, null, null, ok, 4, 0, 64, fake, fake, null, null) == 0
    # B = 0: the [T,B,*] arrays and h_last have no element, and NULL is what an allocator hands out for them
    assert L.gymrl_gru_seq_fwd(null, fake, fake, null, ok, 4, 0, 64, null, null, null) == 0
    assert L.gymrl_gru_seq_bwd(null, fake, fake, null, null, null, null, ok, 4, 0, 64, null, null, null, null) == 0
    assert L.gymrl_gru_seq_fwd(null, null, fake, null, ok, 4, 0, 64, null, null, null) == -22      # W_hh is never empty
    assert L.gymrl_gru_seq_fwd(fake, fake, fake, null, _lens(0, 0), 0, 2, 64, null, null, null) == -22   # T = 0, B > 0: h_last


def test_episode_gae_validates_offsets_without_gpu():
    from gymrl_amd import _lib
    L = _lib.lib()
    null, fake = None, 256
    gae = lambda offs, E, out=fake: L.gymrl_episode_gae(fake, fake, fake, fake, fake, offs, E, 0.995, 0.95, null,  # noqa: E731
                                                         out, fake, null, null)
    assert gae(None, 2) == -22                                           # NULL offsets
    assert gae(_offs(1, 4, 9), 2) == -22                                 # offsets[0] != 0
    assert gae(_offs(0, 4, 3), 2) == -22                                 # decreasing
    assert gae(_offs(0, 4, 4), 2) == -22                                 # empty episode
    assert gae(_offs(0, 4, 9), -1) == -22
    assert gae(_offs(0, 4, 9), 2, out=null) == -22                       # NULL adv_norm
    assert gae(_offs(0), 0) == 0                                         # no episodes


def test_ppg_losses_validate_arguments_without_gpu():
    from gymrl_amd import _lib
    L = _lib.lib()
    null, fake = None, 256
    pol = lambda offs, G, A, adv=fake: L.gymrl_ppg_policy_loss_fwd_bwd(fake, fake, fake, fake, adv, fake, offs, G, A,  # noqa: E731
                                                                       0.2, 3.0, 0.5, 0.01, fake, fake, fake, null, null)
    aux = lambda offs, G, A, ep=fake: L.gymrl_ppg_aux_loss_fwd_bwd(fake, fake, fake, fake, fake, offs, G, A, 1.0,  # noqa: E731
                                                                   fake, fake, ep, null, null)
    good = _offs(0, 3, 10)
    for f in (pol, aux):
        assert f(good, 2, 1) == -22 and f(good, 2, 9) == -22             # 2 <= A <= 8
        assert f(good, 0, 4) == -22                                      # no episode
        assert f(None, 2, 4) == -22                                      # NULL offsets
        assert f(_offs(0, 3, 3), 2, 4) == -22                            # empty episode
        assert f(_offs(2, 3, 10), 2, 4) == -22                           # offsets[0] != 0
        assert f(_offs(0, 5, 4), 2, 4) == -22                            # decreasing
    assert pol(good, 2, 4, adv=null) == -22 and aux(good, 2, 4, ep=null) == -22


def test_ops_wrappers_refuse_cpu_tensors():
    import pytest
    import torch
    from gymrl_amd import ops
    gi = torch.zeros(4, 2, 192)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gru_seq_fwd(gi, torch.zeros(192, 64), torch.zeros(192), [4, 2])
    x = torch.zeros(6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.episode_gae(x, x, x, x.to(torch.uint8), x.to(torch.uint8), np.array([0, 2, 6]), 0.99, 0.95)


def test_reference_fixture_is_self_consistent():
    """ppg_rnn_parts.npz (tests/golden/make_golden_ppg.py, the reference's own compute_advantage and update()):
    v_target = adv + values exactly, each episode's normalised adv has mean ~0 (NaN for a length-1 episode, as torch's
    unbiased std makes it), and the recorded losses restate from the recorded inputs."""
    import torch
    from conftest import load_golden
    g = load_golden("ppg_rnn_parts")
    offs = g["gae_offsets"]
    assert offs[0] == 0 and offs[-1] == g["gae_rew"].size and np.all(np.diff(offs) > 0)
    assert np.array_equal(g["gae_v_target"], g["gae_adv_raw"] + g["gae_val"])
    for e in range(offs.size - 1):
        a = g["gae_adv_norm"][offs[e]:offs[e + 1]]
        if a.size == 1:
            assert np.isnan(a).all()
        else:
            assert abs(float(a.astype(np.float64).mean())) <= 1e-6
            assert abs(float(a.astype(np.float64).std(ddof=1)) - 1.0) <= 1e-5
    for k in range(int(g["loss_cases"][0])):
        vt, v, aux = (torch.from_numpy(g[f"l{k}_{n}"]).double() for n in ("v_target", "value", "aux"))
        m = g[f"l{k}_metrics"]
        assert abs(float(((vt - v) ** 2).mean()) - m[2]) <= 1e-5 * max(1.0, abs(m[2]))
        assert abs(float(((vt - aux) ** 2).mean()) - m[5]) <= 1e-5 * max(1.0, abs(m[5]))
        assert abs(float(g[f"l{k}_adv"].astype(np.float64).mean()) - m[4]) <= 1e-6
    # the tie rows of case 0: ratio exp(lp - old) is exactly dual_clip in f32 (torch.max(min_surr, dual_clip * adv) ties)
    lp = torch.distributions.Categorical(torch.softmax(torch.from_numpy(g["l0_logits"][12:16]), -1)).log_prob(
        torch.from_numpy(g["l0_act"][12:16]).long())
    assert (torch.exp(lp - torch.from_numpy(g["l0_old_logp"][12:16])) == 3.0).all()
    assert (g["l0_adv"][12:16] < 0).all()


def test_ops_wrappers_check_offsets_and_shapes_before_launch():
    """The host lengths / offsets steer the kernels' addressing, so the wrappers refuse tensors that disagree with them."""
    import pytest
    import torch
    from gymrl_amd import ops
    x, u8 = torch.zeros(6), torch.zeros(6, dtype=torch.uint8)
    with pytest.raises(ValueError, match="offsets"):
        ops.episode_gae(x, x, x, u8, u8, [0, 2, 7], 0.99, 0.95)           # ends past the 6 stored rows
    with pytest.raises(ValueError, match="val"):
        ops.episode_gae(x, torch.zeros(5), x, u8, u8, [0, 2, 6], 0.99, 0.95)
    z, a = torch.zeros(6, 4), torch.zeros(6, dtype=torch.int32)
    with pytest.raises(ValueError, match="offsets"):
        ops.ppg_policy_loss_fwd_bwd(z, x, a, x, x, x, [0, 5], 0.2, 3.0, 0.5, 0.01)
    with pytest.raises(ValueError, match="v_target"):
        ops.ppg_aux_loss_fwd_bwd(z, x, a, x, torch.zeros(7), [0, 6], 1.0)
    gi = torch.zeros(4, 2, 192)
    with pytest.raises(ValueError, match="W_hh"):
        ops.gru_seq_fwd(gi, torch.zeros(64, 192), torch.zeros(192), [4, 2])
    with pytest.raises(ValueError, match="h0"):
        ops.gru_seq_fwd(gi, torch.zeros(192, 64), torch.zeros(192), [4, 2], h0=torch.zeros(3, 64))
    with pytest.raises(ValueError, match="lengths"):
        ops.gru_seq_fwd(gi, torch.zeros(192, 64), torch.zeros(192), [4])
    with pytest.raises(ValueError, match="d_hseq"):
        ops.gru_seq_bwd(gi, torch.zeros(192, 64), torch.zeros(192), torch.zeros(4, 2, 64), [4, 2],
                        d_hseq=torch.zeros(4, 3, 64))
    W, b, seq = torch.zeros(192, 64), torch.zeros(192), torch.zeros(4, 2, 64)      # caller-owned outputs of the wrong shape
    for name, bad in (("dgi", torch.zeros(4, 2, 128)), ("dgh", torch.zeros(3, 2, 192)), ("dh0", torch.zeros(2, 63))):
        with pytest.raises(ValueError, match=name):
            ops.gru_seq_bwd(gi, W, b, seq, [4, 2], **{name: bad})
    with pytest.raises(ValueError, match="need_dh0"):
        ops.gru_seq_bwd(gi, W, b, seq, [4, 2], need_dh0=False, dh0=torch.zeros(2, 64))
    with pytest.raises(ValueError, match="h_last"):
        ops.gru_seq_fwd(gi, W, b, [4, 2], h_last=torch.zeros(2, 65))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                     # well-shaped outputs pass the shape checks
        ops.gru_seq_bwd(gi, W, b, seq, [4, 2], dgi=torch.zeros_like(gi), dgh=torch.zeros_like(gi), dh0=torch.zeros(2, 64))
