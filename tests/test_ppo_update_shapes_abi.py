"""The shapes the fused PPO update (gymrl_amd/ppo_net.FusedActorCriticUpdate) covers, checked without a GPU: the library's
gate gymrl_ppo_update_shape_ok, ppo_net.supported against it, the one-pass heads kernel's grid at every hidden width, and
the refusals that stay.  Every call here fails validation or has no rows: none reaches a launch."""
import ctypes
import itertools
import os
import re

import pytest

from conftest import ROOT

WIDTHS, OBS, ACTIONS = (64, 128, 256), (2, 3, 4, 6, 8), (2, 3, 4)


def _lib():
    from gymrl_amd import _lib
    return _lib, _lib.lib()


def test_shape_gate_is_declared_and_answers_the_whole_product():
    _l, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "gymrl.h")).read()
    assert re.search(r"\bint\s+gymrl_ppo_update_shape_ok\s*\(\s*int\s+C\s*,\s*int\s+D\s*,\s*int\s+A\s*\)\s*;", hdr)
    restype, argtypes = _l.SIGNATURES["gymrl_ppo_update_shape_ok"]
    assert restype is ctypes.c_int and list(argtypes) == [ctypes.c_int] * 3
    for C, D, A in itertools.product(WIDTHS, OBS, ACTIONS):
        assert L.gymrl_ppo_update_shape_ok(C, D, A) == 1, (C, D, A)
    for C, D, A in ((32, 6, 3), (512, 6, 3), (64, 5, 3), (64, 7, 3), (64, 6, 1), (64, 6, 5), (0, 0, 0), (96, 4, 4), (256, 1, 2)):
        assert L.gymrl_ppo_update_shape_ok(C, D, A) == 0, (C, D, A)
    assert _l.ABI_VERSION == 4 and L.gymrl_abi_version() == 4


def test_supported_is_the_librarys_answer():
    torch = pytest.importorskip("torch")
    from gymrl_amd import ppo_net
    from gymrl_amd.ppo_lunarlander import ActorCritic
    _l, L = _lib()
    for H, D, A in itertools.product((32, 64, 128, 256, 512), (1, 2, 3, 4, 5, 6, 7, 8), (1, 2, 3, 4, 5)):
        with torch.no_grad():
            net = ActorCritic(D, A, H)
        assert ppo_net.supported(net) == bool(L.gymrl_ppo_update_shape_ok(H, D, A)), (H, D, A)
    assert ppo_net.supported(ActorCritic(6, 3, 64)) and ppo_net.supported(ActorCritic(2, 3, 256))     # Acrobot-v1, MountainCar-v0
    assert not ppo_net.supported(ActorCritic(5, 3, 64)) and not ppo_net.supported(ActorCritic(6, 5, 64))


@pytest.mark.parametrize("C", WIDTHS)
def test_heads_loss_blocks_at_every_width(C):
    _l, L = _lib()
    rpw = 64 // (C // 4)                      # rows per wave-load; a wave's batch is 8 wave-loads, a block has 4 waves
    for B in (1, 32, 33, 131073):
        want = min(1024, -(-(-(-B // (8 * rpw))) // 4))
        assert L.gymrl_heads_loss_blocks(ctypes.c_int64(B), C) == want > 0, (B, C)
    assert L.gymrl_heads_loss_blocks(ctypes.c_int64(0), C) == 0


def test_heads_loss_blocks_refuses_other_widths():
    _l, L = _lib()
    for C in (32, 16, 96, 512, 0):
        assert L.gymrl_heads_loss_blocks(ctypes.c_int64(64), C) == 0


def test_refusals_that_stay():
    _l, L = _lib()
    null, i64 = ctypes.c_void_p(None), ctypes.c_int64
    fake = ctypes.c_void_p(256)                       # never dereferenced: validation fails first
    # gymrl_heads_bwd takes no three-action head (tests/test_abi.py's own call): A = 3 goes through the one pass instead
    assert L.gymrl_heads_bwd(fake, fake, fake, i64(8), 64, 3, fake, fake, fake, fake, fake, fake, fake, fake, 0, null,
                             fake, null) == -22
    for D in (5, 7):
        assert L.gymrl_linear_tanh_smallk(fake, fake, null, i64(8), D, 64, fake, null) == -22
        assert L.gymrl_linear_smallk(fake, fake, null, i64(8), D, 64, fake, null) == -22
    assert L.gymrl_heads_fwd_tanh(fake, i64(8), 64, 5, null, fake, null, fake, null, fake, fake, 1, null) == -22
    cfg = _l.PPOCfg(0.2, 3.0, 0.5, 0.01)

    def heads_loss(C, A, B=8):
        return L.gymrl_heads_loss_fwd_bwd(fake, i64(B), C, A, null, fake, null, fake, null, fake, fake, fake, fake, null,
                                          ctypes.byref(cfg), null, null, null, null, null, fake, fake, null)
    assert heads_loss(32, 3) == -22 and heads_loss(512, 3) == -22 and heads_loss(64, 5) == -22 and heads_loss(64, 1) == -22
    assert heads_loss(64, 3, B=0) == -22              # (no rows: refused as before, not a no-op)

    def finalize(C, A, D):
        return L.gymrl_update_finalize(i64(8), C, A, D, *([fake] * 14), null)
    assert finalize(64, 3, 6) == -22 and finalize(128, 3, 6) == -22      # the one launch stays a hidden-256 affair
    assert finalize(256, 5, 6) == -22 and finalize(256, 3, 5) == -22 and finalize(256, 3, 7) == -22
    # the new first-layer width with no rows is the no-op it is at every width
    assert L.gymrl_linear_tanh_smallk(fake, fake, null, i64(0), 6, 64, fake, null) == 0
    assert L.gymrl_linear_smallk(fake, fake, null, i64(0), 6, 256, fake, null) == 0
    assert L.gymrl_heads_fwd_tanh(fake, i64(0), 64, 3, null, fake, null, fake, null, fake, fake, 1, null) == 0
