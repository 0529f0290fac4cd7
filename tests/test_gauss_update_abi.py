"""The Gaussian head's fused PPO update (gymrl_amd/ppo_net.FusedGaussianUpdate) without a GPU: the new gate over its whole
product, ppo_net.gauss_supported against it, the workspace size, every refusal of gymrl_gauss_heads_loss_fwd_bwd on fake pointers
(-22 before any launch), the ops wrappers' ValueError, header / exports / SIGNATURES, and the categorical gate and entry points
answering A = 1 as they did."""
import ctypes
import itertools
import os
import re

import pytest

torch = pytest.importorskip("torch")

from gymrl_amd import _lib, ops, ppo_net  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gymrl.h")
FAKE = 0x10000                   # aligned to everything asked for, never dereferenced on the host
WIDTHS, OBS = (64, 128, 256), (2, 3, 4, 6, 8)
NEW = ["gymrl_ppo_gauss_update_shape_ok", "gymrl_gauss_heads_loss_workspace_bytes", "gymrl_gauss_heads_loss_fwd_bwd"]
i64 = ctypes.c_int64


def test_gate_answers_the_whole_product():
    L = _lib.lib()
    for C, D in itertools.product(WIDTHS, OBS):
        assert L.gymrl_ppo_gauss_update_shape_ok(C, D, 1) == 1, (C, D)
        assert ops.ppo_gauss_update_shape_ok(C, D, 1) is True
        for A in (0, 2, 3):
            assert L.gymrl_ppo_gauss_update_shape_ok(C, D, A) == 0, (C, D, A)
    for C, D in itertools.product((32, 96, 512), OBS):
        assert L.gymrl_ppo_gauss_update_shape_ok(C, D, 1) == 0, (C, D)
    for C, D in itertools.product(WIDTHS, (1, 5, 7)):
        assert L.gymrl_ppo_gauss_update_shape_ok(C, D, 1) == 0, (C, D)
    assert L.gymrl_ppo_gauss_update_shape_ok(0, 0, 0) == 0 and L.gymrl_ppo_gauss_update_shape_ok(-64, 3, 1) == 0
    for bad in ((64.0, 3, 1), (64, "3", 1), (64, 3, True)):
        with pytest.raises(ValueError):
            ops.ppo_gauss_update_shape_ok(*bad)


def test_the_categorical_gate_and_entry_points_still_refuse_one_action():
    L = _lib.lib()
    null, fake = ctypes.c_void_p(None), ctypes.c_void_p(FAKE)
    for C, D in itertools.product(WIDTHS, OBS):
        assert L.gymrl_ppo_update_shape_ok(C, D, 1) == 0, (C, D)
    from gymrl_amd.ppo_lunarlander import ActorCritic
    from gymrl_amd.ppo_pendulum import GaussianActorCritic
    for H, D in itertools.product((32, 64, 128, 256), (1, 2, 3, 4, 6, 8)):
        with torch.no_grad():
            assert not ppo_net.supported(ActorCritic(D, 1, H)) and not ppo_net.supported(GaussianActorCritic(D, 1, H)), (H, D)
    cfg = _lib.PPOCfg(0.2, 3.0, 0.5, 0.01)
    assert L.gymrl_heads_loss_fwd_bwd(fake, i64(8), 64, 1, null, fake, null, fake, null, fake, fake, fake, fake, null,
                                      ctypes.byref(cfg), null, null, null, null, null, fake, fake, null) == -22
    assert L.gymrl_heads_bwd(fake, fake, fake, i64(8), 64, 1, fake, fake, fake, fake, fake, fake, fake, fake, 0, null, fake, null) == -22
    assert L.gymrl_heads_fwd_tanh(fake, i64(8), 64, 1, null, fake, null, fake, null, fake, fake, 1, null) == -22
    assert L.gymrl_update_finalize(i64(8), 256, 1, 3, *([fake] * 14), null) == -22
    assert L.gymrl_heads_loss_blocks(i64(1000), 64) == 8           # the metric rows, unchanged: ceil(ceil(1000 / 32) / 4)


def test_gauss_supported_is_the_gates_answer():
    from gymrl_amd.ppo_lunarlander import ActorCritic
    from gymrl_amd.ppo_pendulum import GaussianActorCritic
    L = _lib.lib()
    for H, D, A in itertools.product((32, 64, 128, 256, 512), (1, 2, 3, 4, 5, 6, 7, 8), (1, 2, 3)):
        with torch.no_grad():
            net = GaussianActorCritic(D, A, H)
        assert ppo_net.gauss_supported(net) == bool(L.gymrl_ppo_gauss_update_shape_ok(H, D, A)), (H, D, A)
    assert ppo_net.gauss_supported(GaussianActorCritic(3, 1, 64)) and ppo_net.gauss_supported(GaussianActorCritic(3, 1, 256))   # Pendulum-v1
    assert not ppo_net.gauss_supported(ActorCritic(3, 1, 64))      # no log_std: not a Gaussian head
    net = GaussianActorCritic(3, 1, 64)
    net.actor[0] = torch.nn.Linear(64, 128)                        # the same width checks as supported()
    assert not ppo_net.gauss_supported(net)
    with pytest.raises(ValueError):
        ppo_net.FusedGaussianUpdate(ActorCritic(3, 1, 64), 8)
    with pytest.raises(ValueError):
        ppo_net.FusedActorCriticUpdate(GaussianActorCritic(3, 1, 64), 8)
    assert issubclass(ppo_net.FusedGaussianUpdate, ppo_net.FusedActorCriticUpdate)
    assert ppo_net.FusedGaussianUpdate.step is ppo_net.FusedActorCriticUpdate.step                # one launch sequence
    assert ppo_net.FusedGaussianUpdate.metric_blocks is ppo_net.FusedActorCriticUpdate.metric_blocks


def test_workspace_bytes():
    L = _lib.lib()
    q = lambda B, C, A=1: L.gymrl_gauss_heads_loss_workspace_bytes(i64(B), C, A)   # noqa: E731
    for C in WIDTHS:
        batch = 8 * (256 // C)                                     # a wave's batch: 32 / 16 / 8 rows
        for B in (1, batch - 1, batch, batch + 1, 9 * batch + 3, 131073):
            assert q(B, C) == -(-B // batch) * 8, (B, C)
    assert q(0, 64) == q(-1, 64) == q(64, 32) == q(64, 96) == q(64, 512) == q(64, 64, 0) == q(64, 64, 2) == 0


def test_heads_loss_refuses_bad_arguments():
    L, f, n = _lib.lib(), FAKE, None
    cfg = _lib.PPOCfg(0.2, 3.0, 0.5, 0.01)
    names = ("Zac", "bac", "Wa2", "ba2", "Wc2", "bc2", "log_std", "act", "logp_old", "adv", "ret", "mom")
    outs = ("dbac", "dWa2", "dba2", "dWc2", "dbc2", "dls", "met", "ws", "dws")

    def call(B=8, C=64, A=1, grid=0, cfgp=ctypes.byref(cfg), **ptr):
        p = {k: f for k in names + outs}
        p.update(bac=n, ba2=n, bc2=n, mom=n)
        p.update(ptr)
        return L.gymrl_gauss_heads_loss_fwd_bwd(p["Zac"], i64(B), C, A, *[p[k] for k in names[1:]], cfgp, *[p[k] for k in outs], grid, n)
    for name in ("Zac", "Wa2", "Wc2", "log_std", "act", "logp_old", "adv", "ret") + outs:
        assert call(**{name: n}) == -22, name
    assert call(cfgp=None) == -22
    for C in (32, 96, 512, 0):
        assert call(C=C) == -22, C
    for A in (0, 2, 3, 4):
        assert call(A=A) == -22, A
    assert call(B=0) == call(B=-5) == -22                           # (no rows: refused, as gymrl_heads_loss_fwd_bwd refuses them)
    assert call(grid=-1) == -22
    assert call(Zac=f + 4) == call(Zac=f + 8) == call(bac=f + 4) == -22        # 16-byte rows
    assert call(met=f + 4) == call(dws=f + 4) == -22               # float64 tables


def test_header_exports_and_signatures_agree():
    with open(HEADER) as fh:
        text = fh.read()
    L = _lib.lib()
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION and "#define GYMRL_ABI_VERSION 4" in text
    order = [m.group(1) for m in re.finditer(r"^(?:int|size_t)\s+(gymrl_\w+)\(", text, flags=re.M)]
    sig = list(_lib.SIGNATURES)
    for name in NEW:
        assert order.count(name) == 1 and name in _lib.SIGNATURES and name in _lib.SYMBOLS and hasattr(L, name), name
        assert sig[sig.index(name) - 1] == order[order.index(name) - 1], name                    # the binding keeps the header's order
    at = order.index
    assert at(NEW[0]) == at("gymrl_heads_loss_fwd_bwd") + 1 and at(NEW[1]) == at(NEW[0]) + 1 and at(NEW[2]) == at(NEW[1]) + 1
    _i, _vp = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES[NEW[0]] == (_i, [_i, _i, _i])
    assert _lib.SIGNATURES[NEW[1]] == (ctypes.c_size_t, [ctypes.c_int64, _i, _i])
    restype, args = _lib.SIGNATURES[NEW[2]]
    assert restype is _i and len(args) == 27 and args[1] is ctypes.c_int64 and args[25] is _i and args[26] is _vp
    assert args[15] is ctypes.POINTER(_lib.PPOCfg)
    proto = re.search(r"int gymrl_gauss_heads_loss_fwd_bwd\((.*?)\);", text, flags=re.S).group(1)
    params = [re.sub(r"\s+", " ", p).strip() for p in proto.split(",")]
    assert len(params) == 27 and params[9] == "const float* log_std" and params[10] == "const float* act"
    assert params[21] == "float* dlog_std_out" and params[24] == "void* dls_workspace" and params[25] == "int grid_blocks"


def test_ops_wrappers_refuse_before_the_library_is_called():
    z = torch.zeros
    B, C = 8, 64
    good = dict(Zac=z(B, 2 * C), bac=None, Wa2=z(1, C), ba2=z(1), Wc2=z(1, C), bc2=z(1), log_std=z(1), act=z(B, 1), logp_old=z(B),
                adv=z(B), ret=z(B), cfg=(0.2, 3.0, 0.5, 0.01), adv_moments=None, dbac=z(2 * C), dWa2=z(1, C), dba2=z(1), dWc2=z(1, C),
                dbc2=z(1), dlog_std_out=z(1), metric_parts=z(1, 5, dtype=torch.float64), workspace=z(1 << 21, dtype=torch.uint8),
                dls_workspace=z(1, dtype=torch.float64))
    for bad in (dict(Zac=z(B, 2 * 32)), dict(Zac=z(B, 2 * C + 1)), dict(Zac=z(0, 2 * C)), dict(Wa2=z(2, C)), dict(Wa2=z(1, 128)),
                dict(log_std=z(2)), dict(act=z(B)), dict(act=z(B, 1, dtype=torch.int32)), dict(logp_old=z(B + 1)),
                dict(adv=z(B, dtype=torch.float64)), dict(dlog_std_out=None), dict(dbac=None), dict(dbac=z(C)), dict(dWc2=z(2, C)),
                dict(adv_moments=z(3)), dict(metric_parts=z(1, 5)), dict(metric_parts=z(1, 4, dtype=torch.float64)),
                dict(metric_parts=z(0, 5, dtype=torch.float64)), dict(grid_blocks=-1), dict(grid_blocks=1.0), dict(dls_workspace=None),
                dict(Zac=z(2 * C, B).t())):
        with pytest.raises(ValueError):
            ops.gauss_heads_loss_fwd_bwd(**dict(good, **bad))
    with pytest.raises(ValueError):
        ops.gauss_heads_loss_fwd_bwd(**dict(good, Zac=z(33, 2 * C), act=z(33, 1), logp_old=z(33), adv=z(33), ret=z(33)))   # two batches, one row
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gauss_heads_loss_fwd_bwd(**good)
    with pytest.raises(ValueError):
        ops.gauss_heads_loss_workspace(8, 96, 1, "cpu")
