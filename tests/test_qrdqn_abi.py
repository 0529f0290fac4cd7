"""CPU: gymrl_qr_q / gymrl_qr_loss refuse what include/gymrl.h says they refuse, before any HIP call (there is no GPU here);
the ops wrappers refuse CPU tensors and bad shapes; the two trainer modules import with the Config defaults README.md states."""
import ctypes

import pytest
import torch

fake, null = ctypes.c_void_p(256), ctypes.c_void_p(None)              # never dereferenced: validation comes first
INF, NAN = float("inf"), float("nan")


def _q(L, quant=fake, B=8, A=2, N=51, q_out=fake, argmax_out=null):
    return L.gymrl_qr_q(quant, B, A, N, q_out, argmax_out, null)


def _loss(L, B=8, A=2, N=51, kappa=1.0, loss_sum=null, workspace=null, **ptr):
    p = dict(quant=fake, next_online=null, next_target=fake, act=fake, rew=fake, flag=fake, w=null, row_loss_out=fake, dquant_out=fake)
    p.update(ptr)
    return L.gymrl_qr_loss(p["quant"], p["next_online"], p["next_target"], p["act"], p["rew"], p["flag"], p["w"], B, A, N, kappa,
                           0.99, p["row_loss_out"], p["dquant_out"], loss_sum, workspace, null)


BAD_SHAPES = [dict(A=0), dict(A=9), dict(N=0), dict(N=65), dict(B=-1)]
BAD_KAPPA = [0.0, -1.0, INF, NAN]


def test_symbols_are_exported_and_the_abi_version_stays():
    from gymrl_amd import _lib
    L = _lib.lib()
    assert L.gymrl_abi_version() == 4
    for name in ("gymrl_qr_q", "gymrl_qr_loss"):
        assert name in _lib.SIGNATURES and getattr(L, name) is not None


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from gymrl_amd import _lib
    L = _lib.lib()
    for bad in BAD_SHAPES:
        assert _q(L, **bad) == -22, bad
        assert _loss(L, **bad) == -22, bad
    for kappa in BAD_KAPPA:
        assert _loss(L, kappa=kappa) == -22, kappa
    assert _q(L, quant=null) == -22 and _q(L, q_out=null) == -22
    for name in ("quant", "next_target", "act", "rew", "flag", "row_loss_out", "dquant_out"):
        assert _loss(L, **{name: null}) == -22, name
    assert _loss(L, loss_sum=fake) == -22                               # a loss sum without the reduction's workspace
    # an empty batch is a no-op: no launch, so it returns 0 on a machine with no GPU; the optional operands may be given or not
    assert _q(L, B=0) == 0 and _q(L, B=0, argmax_out=fake) == 0 and _q(L, B=0, N=1) == 0 and _q(L, B=0, A=8, N=64) == 0
    assert _loss(L, B=0) == 0 and _loss(L, B=0, next_online=fake, w=fake, loss_sum=fake, workspace=fake) == 0
    assert _loss(L, B=0, kappa=0.5) == 0 and _loss(L, B=0, kappa=1e-30) == 0
    assert _loss(L, B=0, A=9) == -22 and _q(L, B=0, quant=null) == -22 and _loss(L, B=0, kappa=0.0) == -22   # refused at B = 0 too


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from gymrl_amd import ops
    assert (ops.QR_MAX_ACTIONS, ops.QR_MAX_QUANTILES) == (8, 64)
    x = torch.zeros(4, 2, 51)
    r, a = torch.zeros(4), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.qr_q(x.view(4, 102), 2, 51)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.qr_loss(x, x, a, r, r, 0.99)
    assert ops.qr_shape_ok(0, 1, 1, 1.0) and ops.qr_shape_ok(7, 8, 64, 0.5) and ops.qr_shape_ok(7, 8, 64)
    for bad in ((1, 0, 51, 1.0), (1, 9, 51, 1.0), (1, 2, 0, 1.0), (1, 2, 65, 1.0), (-1, 2, 51, 1.0), (1, 2, 51, 0.0), (1, 2, 51, -1.0),
                (1, 2, 51, INF), (1, 2, 51, NAN), (1, 2, 51, 1e39), (1, 2, 51, 1e-50)):      # the last two: inf and 0 as a float32
        assert not ops.qr_shape_ok(*bad), bad
    # a refused shape is a ValueError before any pointer is read
    for A, N in ((0, 51), (9, 51), (2, 0), (2, 65)):
        with pytest.raises(ValueError, match="qr_q"):
            ops.qr_q(torch.zeros(4, A * N), A, N)
        with pytest.raises(ValueError, match="qr_loss"):
            y = torch.zeros(4, A, N)
            ops.qr_loss(y, y, a, r, r, 0.99)
    for kappa in BAD_KAPPA:
        with pytest.raises(ValueError, match="qr_loss"):
            ops.qr_loss(x, x, a, r, r, 0.99, kappa)
    with pytest.raises(ValueError, match="qr_q"):
        ops.qr_q(torch.zeros(4, 100), 2, 51)                             # not A * N columns
    for name, bad in (("next_target", torch.zeros(4, 2, 50)), ("next_online", torch.zeros(3, 2, 51)), ("w", torch.zeros(5)),
                      ("loss_sum", torch.zeros(2, dtype=torch.float64))):
        kw = dict(next_target=x, next_online=None, w=None, loss_sum=None)
        kw[name] = bad
        with pytest.raises(ValueError, match=name):
            ops.qr_loss(x, kw.pop("next_target"), a, r, r, 0.99, **kw)
    for name, args in (("act", (torch.zeros(3, dtype=torch.int32), r, r)), ("rew", (a, torch.zeros(5), r)), ("flag", (a, r, torch.zeros(4, 1)))):
        with pytest.raises(ValueError, match=name):
            ops.qr_loss(x, x, *args, 0.99)


def test_trainer_modules_import_with_the_documented_defaults():
    from gymrl_amd import c51_cartpole, ddqn_per_cartpole, dqn_cartpole, qrdqn_cartpole, qrdqn_per_cartpole
    c = qrdqn_cartpole.Config()
    assert (c.num_quantiles, c.kappa, c.double_q, c.fused_step) == (51, 1.0, False, False)
    assert (c.env_name, c.gamma, c.batch_size, c.hidden_dim) == ("CartPole-v1", 0.99, 64, 256)
    assert vars(dqn_cartpole.Config()).items() <= vars(c).items()          # DQN's Config, plus the three fields
    assert set(vars(c)) - set(vars(dqn_cartpole.Config())) == {"num_quantiles", "kappa", "double_q"}      # no support to configure
    p = qrdqn_per_cartpole.Config()
    assert (p.num_quantiles, p.kappa, p.error_max, p.gamma, p.fused_step) == (51, 1.0, 0.0, 0.9, False)
    assert {k: v for k, v in vars(ddqn_per_cartpole.Config()).items() if k != "error_max"}.items() <= vars(p).items()
    assert issubclass(qrdqn_cartpole.Config, dqn_cartpole.Config) and issubclass(qrdqn_per_cartpole.Config, ddqn_per_cartpole.Config)
    Q, P = qrdqn_cartpole.QRDQNTrainer, qrdqn_per_cartpole.QRDQNPERTrainer
    assert issubclass(Q, qrdqn_cartpole.QRHead) and issubclass(Q, dqn_cartpole.DQNTrainer)
    assert issubclass(P, qrdqn_cartpole.QRHead) and issubclass(P, ddqn_per_cartpole.DDQNPERTrainer)
    assert Q.__mro__.index(qrdqn_cartpole.QRHead) < Q.__mro__.index(dqn_cartpole.DQNTrainer)
    assert P.__mro__.index(qrdqn_cartpole.QRHead) < P.__mro__.index(ddqn_per_cartpole.DDQNPERTrainer)
    assert not issubclass(Q, c51_cartpole.C51Head)
    # the head refuses a bad Config by name, before anything is built
    for field, value in (("num_quantiles", 0), ("num_quantiles", 65), ("kappa", 0.0), ("kappa", NAN), ("fused_step", True)):
        for mod, cls in ((qrdqn_cartpole, Q), (qrdqn_per_cartpole, P)):
            cfg = mod.Config()
            setattr(cfg, field, value)
            with pytest.raises(ValueError, match="fused" if field == "fused_step" else field):
                cls(cfg)
