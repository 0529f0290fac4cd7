"""CPU: gymrl_c51_q / gymrl_c51_loss refuse what include/gymrl.h says they refuse, before any HIP call (there is no GPU here);
the ops wrappers refuse CPU tensors and bad shapes; the two trainer modules import with the Config defaults README.md states."""
import ctypes

import pytest
import torch

fake, null = ctypes.c_void_p(256), ctypes.c_void_p(None)              # never dereferenced: validation comes first


def _q(L, logits=fake, B=8, A=2, M=51, vmin=0.0, vmax=100.0, q_out=fake, argmax_out=null):
    return L.gymrl_c51_q(logits, B, A, M, vmin, vmax, q_out, argmax_out, null)


def _loss(L, B=8, A=2, M=51, vmin=0.0, vmax=100.0, loss_sum=null, workspace=null, **ptr):
    p = dict(logits=fake, next_online=null, next_target=fake, act=fake, rew=fake, flag=fake, w=null, row_loss_out=fake, dlogits_out=fake)
    p.update(ptr)
    return L.gymrl_c51_loss(p["logits"], p["next_online"], p["next_target"], p["act"], p["rew"], p["flag"], p["w"], B, A, M, vmin, vmax,
                            0.99, p["row_loss_out"], p["dlogits_out"], loss_sum, workspace, null)


BAD_SHAPES = [dict(A=0), dict(A=9), dict(M=1), dict(M=65), dict(vmin=1.0, vmax=1.0), dict(vmin=2.0, vmax=1.0), dict(B=-1),
              dict(vmin=float("nan")), dict(vmin=-3e38, vmax=3e38)]          # the last: vmax - vmin overflows float32


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from gymrl_amd import _lib
    L = _lib.lib()
    for bad in BAD_SHAPES:
        assert _q(L, **bad) == -22, bad
        assert _loss(L, **bad) == -22, bad
    assert _q(L, logits=null) == -22 and _q(L, q_out=null) == -22
    for name in ("logits", "next_target", "act", "rew", "flag", "row_loss_out", "dlogits_out"):
        assert _loss(L, **{name: null}) == -22, name
    assert _loss(L, loss_sum=fake) == -22                               # a loss sum without the reduction's workspace
    # an empty batch is a no-op: no launch, so it returns 0 on a machine with no GPU; the optional operands may be given or not
    assert _q(L, B=0) == 0 and _q(L, B=0, argmax_out=fake) == 0
    assert _loss(L, B=0) == 0 and _loss(L, B=0, next_online=fake, w=fake, loss_sum=fake, workspace=fake) == 0
    assert _loss(L, B=0, A=9) == -22 and _q(L, B=0, logits=null) == -22   # ... but a refused shape is refused at B = 0 too


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from gymrl_amd import ops
    x = torch.zeros(4, 2, 51)
    r, a = torch.zeros(4), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.c51_q(x.view(4, 102), 2, 51, 0.0, 100.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.c51_loss(x, x, a, r, r, 0.99, 0.0, 100.0)
    assert ops.c51_shape_ok(0, 1, 2, 0.0, 1.0) and ops.c51_shape_ok(7, 8, 64, -1.0, 1.0)
    for bad in ((1, 0, 51, 0.0, 1.0), (1, 9, 51, 0.0, 1.0), (1, 2, 1, 0.0, 1.0), (1, 2, 65, 0.0, 1.0), (1, 2, 51, 1.0, 1.0), (-1, 2, 51, 0.0, 1.0)):
        assert not ops.c51_shape_ok(*bad), bad
    # a refused shape is a ValueError before any pointer is read
    for A, M, lo, hi in ((0, 51, 0.0, 1.0), (9, 51, 0.0, 1.0), (2, 1, 0.0, 1.0), (2, 65, 0.0, 1.0), (2, 51, 1.0, 1.0), (2, 51, 2.0, 1.0)):
        with pytest.raises(ValueError, match="c51_q"):
            ops.c51_q(torch.zeros(4, A * M), A, M, lo, hi)
        with pytest.raises(ValueError, match="c51_loss"):
            y = torch.zeros(4, A, M)
            ops.c51_loss(y, y, a, r, r, 0.99, lo, hi)
    with pytest.raises(ValueError, match="c51_q"):
        ops.c51_q(torch.zeros(4, 100), 2, 51, 0.0, 1.0)                  # not A * M columns
    for name, bad in (("next_target", torch.zeros(4, 2, 50)), ("next_online", torch.zeros(3, 2, 51)), ("w", torch.zeros(5)),
                      ("loss_sum", torch.zeros(2, dtype=torch.float64))):
        kw = dict(next_target=x, next_online=None, w=None, loss_sum=None)
        kw[name] = bad
        with pytest.raises(ValueError, match=name):
            ops.c51_loss(x, kw.pop("next_target"), a, r, r, 0.99, 0.0, 100.0, **kw)
    with pytest.raises(ValueError, match="act"):
        ops.c51_loss(x, x, torch.zeros(3, dtype=torch.int32), r, r, 0.99, 0.0, 100.0)


def test_trainer_modules_import_with_the_documented_defaults():
    from gymrl_amd import c51_cartpole, c51_per_cartpole, dqn_cartpole, ddqn_per_cartpole
    c = c51_cartpole.Config()
    assert (c.num_atoms, c.v_min, c.v_max, c.double_q, c.fused_step) == (51, 0.0, 100.0, False, False)
    assert (c.env_name, c.gamma, c.batch_size, c.hidden_dim) == ("CartPole-v1", 0.99, 64, 256)
    assert vars(dqn_cartpole.Config()).items() <= vars(c).items()          # DQN's Config, plus the four fields
    p = c51_per_cartpole.Config()
    assert (p.num_atoms, p.v_min, p.v_max, p.error_max, p.gamma, p.fused_step) == (51, 0.0, 10.0, 0.0, 0.9, False)
    assert {k: v for k, v in vars(ddqn_per_cartpole.Config()).items() if k != "error_max"}.items() <= vars(p).items()
    assert c51_cartpole.default_support("MountainCar-v0", 0.99) == (-100.0, 0.0)
    assert c51_cartpole.default_support("Acrobot-v1", 0.9) == (-10.0, 0.0)
    assert issubclass(c51_cartpole.C51Trainer, dqn_cartpole.DQNTrainer)
    assert issubclass(c51_per_cartpole.C51PERTrainer, ddqn_per_cartpole.DDQNPERTrainer)
