"""CPU-side checks of the policy episode kernel's boundary: gymrl_classic_policy_eval declared, exported and mirrored, its argument
struct the size the library reports, and every pointer, size or shape error refused with -22 before anything is launched (no
GPU here)."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

CARTPOLE, PENDULUM, LUNARLANDER, MOUNTAINCAR = 0, 1, 2, 3
FAKE = 256                                             # never dereferenced: validation fails first


def _args(kind=CARTPOLE, **kw):
    from gymrl_amd import _lib
    a = _lib.ClassicEvalArgs()
    a.P, a.E, a.cap, a.env_kind = 1, 10, 500 if kind == CARTPOLE else 200, kind
    a.head, a.D, a.A, a.H, a.bound = (0, 4, 2, 64, 0.0) if kind == CARTPOLE else (1, 3, 1, 64, 2.0)
    for k in range(3):
        a.w[k] = a.b[k] = FAKE
    a.policy_stride, a.images, a.seed, a.stream_id0, a.start = 0, None, 42, 1 << 40, None
    a.returns = a.lengths = a.terminated = FAKE
    a.final_obs = None
    for k, v in kw.items():
        if k in ("w0", "w1", "w2", "b0", "b1", "b2"):
            getattr(a, k[0])[int(k[1])] = v
        else:
            assert hasattr(a, k), k
            setattr(a, k, v)
    return a


def _call(kind=CARTPOLE, **kw):
    from gymrl_amd import _lib
    return _lib.lib().gymrl_classic_policy_eval(ctypes.byref(_args(kind, **kw)), None)


def test_header_declares_and_binding_mirrors_the_entry_point():
    from gymrl_amd import _lib
    functions, structs = _parse_header()
    mirrors = _mirrors()
    L = _lib.lib()
    name = "gymrl_classic_policy_eval"
    assert name in functions and hasattr(L, name) and "gymrl_classic_eval_args_bytes" in functions
    ret, params = functions[name]
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 2
    for ct, htype in zip(argtypes, params):
        assert _agrees(ct, htype, mirrors)
    assert [f for f, _ in structs["gymrl_classic_eval_args"]] == [f for f, _ in _lib.ClassicEvalArgs._fields_] == \
        ["P", "E", "cap", "env_kind", "head", "D", "A", "H", "bound", "w", "b", "policy_stride", "images", "seed", "stream_id0",
         "start", "returns", "lengths", "terminated", "final_obs"]
    assert L.gymrl_classic_eval_args_bytes() == ctypes.sizeof(_lib.ClassicEvalArgs)
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION          # an addition


def test_the_defaults_of_this_file_are_accepted_shapes():
    """Every refusal below changes ONE field of an argument block that passes every check: the ops-side shape test agrees."""
    from gymrl_amd import ops
    assert ops.classic_eval_shape_ok(CARTPOLE, 0, 4, 2, 64) and ops.classic_eval_shape_ok(PENDULUM, 1, 3, 1, 256)
    assert not ops.classic_eval_shape_ok(CARTPOLE, 1, 4, 2, 64) and not ops.classic_eval_shape_ok(PENDULUM, 0, 3, 1, 64)
    assert not ops.classic_eval_shape_ok(CARTPOLE, 0, 4, 2, 260) and not ops.classic_eval_shape_ok(CARTPOLE, 0, 4, 2, 62)
    assert not ops.classic_eval_shape_ok(MOUNTAINCAR, 0, 2, 3, 64) and not ops.classic_eval_shape_ok(LUNARLANDER, 0, 8, 4, 64)


def test_eval_refuses_bad_arguments_before_any_launch():
    from gymrl_amd import _lib
    L = _lib.lib()
    assert L.gymrl_classic_policy_eval(None, None) == -22                                          # NULL args
    for kind in (CARTPOLE, PENDULUM):
        for req in ("w0", "w1", "w2", "b0", "b1", "b2", "returns", "lengths", "terminated"):
            assert _call(kind, **{req: None}) == -22, f"NULL {req}"
        assert _call(kind, P=0) == -22 and _call(kind, P=-1) == -22
        assert _call(kind, E=0) == -22 and _call(kind, E=-5) == -22
        assert _call(kind, cap=0) == -22 and _call(kind, cap=-1) == -22
        assert _call(kind, stream_id0=-1) == -22
        for name, bad in (("w0", 264), ("w1", 260), ("w2", 264), ("b0", 258), ("b2", 257), ("images", 264), ("start", 260),
                          ("returns", 258), ("lengths", 258), ("final_obs", 258)):
            assert _call(kind, **{name: bad}) == -22, f"misaligned {name}"
        assert _call(kind, P=3) == -22                                                             # stride 0 is ONE policy
        assert _call(kind, P=3, policy_stride=4098) == -22 and _call(kind, policy_stride=6) == -22  # % 4
        assert _call(kind, P=3, policy_stride=-4096) == -22
        assert _call(kind, P=3, policy_stride=4096, images=FAKE) == -22                            # an image is of ONE policy
        assert _call(kind, P=1 << 16, E=1 << 15, policy_stride=4096) == -22                        # P * E = 2^31
        assert _call(kind, P=46341, E=46341, policy_stride=4096) == -22                            # just above INT32_MAX
        for H in (0, 2, 62, 260, 512, -64):
            assert _call(kind, H=H) == -22, f"H = {H}"
    assert _call(CARTPOLE, cap=501) == -22 and _call(PENDULUM, cap=201) == -22                     # the TimeLimits
    # the env kinds: MountainCar, LunarLander and what nobody has
    for kind in (LUNARLANDER, MOUNTAINCAR, 4, -1):
        assert _call(env_kind=kind) == -22
    assert _call(env_kind=MOUNTAINCAR, D=2, A=3, cap=200) == -22 and _call(env_kind=LUNARLANDER, D=8, A=4) == -22
    # (head, D, A) is the kind's
    assert _call(CARTPOLE, head=1) == -22 and _call(CARTPOLE, D=3) == -22 and _call(CARTPOLE, A=3) == -22
    assert _call(CARTPOLE, A=1) == -22 and _call(CARTPOLE, head=2) == -22
    assert _call(PENDULUM, head=0) == -22 and _call(PENDULUM, D=4) == -22 and _call(PENDULUM, A=2) == -22
    assert _call(PENDULUM, env_kind=CARTPOLE) == -22 and _call(CARTPOLE, env_kind=PENDULUM) == -22
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_classic_policy_eval(ctypes.byref(_lib.MlpDesc()), None)                            # another struct's pointer


def test_ops_wrapper_refuses_wrong_shapes_and_cpu_tensors():
    import torch
    from gymrl_amd import ops
    from gymrl_amd.nn import SmallLinear
    layers = (SmallLinear(4, 64, act="relu"), SmallLinear(64, 64, act="relu"), SmallLinear(64, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.classic_policy_eval(ops.CARTPOLE, layers, 4, 42, 1 << 40, 500, ops.CLASSIC_HEAD_ARGMAX)
    with pytest.raises(ValueError):
        ops.classic_policy_eval(ops.CARTPOLE, (layers[0], layers[2], layers[2]), 4, 42, 1 << 40, 500, ops.CLASSIC_HEAD_ARGMAX)
    with pytest.raises(ValueError):
        ops.classic_policy_eval(ops.CARTPOLE, layers, 4, 42, 1 << 40, 500, ops.CLASSIC_HEAD_ARGMAX, params=torch.zeros(2, 100))
    with pytest.raises(ValueError):
        ops.lin_fwd_image(torch.zeros(36, 36))
    W = torch.arange(32 * 32, dtype=torch.float32).view(32, 32)
    img = ops.lin_fwd_image(W)
    assert sorted(img.tolist()) == W.reshape(-1).tolist()                                          # a permutation
    # lane (r, q) of (tile t, step c) holds W[16 t + r][16 c + 4 q .. + 3]
    t, c, r, q = 1, 1, 5, 2
    at = ((t * 2 + c) * 64 + q * 16 + r) * 4
    assert img[at:at + 4].tolist() == W[16 * t + r, 16 * c + 4 * q:16 * c + 4 * q + 4].tolist()


def test_the_five_configs_carry_the_switch_off():
    from gymrl_amd import ddpg_pendulum, ddqn_per_cartpole, dqn_cartpole, sac_cartpole, td3_pendulum
    for mod in (dqn_cartpole, ddqn_per_cartpole, sac_cartpole, td3_pendulum, ddpg_pendulum):
        assert mod.Config().fused_eval is False, mod.__name__
