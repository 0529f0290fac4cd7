"""CPU-side checks of the MountainCar-v0 boundary: env kind 3 in the size queries, gymrl_mountaincar_rule_eval declared, exported
and mirrored, and every pointer or size error refused with -22 before anything is launched (no GPU here)."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

MOUNTAINCAR = 3
FAKE = 256                                             # never dereferenced: validation fails first


def _args(**kw):
    from gymrl_amd import _lib
    a = _lib.MountainCarEvalArgs()
    a.P, a.E, a.cap, a.seed, a.stream_id0 = 1, 10, 200, 42, 1 << 40
    a.coefs, a.start, a.final_state = None, None, None
    a.returns = a.lengths = a.reached = FAKE
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def _call(**kw):
    from gymrl_amd import _lib
    return _lib.lib().gymrl_mountaincar_rule_eval(ctypes.byref(_args(**kw)), None)


def test_size_queries():
    from gymrl_amd import _lib, ops
    L = _lib.lib()
    assert ops.MOUNTAINCAR == MOUNTAINCAR and ops.ENV_KINDS["MountainCar-v0"] == MOUNTAINCAR
    assert L.gymrl_env_obs_dim(3) == 2 and L.gymrl_env_act_dim(3) == 3
    assert L.gymrl_env_is_discrete(3) == 1 and L.gymrl_env_max_steps(3) == 200
    assert ops.env_dims(ops.MOUNTAINCAR) == (2, 3, True, 200)
    # five SoA fields (three f64, two 32-bit), each padded to 256 bytes
    assert L.gymrl_env_state_bytes(3, 1) == 5 * 256
    assert L.gymrl_env_state_bytes(3, 65) == 3 * 768 + 2 * 512
    assert L.gymrl_env_state_bytes(3, 4096) == 4096 * (3 * 8 + 2 * 4)
    assert L.gymrl_env_state_bytes(3, 0) == 0
    assert L.gymrl_env_obs_dim(4) == -22 and L.gymrl_env_state_bytes(4, 8) == 0      # the next kind is still nobody's
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION


def test_stepper_entry_points_refuse_null_like_the_other_kinds():
    from gymrl_amd import _lib
    L = _lib.lib()
    null, fake = None, FAKE
    for kind in (0, 1, 2, MOUNTAINCAR):
        assert L.gymrl_env_step(kind, null, 8, 42, 0, fake, fake, null, fake, fake, fake, null, null, null, null, null) == -22
        assert L.gymrl_env_step(kind, fake, 8, 42, 0, null, fake, null, fake, fake, fake, null, null, null, null, null) == -22
        assert L.gymrl_env_step(kind, fake, 8, 42, 0, fake, null, null, fake, fake, fake, null, null, null, null, null) == -22
        assert L.gymrl_env_step(kind, fake, 8, 42, 0, fake, fake, null, null, fake, fake, null, null, null, null, null) == -22
        assert L.gymrl_env_step(kind, fake, 8, 42, 0, fake, fake, null, fake, null, fake, null, null, null, null, null) == -22
        assert L.gymrl_env_step(kind, fake, 8, 42, 0, fake, fake, null, fake, fake, null, null, null, null, null, null) == -22
        assert L.gymrl_env_step(kind, 260, 8, 42, 0, fake, fake, null, fake, fake, fake, null, null, null, null, null) == -22    # misaligned
        assert L.gymrl_env_step(kind, fake, 0, 42, 0, fake, fake, null, fake, fake, fake, null, null, null, null, null) == 0      # no envs
        assert L.gymrl_env_reset(kind, null, 8, 42, 0, fake, null) == -22 and L.gymrl_env_reset(kind, fake, 8, 42, 0, null, null) == -22
        assert L.gymrl_env_reset(kind, fake, 0, 42, 0, fake, null) == 0
    assert L.gymrl_env_abandon(MOUNTAINCAR, null, 8, 42, 0, 50, fake, null, null, null, null, null) == -22
    assert L.gymrl_env_abandon(MOUNTAINCAR, fake, 8, 42, 0, 0, fake, null, null, null, null, null) == -22          # cap
    assert L.gymrl_env_abandon(MOUNTAINCAR, fake, 0, 42, 0, 50, fake, null, null, null, null, null) == 0
    assert L.gymrl_env_abandon(2, fake, 0, 42, 0, 50, fake, null, null, null, null, null) == -22                   # LunarLander: as before
    assert L.gymrl_env_refill(MOUNTAINCAR, fake, 8, 42, 0, null) == 0 and L.gymrl_env_refill(MOUNTAINCAR, null, 8, 42, 0, null) == -22
    assert L.gymrl_env_step(4, fake, 8, 42, 0, fake, fake, null, fake, fake, fake, null, null, null, null, null) == -22


def test_learner_kernels_refuse_the_kind():
    """No learner runs on MountainCar: the fused acting kernels and the rollout kernels keep returning -22 for kind 3."""
    from gymrl_amd import _lib
    L = _lib.lib()
    for cls, fn in ((_lib.SacActArgs, L.gymrl_sac_act_step), (_lib.Td3ActArgs, L.gymrl_td3_act_step), (_lib.DsacActArgs, L.gymrl_dsac_act_step),
                    (_lib.DqnActArgs, L.gymrl_dqn_act_step), (_lib.DqnActArgs, L.gymrl_ddqn_duel_act_step),
                    (_lib.RainbowActArgs, L.gymrl_rainbow_act_step), (_lib.NdqnActArgs, L.gymrl_ndqn_act_step)):
        a = cls()
        a.N, a.D, a.A, a.H, a.env_kind = 8, 2, 3, 64, MOUNTAINCAR
        a.env_state = a.obs = a.obs_out = FAKE
        assert fn(ctypes.byref(a), None) == -22, fn.__name__


def test_header_declares_and_binding_mirrors_the_entry_point():
    from gymrl_amd import _lib
    functions, structs = _parse_header()
    mirrors = _mirrors()
    name = "gymrl_mountaincar_rule_eval"
    assert name in functions and hasattr(_lib.lib(), name) and list(functions)[-1] == name          # an addition, at the end
    ret, params = functions[name]
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 2
    for ct, htype in zip(argtypes, params):
        assert _agrees(ct, htype, mirrors)
    assert [f for f, _ in structs["gymrl_mountaincar_eval_args"]] == [f for f, _ in _lib.MountainCarEvalArgs._fields_] == \
        ["P", "E", "cap", "seed", "stream_id0", "coefs", "start", "returns", "lengths", "reached", "final_state"]


def test_rule_eval_refuses_bad_arguments_before_any_launch():
    from gymrl_amd import _lib
    L = _lib.lib()
    assert L.gymrl_mountaincar_rule_eval(None, None) == -22                                        # NULL args
    for out in ("returns", "lengths", "reached"):
        assert _call(**{out: None}) == -22, f"NULL {out}"
    assert _call(P=0) == -22 and _call(P=-1) == -22
    assert _call(E=0) == -22 and _call(E=-5) == -22
    assert _call(cap=0) == -22 and _call(cap=201) == -22 and _call(cap=-1) == -22
    assert _call(P=2) == -22 and _call(P=3, coefs=None) == -22                                     # the reference's constants are ONE policy
    assert _call(P=1 << 16, E=1 << 15, coefs=FAKE) == -22                                          # P * E = 2^31
    assert _call(P=46341, E=46341, coefs=FAKE) == -22                                              # just above INT32_MAX
    assert _call(stream_id0=-1) == -22
    for name, bad in (("coefs", 260), ("start", 260), ("returns", 260), ("lengths", 258), ("final_state", 260)):
        assert _call(**{name: bad}) == -22, f"misaligned {name}"
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_mountaincar_rule_eval(ctypes.byref(_lib.MlpDesc()), None)                          # another struct's pointer


def test_ops_wrapper_refuses_wrong_shapes_and_cpu_tensors():
    import torch
    from gymrl_amd import ops
    assert ops.MOUNTAINCAR_RULE_COEFS == (-0.09, 0.25, 0.03, 0.3, 0.9, 0.008, -0.07, 0.38, 0.07)
    with pytest.raises(ValueError):
        ops.mountaincar_rule_eval(4, 42, 1 << 40, 200, "cpu", coefs=torch.zeros(2, 8, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.mountaincar_rule_eval(4, 42, 1 << 40, 200, "cpu", start=torch.zeros(1, 3, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mountaincar_rule_eval(4, 42, 1 << 40, 200, "cpu", coefs=torch.zeros(2, 9, dtype=torch.float64))
    from gymrl_amd.envs import VecEnv
    with pytest.raises(ValueError, match="MountainCar-v0"):
        VecEnv("MountainCar-v1", 1, device="cpu")                                                  # the message lists what there is
