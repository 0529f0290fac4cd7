"""CPU-side checks of the fused TD3 / DDPG vector step's boundary: include/gymrl.h declares its entry points and structs, the
ctypes binding says what the header says, the shape predicate draws the documented limits, and the feature is opt-in.
No compute is launched (no GPU here)."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

ENTRY_POINTS = ("gymrl_td3_update_workspace_bytes", "gymrl_td3_pack_images", "gymrl_td3_args_bytes", "gymrl_td3_act_step",
                "gymrl_td3_update")
STRUCTS = {"gymrl_td3_actor_params": "Td3ActorParams", "gymrl_td3_act_args": "Td3ActArgs", "gymrl_td3_update_args": "Td3UpdateArgs"}


def test_header_declares_the_td3_entry_points_and_structs():
    functions, structs = _parse_header()
    for name in ENTRY_POINTS:
        assert name in functions, f"{name} is not declared in include/gymrl.h"
    for name in STRUCTS:
        assert name in structs, f"struct {name} is not declared in include/gymrl.h"
    fields = [f for f, _ in structs["gymrl_td3_update_args"]]
    for f in ("n_critics", "delayed", "delayed_dev", "policy_noise", "noise_clip", "actor_target", "critic_target", "images"):
        assert f in fields
    # next to the SAC ones, after them
    order = list(functions)
    assert order.index("gymrl_sac_update") < order.index("gymrl_td3_act_step")


def test_signatures_match_the_header():
    from gymrl_amd import _lib
    functions, _ = _parse_header()
    mirrors = _mirrors()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        ret, params = functions[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters in the header, {len(argtypes)} in the table"
        for i, (ct, htype) in enumerate(zip(argtypes, params)):
            assert _agrees(ct, htype, mirrors), f"{name}: parameter {i}"
    assert restype_of(_lib, "gymrl_td3_args_bytes") is ctypes.c_size_t and restype_of(_lib, "gymrl_td3_update") is ctypes.c_int
    # the header's order
    names = [n for n in functions if n.startswith("gymrl_td3_")]
    assert [n for n in _lib.SIGNATURES if n.startswith("gymrl_td3_")] == names


def restype_of(_lib, name):
    return _lib.SIGNATURES[name][0]


def test_mirrors_match_their_structs_field_by_field():
    from gymrl_amd import _lib
    _, structs = _parse_header()
    mirrors = _mirrors()
    for cname, pyname in STRUCTS.items():
        cls = getattr(_lib, pyname)
        assert cls._c_name_ == cname and mirrors[cname] is cls
        assert [f for f, _ in cls._fields_] == [f for f, _ in structs[cname]], f"{cname}: field names or their order differ"
        for (fname, ct), (_, htype) in zip(cls._fields_, structs[cname]):
            assert _agrees(ct, htype, mirrors), f"{cname}.{fname}"
    L = _lib.lib()
    assert (L.gymrl_td3_args_bytes(0), L.gymrl_td3_args_bytes(1)) == (ctypes.sizeof(_lib.Td3ActArgs), ctypes.sizeof(_lib.Td3UpdateArgs))
    assert L.gymrl_td3_args_bytes(2) == 0
    assert L.gymrl_td3_update_workspace_bytes(128, 3, 1, 256) > 0 and L.gymrl_td3_update_workspace_bytes(0, 3, 1, 256) == 0


def test_a_mistyped_argument_raises():
    from gymrl_amd import _lib
    L = _lib.lib()
    null = ctypes.c_void_p(None)
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_td3_update(ctypes.byref(_lib.Td3ActArgs()), null)              # another struct's pointer
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_td3_act_step(ctypes.byref(_lib.SacActArgs()), null)
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_td3_update_workspace_bytes(128, 3, 1, 256.0)                   # float for an int
    with pytest.raises(TypeError):
        L.gymrl_td3_args_bytes()                                               # a missing argument
    # arguments that are well typed and wrong are refused by the library before anything is launched
    assert L.gymrl_td3_update(ctypes.byref(_lib.Td3UpdateArgs()), null) == -22
    assert L.gymrl_td3_act_step(ctypes.byref(_lib.Td3ActArgs()), null) == -22
    assert L.gymrl_td3_pack_images(ctypes.byref(_lib.Td3UpdateArgs()), null) == -22


def test_shape_predicate_draws_the_documented_limits():
    from gymrl_amd import ops
    assert ops.td3_fused_shape_ok(128, 3, 1, 256)
    assert ops.td3_fused_shape_ok(256, 8, 4, 4)
    assert not ops.td3_fused_shape_ok(128, 3, 1, 258)       # H % 4
    assert not ops.td3_fused_shape_ok(128, 3, 1, 260)       # H <= 256
    assert not ops.td3_fused_shape_ok(128, 9, 1, 256)
    assert not ops.td3_fused_shape_ok(128, 3, 5, 256)
    assert not ops.td3_fused_shape_ok(257, 3, 1, 256)       # one grid per phase: B <= 256
    assert not ops.td3_fused_shape_ok(0, 3, 1, 256)
    assert ops.TD3_FUSED_MAX_BATCH == 256


def test_the_fused_step_is_opt_in():
    from gymrl_amd import ddpg_pendulum, td3_pendulum
    for mod in (td3_pendulum, ddpg_pendulum):
        cfg = mod.Config()
        assert cfg.fused_step is False
        assert cfg.fused_images is True
