"""CPU-side checks of the fused discrete-SAC vector step's boundary: include/gymrl.h declares its entry points and structs,
the ctypes binding says what the header says, the shape predicate draws the documented limits, and the feature is opt-in.
No compute is launched (no GPU here)."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

ENTRY_POINTS = ("gymrl_dsac_update_workspace_bytes", "gymrl_dsac_pack_images", "gymrl_dsac_args_bytes", "gymrl_dsac_act_step",
                "gymrl_dsac_update", "gymrl_softmax_rows_fwd", "gymrl_softmax_rows_bwd")
STRUCTS = {"gymrl_dsac_act_args": "DsacActArgs", "gymrl_dsac_update_args": "DsacUpdateArgs"}


def test_header_declares_the_dsac_entry_points_and_structs():
    functions, structs = _parse_header()
    for name in ENTRY_POINTS:
        assert name in functions, f"{name} is not declared in include/gymrl.h"
    for name in STRUCTS:
        assert name in structs, f"struct {name} is not declared in include/gymrl.h"
    fields = [f for f, _ in structs["gymrl_dsac_update_args"]]
    for f in ("critic1", "critic2", "critic1_target", "critic2_target", "critic1_p", "critic2_p", "adam_critic2_dev", "log_alpha",
              "alpha_t", "alpha_bias_dev", "target_entropy", "images"):
        assert f in fields
    fields = [f for f, _ in structs["gymrl_dsac_act_args"]]
    for f in ("noise_exp", "seed", "counter", "counter_dev", "cursor_dev", "action_out"):
        assert f in fields
    # additions only, after what was there
    order = list(functions)
    assert order.index("gymrl_td3_update") < order.index("gymrl_dsac_update_workspace_bytes")


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
    assert _lib.SIGNATURES["gymrl_dsac_args_bytes"][0] is ctypes.c_size_t and _lib.SIGNATURES["gymrl_dsac_update"][0] is ctypes.c_int
    names = [n for n in functions if n.startswith(("gymrl_dsac_", "gymrl_softmax_"))]
    assert [n for n in _lib.SIGNATURES if n.startswith(("gymrl_dsac_", "gymrl_softmax_"))] == names      # the header's order


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
    assert (L.gymrl_dsac_args_bytes(0), L.gymrl_dsac_args_bytes(1)) == (ctypes.sizeof(_lib.DsacActArgs), ctypes.sizeof(_lib.DsacUpdateArgs))
    assert L.gymrl_dsac_args_bytes(2) == 0
    assert L.gymrl_dsac_update_workspace_bytes(128, 4, 2, 256) > 0 and L.gymrl_dsac_update_workspace_bytes(0, 4, 2, 256) == 0
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION         # additions only


def test_null_and_empty_arguments_are_refused():
    from gymrl_amd import _lib
    L = _lib.lib()
    null = ctypes.c_void_p(None)
    assert L.gymrl_dsac_update(None, null) == -22 and L.gymrl_dsac_act_step(None, null) == -22 and L.gymrl_dsac_pack_images(None, null) == -22
    # arguments that are well typed and wrong are refused by the library before anything is launched
    assert L.gymrl_dsac_update(ctypes.byref(_lib.DsacUpdateArgs()), null) == -22
    assert L.gymrl_dsac_act_step(ctypes.byref(_lib.DsacActArgs()), null) == -22
    assert L.gymrl_dsac_pack_images(ctypes.byref(_lib.DsacUpdateArgs()), null) == -22
    assert L.gymrl_softmax_rows_fwd(null, 4, 2, null, null) == -22 and L.gymrl_softmax_rows_bwd(null, null, 4, 2, null, null) == -22
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_dsac_update(ctypes.byref(_lib.DsacActArgs()), null)             # another struct's pointer
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_dsac_act_step(ctypes.byref(_lib.Td3ActArgs()), null)


def test_shape_predicate_draws_the_documented_limits():
    from gymrl_amd import ops
    ok = ops.dsac_fused_shape_ok
    assert ok(256, 4, 2, 256) and not ok(257, 4, 2, 256)         # one grid per phase: B <= 256
    assert ok(128, 4, 2, 36) and not ok(128, 4, 2, 38)           # H % 4
    assert ok(128, 4, 2, 256) and not ok(128, 4, 2, 260)         # H <= 256
    assert ok(128, 4, 2, 256) and not ok(128, 4, 5, 256)         # A <= kMaxA
    assert not ok(128, 9, 2, 256) and not ok(0, 4, 2, 256)
    assert ops.DSAC_FUSED_MAX_BATCH == 256


def test_the_fused_step_and_the_kernel_softmax_are_opt_in():
    from gymrl_amd import sac_cartpole
    cfg = sac_cartpole.Config()
    assert cfg.fused_step is False and cfg.fused_images is True and cfg.kernel_softmax is False
    assert sac_cartpole.Actor(4, 2, 8).kernel_softmax is False
