"""CPU-side checks of the fused DDQN + PER update's boundary: include/gymrl.h declares its entry points and struct, the ctypes
binding says what the header says, the library refuses bad shapes and null pointers with -22 before anything touches HIP, the
shape predicate draws the documented limits, and the feature is opt-in.  No compute is launched (no GPU here)."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

ENTRY_POINTS = ("gymrl_ddqn_update_workspace_bytes", "gymrl_ddqn_pack_images", "gymrl_ddqn_args_bytes", "gymrl_ddqn_update",
                "gymrl_ddqn_duel_act_step")
STRUCTS = {"gymrl_ddqn_update_args": "DdqnUpdateArgs"}


def test_header_declares_the_ddqn_entry_points_and_struct():
    functions, structs = _parse_header()
    for name in ENTRY_POINTS:
        assert name in functions, f"{name} is not declared in include/gymrl.h"
    fields = [f for f, _ in structs["gymrl_ddqn_update_args"]]
    for f in ("dueling", "cap", "idx", "is_weight", "policy", "target", "policy_p", "policy_m", "policy_v", "adam_policy", "adam_policy_dev", "clamp_abs",
              "td_out", "loss_sum", "workspace", "images"):
        assert f in fields
    order = list(functions)
    assert order.index("gymrl_dqn_update") < order.index("gymrl_ddqn_update_workspace_bytes")      # additions only, after what was there


def test_signatures_match_the_header():
    from gymrl_amd import _lib
    functions, _ = _parse_header()
    mirrors = _mirrors()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        assert name in _lib.SYMBOLS and _lib.SYMBOLS.count(name) == 1
        ret, params = functions[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters in the header, {len(argtypes)} in the table"
        for i, (ct, htype) in enumerate(zip(argtypes, params)):
            assert _agrees(ct, htype, mirrors), f"{name}: parameter {i}"
    assert _lib.SIGNATURES["gymrl_ddqn_args_bytes"][0] is ctypes.c_size_t and _lib.SIGNATURES["gymrl_ddqn_update"][0] is ctypes.c_int
    assert _lib.SIGNATURES["gymrl_ddqn_update_workspace_bytes"][0] is ctypes.c_size_t
    names = [n for n in functions if n.startswith("gymrl_ddqn_")]
    assert [n for n in _lib.SIGNATURES if n.startswith("gymrl_ddqn_")] == names == list(ENTRY_POINTS)      # the header's order
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), f"{name} is not exported by the library"


def test_mirror_matches_its_struct_field_by_field():
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
    assert L.gymrl_ddqn_args_bytes(1) == ctypes.sizeof(_lib.DdqnUpdateArgs)
    assert L.gymrl_ddqn_args_bytes(0) == 0 and L.gymrl_ddqn_args_bytes(2) == 0
    assert L.gymrl_ddqn_update_workspace_bytes(64, 4, 2, 256) > 0 and L.gymrl_ddqn_update_workspace_bytes(0, 4, 2, 256) == 0
    # the third chain keeps nothing for the tile phase: the hand-off is DQN's
    assert L.gymrl_ddqn_update_workspace_bytes(64, 4, 2, 256) == L.gymrl_dqn_update_workspace_bytes(64, 4, 2, 256)
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION         # additions only


POINTERS = ("r_state", "r_action", "r_reward", "r_next", "r_flag", "idx", "is_weight", "policy_p", "policy_m", "policy_v", "td_out",
            "loss_sum", "workspace")


def _filled_update(B=64, D=4, A=2, H=64):
    """A gymrl_ddqn_update_args whose every pointer is set (to a host address nothing may touch: a refusal comes before HIP)."""
    from gymrl_amd import _lib
    a = _lib.DdqnUpdateArgs()
    a.B, a.D, a.A, a.H, a.gamma, a.clamp_abs, a.cap = B, D, A, H, 0.9, 1.0, 1 << 16
    dummy = 0x1000
    for f in POINTERS:
        setattr(a, f, dummy)
    for net in (a.policy, a.target):
        for k in range(3):
            net.w[k], net.b[k] = dummy, dummy
    a.beta1, a.beta2, a.eps_adam = 0.9, 0.999, 1e-8
    return a


def test_bad_shapes_and_null_pointers_are_refused_without_a_device():
    """-22 for every documented refusal.  Each case differs from a fully set argument block in ONE field, so the refusal is that
    field's (the block itself would be taken: its pointers are never dereferenced on the host, and this machine has no device
    a launch could reach)."""
    from gymrl_amd import _lib
    L = _lib.lib()
    null = ctypes.c_void_p(None)
    assert L.gymrl_ddqn_update(None, null) == -22 and L.gymrl_ddqn_pack_images(None, null) == -22
    assert L.gymrl_ddqn_update(ctypes.byref(_lib.DdqnUpdateArgs()), null) == -22
    assert L.gymrl_ddqn_pack_images(ctypes.byref(_lib.DdqnUpdateArgs()), null) == -22
    for change in (dict(B=257), dict(B=300), dict(B=0), dict(H=0), dict(H=260), dict(H=38), dict(D=9), dict(D=0), dict(A=5), dict(A=0)):
        a = _filled_update(**{**dict(B=64, D=4, A=2, H=64), **change})
        assert L.gymrl_ddqn_update(ctypes.byref(a), null) == -22, change
    for f in POINTERS:
        a = _filled_update()
        setattr(a, f, None)
        assert L.gymrl_ddqn_update(ctypes.byref(a), null) == -22, f
    for net in ("policy", "target"):
        for k in range(3):
            for which in ("w", "b"):
                a = _filled_update()
                getattr(getattr(a, net), which)[k] = None
                assert L.gymrl_ddqn_update(ctypes.byref(a), null) == -22, (net, which, k)
    for change in (dict(clamp_abs=-1.0), dict(cap=0), dict(dueling=2), dict(dueling=-1)):
        a = _filled_update()
        for f, v in change.items():
            setattr(a, f, v)
        assert L.gymrl_ddqn_update(ctypes.byref(a), null) == -22, change
    for A in (3, 4, 1):                                                       # the dueling combine is pinned for two actions
        a = _filled_update(A=A)
        a.dueling = 1
        assert L.gymrl_ddqn_update(ctypes.byref(a), null) == -22, A
    a = _filled_update(H=64)
    a.images, a.dueling = 0x1000, 1
    assert L.gymrl_ddqn_pack_images(ctypes.byref(a), null) == -22            # the dueling net has no H x H layer
    assert L.gymrl_ddqn_duel_act_step(None, null) == -22
    assert L.gymrl_ddqn_duel_act_step(ctypes.byref(_lib.DqnActArgs()), null) == -22
    from test_dqn_step_abi import _filled_act
    for change in (dict(N=0), dict(H=0), dict(H=260), dict(D=3), dict(A=3)):
        a = _filled_act(**{**dict(N=32, D=4, A=2, H=64), **change})
        assert L.gymrl_ddqn_duel_act_step(ctypes.byref(a), null) == -22, change
    for f in ("env_state", "obs", "obs_out", "r_state", "r_flag"):
        a = _filled_act()
        setattr(a, f, None)
        assert L.gymrl_ddqn_duel_act_step(ctypes.byref(a), null) == -22, f
    a = _filled_update(H=64)
    assert L.gymrl_ddqn_pack_images(ctypes.byref(a), null) == -22            # no images buffer
    a.images, a.H = 0x1000, 36
    assert L.gymrl_ddqn_pack_images(ctypes.byref(a), null) == -22            # not whole 16-column tiles
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_ddqn_update(ctypes.byref(_lib.DqnUpdateArgs()), null)         # another struct's pointer


def test_shape_predicate_draws_the_documented_limits():
    from gymrl_amd import ops
    ok = ops.ddqn_fused_shape_ok
    assert ok(256, 4, 2, 256) and not ok(257, 4, 2, 256)         # one grid in the row phase: B <= 256
    assert ok(64, 4, 2, 36) and not ok(64, 4, 2, 38)             # H % 4
    assert ok(64, 4, 2, 256) and not ok(64, 4, 2, 260)           # H <= 256
    assert ok(64, 4, 4, 256) and not ok(64, 4, 5, 256)           # A <= kMaxA
    assert ok(64, 8, 2, 256) and not ok(64, 9, 2, 256) and not ok(0, 4, 2, 256)
    assert ok(64, 4, 2, 256, dueling=True) and not ok(64, 4, 3, 256, dueling=True) and ok(64, 4, 3, 256)
    assert ops.DDQN_FUSED_MAX_BATCH == 256
