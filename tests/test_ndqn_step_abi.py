"""CPU-side checks of the fused NoisyNet DQN step's boundary: include/gymrl.h declares its entry points and structs, the ctypes
binding says what the header says, the library refuses bad shapes and null pointers with -22 before anything touches HIP, the
shape predicate draws the documented limits, and the feature is opt-in.  No compute is launched (no GPU here)."""
import ctypes

from test_abi import _agrees, _mirrors, _parse_header

ENTRY_POINTS = ("gymrl_ndqn_args_bytes", "gymrl_ndqn_combine", "gymrl_ndqn_act_step", "gymrl_ndqn_update_workspace_bytes",
                "gymrl_ndqn_update")
STRUCTS = {"gymrl_ndqn_params": "NdqnParams", "gymrl_ndqn_combine_args": "NdqnCombineArgs", "gymrl_ndqn_act_args": "NdqnActArgs",
           "gymrl_ndqn_update_args": "NdqnUpdateArgs"}
DUMMY = 0x1000
RING = ("r_state", "r_action", "r_reward", "r_next", "r_flag")


def test_header_declares_the_ndqn_entry_points_and_structs():
    functions, structs = _parse_header()
    for name in ENTRY_POINTS:
        assert name in functions, f"{name} is not declared in include/gymrl.h"
    for cname in STRUCTS:
        assert cname in structs
    fields = [f for f, _ in structs["gymrl_ndqn_update_args"]]
    for f in RING + ("cap", "idx", "idx_dev", "policy", "target", "policy_p", "policy_m", "policy_v", "adam_policy", "adam_policy_dev",
                     "loss_sum", "workspace"):
        assert f in fields
    assert [f for f, _ in structs["gymrl_ndqn_params"]] == ["w_mu", "w_sigma", "b_mu", "b_sigma"]
    order = list(functions)
    assert order.index("gymrl_ddqn_duel_act_step") < order.index("gymrl_ndqn_args_bytes")      # additions only, after what was there


def test_signatures_match_the_header_in_its_order():
    from gymrl_amd import _lib
    functions, _ = _parse_header()
    mirrors = _mirrors()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and _lib.SYMBOLS.count(name) == 1
        ret, params = functions[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(params)
        for i, (ct, htype) in enumerate(zip(argtypes, params)):
            assert _agrees(ct, htype, mirrors), f"{name}: parameter {i}"
    names = [n for n in functions if n.startswith("gymrl_ndqn_")]
    assert [n for n in _lib.SIGNATURES if n.startswith("gymrl_ndqn_")] == names == list(ENTRY_POINTS)
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name)


def test_mirrors_match_their_structs_field_by_field():
    from gymrl_amd import _lib
    _, structs = _parse_header()
    mirrors = _mirrors()
    for cname, pyname in STRUCTS.items():
        cls = getattr(_lib, pyname)
        assert cls._c_name_ == cname and mirrors[cname] is cls
        assert [f for f, _ in cls._fields_] == [f for f, _ in structs[cname]], cname
        for (fname, ct), (_, htype) in zip(cls._fields_, structs[cname]):
            assert _agrees(ct, htype, mirrors), f"{cname}.{fname}"
    L = _lib.lib()
    assert L.gymrl_ndqn_args_bytes(0) == ctypes.sizeof(_lib.NdqnActArgs)
    assert L.gymrl_ndqn_args_bytes(1) == ctypes.sizeof(_lib.NdqnUpdateArgs)
    assert L.gymrl_ndqn_args_bytes(2) == ctypes.sizeof(_lib.NdqnCombineArgs) and L.gymrl_ndqn_args_bytes(3) == 0
    assert L.gymrl_ndqn_update_workspace_bytes(64, 4, 2, 64) > 3 * 4 * (64 * 5 + 64 * 65 + 65 + 2 * 65)      # three parameter sets and more
    assert L.gymrl_ndqn_update_workspace_bytes(0, 4, 2, 64) == 0
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION         # additions only


def _net(n, sigma=True):
    for k in range(4):
        n.w_mu[k], n.b_mu[k] = DUMMY, DUMMY
        if sigma:
            n.w_sigma[k], n.b_sigma[k] = DUMMY, DUMMY


def _combine(**ch):
    from gymrl_amd import _lib
    a = _lib.NdqnCombineArgs()
    a.D, a.A, a.H, a.workspace = 4, 2, 64, DUMMY
    _net(a.policy)
    for f, v in ch.items():
        setattr(a, f, v)
    return a


def _act(**ch):
    from gymrl_amd import _lib, ops
    a = _lib.NdqnActArgs()
    a.N, a.D, a.A, a.H, a.cap, a.cursor, a.env_kind = 20, 4, 2, 64, 20, 0, ops.CARTPOLE
    for f in ("env_state", "obs", "obs_out", "workspace") + RING:
        setattr(a, f, DUMMY)
    for f, v in ch.items():
        setattr(a, f, v)
    return a


def _update(**ch):
    from gymrl_amd import _lib
    a = _lib.NdqnUpdateArgs()
    a.B, a.D, a.A, a.H, a.cap, a.idx = 24, 4, 2, 64, 1 << 10, DUMMY
    for f in RING + ("policy_p", "policy_m", "policy_v", "loss_sum", "workspace"):
        setattr(a, f, DUMMY)
    _net(a.policy)
    _net(a.target, sigma=False)
    for f, v in ch.items():
        setattr(a, f, v)
    return a


def test_refusals_come_before_any_launch():
    """-22 for every documented refusal; each case differs from an acceptable block in ONE field (a fully valid block is never
    passed: it would launch on the dummy addresses)."""
    from gymrl_amd import _lib
    L = _lib.lib()
    null = ctypes.c_void_p(None)
    for fn in (L.gymrl_ndqn_combine, L.gymrl_ndqn_act_step, L.gymrl_ndqn_update):
        assert fn(None, null) == -22
    shapes = (dict(A=3), dict(A=1), dict(A=0), dict(A=5), dict(D=9), dict(D=0), dict(H=0), dict(H=260), dict(H=62), dict(H=2))
    for ch in shapes + (dict(workspace=None),):
        assert L.gymrl_ndqn_combine(ctypes.byref(_combine(**ch)), null) == -22, ch
    for ch in shapes + (dict(B=0), dict(B=257), dict(cap=0), dict(idx=None, idx_size=23)) + tuple({f: None} for f in RING + (
            "policy_p", "policy_m", "policy_v", "loss_sum", "workspace")):
        assert L.gymrl_ndqn_update(ctypes.byref(_update(**ch)), null) == -22, ch
    for ch in (dict(N=0), dict(D=5), dict(D=3), dict(A=3), dict(H=0), dict(H=260), dict(H=62), dict(cap=19), dict(env_kind=2), dict(cursor=-1)) + tuple(
            {f: None} for f in ("env_state", "obs", "obs_out", "workspace") + RING):
        assert L.gymrl_ndqn_act_step(ctypes.byref(_act(**ch)), null) == -22, ch
    for member, sigma in (("policy", True), ("target", False)):
        for kind in ("w_mu", "b_mu") + (("w_sigma", "b_sigma") if sigma else ()):
            for k in range(4):
                a = _update()
                getattr(getattr(a, member), kind)[k] = None
                assert L.gymrl_ndqn_update(ctypes.byref(a), null) == -22, (member, kind, k)
    for kind in ("w_mu", "w_sigma", "b_mu", "b_sigma"):
        a = _combine()
        getattr(a.policy, kind)[2] = None
        assert L.gymrl_ndqn_combine(ctypes.byref(a), null) == -22, kind


def test_shape_predicate_and_opt_in():
    from gymrl_amd import noisy_dqn_cartpole, ops
    ok = ops.ndqn_fused_shape_ok
    assert ok(256, 4, 2, 256) and not ok(257, 4, 2, 256) and not ok(0, 4, 2, 64)
    assert ok(64, 4, 2, 36) and not ok(64, 4, 2, 38) and not ok(64, 4, 2, 20 + 2) and ok(64, 4, 2, 20)
    assert not ok(64, 4, 3, 64) and not ok(64, 4, 1, 64) and not ok(64, 9, 2, 64) and not ok(64, 4, 2, 260)
    assert ops.NDQN_FUSED_MAX_BATCH == 256 and ops.ndqn_raw_len(4, 2, 32) == 167
    assert noisy_dqn_cartpole.Config().fused_step is False
