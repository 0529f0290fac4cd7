"""CPU-side checks of gymrl_dqn_act_step_classic / gymrl_dsac_act_step_classic: the DQN and discrete-SAC act launches for the env
kind the argument block names (CartPole-v1, MountainCar-v0, Acrobot-v1).  include/gymrl.h declares them beside the entry points
they generalise, the binding mirrors them, and every documented refusal is -22 before anything touches HIP: each case differs
from a fully set block in ONE field, and the block's pointers are host addresses nothing may dereference.  No compute is
launched (no GPU here)."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

FAKE = 0x1000
CARTPOLE, PENDULUM, LUNARLANDER, MOUNTAINCAR, ACROBOT = 0, 1, 2, 3, 5
DIMS = {CARTPOLE: (4, 2), MOUNTAINCAR: (2, 3), ACROBOT: (6, 3)}
# entry point -> (the entry point it stands beside, the block's mirror, the network's field)
ENTRIES = {"gymrl_dqn_act_step_classic": ("gymrl_dqn_act_step", "DqnActArgs", "policy"),
           "gymrl_dsac_act_step_classic": ("gymrl_dsac_act_step", "DsacActArgs", "actor")}
POINTERS = ("env_state", "obs", "obs_out", "r_state", "r_action", "r_reward", "r_next", "r_flag")


def _filled(name, kind=ACROBOT, N=32, H=64, D=None, A=None):
    from gymrl_amd import _lib
    a = getattr(_lib, ENTRIES[name][1])()
    a.N, a.H, a.env_kind = N, H, kind
    a.D, a.A = DIMS.get(kind, (4, 2)) if D is None else (D, A)
    for f in POINTERS:
        setattr(a, f, FAKE)
    net = getattr(a, ENTRIES[name][2])
    for k in range(3):
        net.w[k], net.b[k] = FAKE, FAKE
    a.cap, a.cursor = 1 << 20, 0
    return a


def _call(name, a):
    from gymrl_amd import _lib
    return getattr(_lib.lib(), name)(ctypes.byref(a), ctypes.c_void_p(None))


def test_header_declares_and_library_exports_both_entry_points():
    from gymrl_amd import _lib
    functions, structs = _parse_header()
    order, L = list(functions), _lib.lib()
    for name, (sibling, _, _) in ENTRIES.items():
        assert name in functions, f"{name} is not declared in include/gymrl.h"
        assert hasattr(L, name), f"{name} is not exported by the library"
        assert order.index(name) == order.index(sibling) + 1                # beside the entry point it generalises
        assert functions[name] == functions[sibling]                        # the same block: no field was added
    assert order[-1] == "gymrl_mountaincar_rule_eval"                       # the header still ends where it did


def test_binding_mirrors_them_and_the_abi_version_stays():
    from gymrl_amd import _lib, ops
    functions, _ = _parse_header()
    mirrors = _mirrors()
    table = list(_lib.SIGNATURES)
    assert table == list(functions)                                         # one order
    for name, (sibling, mirror, _) in ENTRIES.items():
        assert table.count(name) == 1 and _lib.SYMBOLS.count(name) == 1
        restype, argtypes = _lib.SIGNATURES[name]
        ret, params = functions[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params) == 2
        for ct, htype in zip(argtypes, params):
            assert _agrees(ct, htype, mirrors)
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[sibling]
        assert argtypes[0] == ctypes.POINTER(getattr(_lib, mirror))
    L = _lib.lib()
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION                   # additions only
    assert L.gymrl_dqn_args_bytes(0) == ctypes.sizeof(_lib.DqnActArgs) and L.gymrl_dsac_args_bytes(0) == ctypes.sizeof(_lib.DsacActArgs)
    assert ops.FUSED_ACT_KINDS == (ops.CARTPOLE, ops.MOUNTAINCAR, ops.ACROBOT) == (CARTPOLE, MOUNTAINCAR, ACROBOT)
    for kind, dims in DIMS.items():
        assert ops.env_dims(kind)[:2] == dims == ops.EPISODE_ENVS[kind][1:3]


def test_python_picks_the_entry_by_kind():
    """CartPole keeps the entry point it has always called; kinds 3 and 5 take the new one; Pendulum is left to the old one's refusal."""
    from gymrl_amd import ops
    for base in ("gymrl_dqn_act_step", "gymrl_dsac_act_step"):
        assert ops._classic_act_entry(base, ops.CARTPOLE) == base
        assert ops._classic_act_entry(base, ops.MOUNTAINCAR) == ops._classic_act_entry(base, ops.ACROBOT) == base + "_classic"
        assert ops._classic_act_entry(base, ops.PENDULUM) == base


@pytest.mark.parametrize("name", list(ENTRIES))
def test_refusals_come_before_any_launch(name):
    from gymrl_amd import _lib
    assert getattr(_lib.lib(), name)(None, ctypes.c_void_p(None)) == -22                       # a null args
    assert _call(name, getattr(_lib, ENTRIES[name][1])()) == -22                               # an empty block
    for kind in (PENDULUM, LUNARLANDER, 4, 6, -1):                                              # kinds without an instance
        for D, A in ((4, 2), (2, 3), (6, 3), (3, 1), (8, 4)):
            assert _call(name, _filled(name, kind, D=D, A=A)) == -22, (kind, D, A)
    # a (D, A) that is not the kind's
    assert _call(name, _filled(name, MOUNTAINCAR, D=4, A=2)) == -22
    assert _call(name, _filled(name, ACROBOT, D=2, A=3)) == -22
    assert _call(name, _filled(name, CARTPOLE, D=6, A=3)) == -22
    for kind, (D, A) in DIMS.items():
        for bad in ((D + 1, A), (D, A + 1), (D - 1, A), (D, A - 1), (0, A), (D, 0), (9, A), (D, 5)):
            assert _call(name, _filled(name, kind, D=bad[0], A=bad[1])) == -22, (kind, bad)
    for kind in DIMS:
        assert _call(name, _filled(name, kind, N=0)) == -22 and _call(name, _filled(name, kind, N=-3)) == -22
        for H in (0, 260, 6, 2, -64):
            assert _call(name, _filled(name, kind, H=H)) == -22, (kind, H)
        a = _filled(name, kind)
        a.cap = a.N - 1                                                                         # cap < N
        assert _call(name, a) == -22
        a = _filled(name, kind)
        a.cursor = -1
        assert _call(name, a) == -22
        for f in POINTERS:                                                                      # env_state, obs, obs_out, the five ring pointers
            a = _filled(name, kind)
            setattr(a, f, None)
            assert _call(name, a) == -22, (kind, f)
        for k in range(3):                                                                      # the six weight / bias slots
            for which in ("w", "b"):
                a = _filled(name, kind)
                getattr(getattr(a, ENTRIES[name][2]), which)[k] = None
                assert _call(name, a) == -22, (kind, which, k)


def test_the_old_entry_points_keep_their_kind():
    """gymrl_dqn_act_step / gymrl_dsac_act_step / gymrl_ddqn_duel_act_step refuse kinds 3 and 5 with the kinds' own shapes, as before."""
    for name, old in (("gymrl_dqn_act_step_classic", "gymrl_dqn_act_step"), ("gymrl_dqn_act_step_classic", "gymrl_ddqn_duel_act_step"),
                      ("gymrl_dsac_act_step_classic", "gymrl_dsac_act_step")):
        for kind in (MOUNTAINCAR, ACROBOT):
            assert _call(old, _filled(name, kind)) == -22
            assert _call(old, _filled(name, kind, D=4, A=2)) == -22
        assert _call(old, _filled(name, CARTPOLE, D=6, A=3)) == -22
    from gymrl_amd import _lib
    with pytest.raises(ctypes.ArgumentError):
        _lib.lib().gymrl_dqn_act_step_classic(ctypes.byref(_lib.DsacActArgs()), None)           # another struct's pointer
    with pytest.raises(ctypes.ArgumentError):
        _lib.lib().gymrl_dsac_act_step_classic(ctypes.byref(_lib.DqnActArgs()), None)
