"""CPU-side checks of the dueling episode kernel's boundary: gymrl_classic_duel_eval declared, exported and mirrored, its argument
struct the size the library reports, and every pointer, size or shape error refused with -22 before anything is launched (no
GPU here)."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

CARTPOLE, PENDULUM, LUNARLANDER, MOUNTAINCAR = 0, 1, 2, 3
FAKE = 256                                             # never dereferenced: validation fails first
FIELDS = ["P", "E", "cap", "env_kind", "n_hidden", "D", "A", "H", "w", "b", "value_w", "value_b", "adv_w", "adv_b", "policy_stride",
          "images", "seed", "stream_id0", "start", "returns", "lengths", "terminated", "final_obs"]


def _args(nh=2, **kw):
    from gymrl_amd import _lib
    a = _lib.ClassicDuelEvalArgs()
    a.P, a.E, a.cap, a.env_kind = 1, 10, 500, CARTPOLE
    a.n_hidden, a.D, a.A, a.H = nh, 4, 2, 64
    for k in range(2):
        a.w[k] = a.b[k] = FAKE if k < nh else None
    a.value_w = a.value_b = a.adv_w = a.adv_b = FAKE
    a.policy_stride, a.images, a.seed, a.stream_id0, a.start = 0, None, 42, 1 << 40, None
    a.returns = a.lengths = a.terminated = FAKE
    a.final_obs = None
    for k, v in kw.items():
        if k in ("w0", "w1", "b0", "b1"):
            getattr(a, k[0])[int(k[1])] = v
        else:
            assert hasattr(a, k), k
            setattr(a, k, v)
    return a


def _call(nh=2, **kw):
    from gymrl_amd import _lib
    return _lib.lib().gymrl_classic_duel_eval(ctypes.byref(_args(nh, **kw)), None)


def test_header_declares_and_binding_mirrors_the_entry_point():
    from gymrl_amd import _lib
    functions, structs = _parse_header()
    mirrors = _mirrors()
    L = _lib.lib()
    name = "gymrl_classic_duel_eval"
    assert name in functions and hasattr(L, name) and "gymrl_classic_duel_eval_args_bytes" in functions
    ret, params = functions[name]
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 2
    for ct, htype in zip(argtypes, params):
        assert _agrees(ct, htype, mirrors)
    assert [f for f, _ in structs["gymrl_classic_duel_eval_args"]] == [f for f, _ in _lib.ClassicDuelEvalArgs._fields_] == FIELDS
    assert L.gymrl_classic_duel_eval_args_bytes() == ctypes.sizeof(_lib.ClassicDuelEvalArgs)
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION          # an addition
    # directly behind gymrl_classic_policy_eval, in front of the MountainCar section
    names = list(functions)
    at = names.index("gymrl_classic_policy_eval")
    assert names[at + 1:at + 4] == ["gymrl_classic_duel_eval_args_bytes", name, "gymrl_mountaincar_rule_eval"]


def test_the_defaults_of_this_file_are_accepted_shapes():
    """Every refusal below changes ONE field of an argument block that passes every check (it is never sent as it is: its pointers
    are fakes): the ops-side shape test agrees with its defaults."""
    from gymrl_amd import ops
    assert ops.classic_duel_eval_shape_ok(CARTPOLE, 1, 4, 2, 64) and ops.classic_duel_eval_shape_ok(CARTPOLE, 2, 4, 2, 256)
    assert ops.classic_duel_eval_shape_ok(CARTPOLE, 2, 4, 2, 36)
    assert not ops.classic_duel_eval_shape_ok(CARTPOLE, 0, 4, 2, 64) and not ops.classic_duel_eval_shape_ok(CARTPOLE, 3, 4, 2, 64)
    assert not ops.classic_duel_eval_shape_ok(CARTPOLE, 2, 4, 3, 64) and not ops.classic_duel_eval_shape_ok(CARTPOLE, 2, 3, 2, 64)
    assert not ops.classic_duel_eval_shape_ok(CARTPOLE, 2, 4, 2, 260) and not ops.classic_duel_eval_shape_ok(CARTPOLE, 2, 4, 2, 62)
    assert not ops.classic_duel_eval_shape_ok(PENDULUM, 2, 3, 1, 64) and not ops.classic_duel_eval_shape_ok(MOUNTAINCAR, 2, 2, 3, 64)
    assert not ops.classic_duel_eval_shape_ok(LUNARLANDER, 2, 8, 4, 64)


def test_eval_refuses_bad_arguments_before_any_launch():
    from gymrl_amd import _lib
    L = _lib.lib()
    assert L.gymrl_classic_duel_eval(None, None) == -22                                            # NULL args
    for nh in (1, 2):
        required = ["w0", "b0", "value_w", "value_b", "adv_w", "adv_b", "returns", "lengths", "terminated"] + (["w1", "b1"] if nh == 2 else [])
        for req in required:
            assert _call(nh, **{req: None}) == -22, f"NULL {req}"
        assert _call(nh, P=0) == -22 and _call(nh, P=-1) == -22
        assert _call(nh, E=0) == -22 and _call(nh, E=-5) == -22
        assert _call(nh, cap=0) == -22 and _call(nh, cap=-1) == -22 and _call(nh, cap=501) == -22      # CartPole's TimeLimit
        assert _call(nh, stream_id0=-1) == -22
        misaligned = [("w0", 264), ("b0", 258), ("value_w", 264), ("value_b", 257), ("adv_w", 260), ("adv_b", 258), ("start", 260),
                      ("returns", 258), ("lengths", 258), ("final_obs", 258)] + ([("w1", 260), ("b1", 258), ("images", 264)] if nh == 2 else [])
        for name, bad in misaligned:
            assert _call(nh, **{name: bad}) == -22, f"misaligned {name}"
        assert _call(nh, P=3) == -22                                                               # stride 0 is ONE policy
        assert _call(nh, P=3, policy_stride=4098) == -22 and _call(nh, policy_stride=6) == -22     # % 4
        assert _call(nh, P=3, policy_stride=-4096) == -22
        assert _call(nh, P=1 << 16, E=1 << 15, policy_stride=4096) == -22                          # P * E = 2^31
        assert _call(nh, P=46341, E=46341, policy_stride=4096) == -22                              # just above INT32_MAX
        for H in (0, 2, 62, 260, 512, -64):
            assert _call(nh, H=H) == -22, f"H = {H}"
        # the env kinds: Pendulum, MountainCar, LunarLander and what nobody has
        for kind in (PENDULUM, LUNARLANDER, MOUNTAINCAR, 4, -1):
            assert _call(nh, env_kind=kind) == -22
        assert _call(nh, env_kind=PENDULUM, D=3, A=1, cap=200) == -22 and _call(nh, env_kind=MOUNTAINCAR, D=2, A=3, cap=200) == -22
        assert _call(nh, D=3) == -22 and _call(nh, D=8) == -22 and _call(nh, A=1) == -22 and _call(nh, A=3) == -22 and _call(nh, A=4) == -22
    # the trunk's depth, and what belongs to a second layer only
    for nh in (0, 3, -1):
        assert _call(2, n_hidden=nh) == -22 and _call(1, n_hidden=nh) == -22
    assert _call(1, w1=FAKE) == -22 and _call(1, b1=FAKE) == -22 and _call(1, w1=FAKE, b1=FAKE) == -22
    assert _call(1, images=FAKE) == -22                                                            # one hidden layer has no fc2
    assert _call(2, P=3, policy_stride=4096, images=FAKE) == -22                                   # an image is of ONE policy
    assert _call(2, H=36, images=FAKE) == -22                                                      # an image needs H % 16 == 0
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_classic_duel_eval(ctypes.byref(_lib.ClassicEvalArgs()), None)                      # another struct's pointer


def _pairs(H=64, A=2, D=4):
    import torch
    lin = lambda n, k: (torch.zeros(n, k), torch.zeros(n))     # noqa: E731
    return [lin(H, D), lin(H, H)], lin(1, H), lin(A, H)


def test_ops_wrapper_refuses_wrong_shapes_and_cpu_tensors():
    import torch
    from gymrl_amd import ops
    trunk, value, adv = _pairs()
    kw = dict(n_episodes=4, seed=42, stream_id0=1 << 40, cap=500)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.classic_duel_eval(ops.CARTPOLE, trunk, value, adv, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.classic_duel_eval(ops.CARTPOLE, trunk[:1], value, adv, **kw)
    for bad_value, bad_adv in ((adv, adv), (_pairs(32)[1], adv), (value, _pairs(32)[2]), ((value[0], torch.zeros(2)), adv),
                               ((value[0].view(-1), value[1]), adv)):
        with pytest.raises(ValueError):                                                            # heads not H -> 1 / H -> A
            ops.classic_duel_eval(ops.CARTPOLE, trunk, bad_value, bad_adv, **kw)
    for bad_trunk in ([], trunk + trunk[1:], [trunk[0], _pairs(32)[0][1]], [trunk[0], trunk[0]], [(trunk[0][0],)]):
        with pytest.raises(ValueError):                                                            # a trunk of the wrong shape
            ops.classic_duel_eval(ops.CARTPOLE, bad_trunk, value, adv, **kw)
    # a population: params narrower than flat, no flat at all, tensors that are no views of flat
    flat = torch.zeros(64 * 5 + 64 * 65 + 65 + 2 * 65)
    with pytest.raises(ValueError, match="stack"):
        ops.classic_duel_eval(ops.CARTPOLE, trunk, value, adv, flat=flat, params=torch.zeros(2, 100), **kw)
    with pytest.raises(ValueError, match="stack"):
        ops.classic_duel_eval(ops.CARTPOLE, trunk, value, adv, params=torch.zeros(2, flat.numel()), **kw)
    with pytest.raises(ValueError, match="stack"):
        ops.classic_duel_eval(ops.CARTPOLE, trunk, value, adv, flat=flat, params=torch.zeros(flat.numel()), **kw)


def test_ops_wrapper_refuses_tensors_that_are_no_views_of_flat():
    import torch
    from gymrl_amd import ops
    trunk, value, adv = _pairs()
    n = 64 * 5 + 64 * 65 + 65 + 2 * 65
    kw = dict(n_episodes=4, seed=42, stream_id0=1 << 40, cap=500)
    with pytest.raises(ValueError, match="views"):                                                 # tensors of their own
        ops.classic_duel_eval(ops.CARTPOLE, trunk, value, adv, flat=torch.zeros(n), params=torch.zeros(2, n), **kw)
    # views of ONE buffer pass that check and reach the device pointer of the stack: a CPU stack is refused there
    flat, o = torch.zeros(n), 0
    views = []
    for w, b in trunk + [value, adv]:
        views.append((flat[o:o + w.numel()].view_as(w), flat[o + w.numel():o + w.numel() + b.numel()]))
        o += w.numel() + b.numel()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.classic_duel_eval(ops.CARTPOLE, views[:2], views[2], views[3], flat=flat, params=torch.zeros(2, n), **kw)
    with pytest.raises(ValueError, match="views"):                                                 # the advantage head lies outside
        ops.classic_duel_eval(ops.CARTPOLE, views[:2], views[2], adv, flat=flat, params=torch.zeros(2, n), **kw)
    with pytest.raises(ValueError, match="views"):                                                 # a buffer that ends in front of the heads
        ops.classic_duel_eval(ops.CARTPOLE, views[:2], views[2], views[3], flat=flat[:64 * 5 + 64 * 65], params=torch.zeros(2, n), **kw)


def test_the_three_new_configs_carry_the_switch_off():
    from gymrl_amd import ddqn_per_duel_cartpole, noisy_dqn_cartpole, rainbow_dqn_cartpole, sac_pendulum
    for mod in (noisy_dqn_cartpole, rainbow_dqn_cartpole, sac_pendulum, ddqn_per_duel_cartpole):
        assert mod.Config().fused_eval is False, mod.__name__
