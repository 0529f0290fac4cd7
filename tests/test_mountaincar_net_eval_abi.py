"""CPU-side checks of the MountainCar-v0 policy-episode boundary: gymrl_mountaincar_net_eval declared in its slot, exported and
mirrored, its argument struct the size the library reports, and every pointer, size or shape error refused with -22 before
anything is launched (no GPU here)."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

FAKE = 256                                             # never dereferenced: validation fails first
FIELDS = ["P", "E", "cap", "net", "n_hidden", "H", "w", "b", "head_w", "head_b", "value_w", "value_b", "policy_stride", "images",
          "seed", "stream_id0", "start", "returns", "lengths", "terminated", "final_obs"]
NETS = ((0, 2), (1, 1), (1, 2), (2, 1), (2, 2))        # (net, n_hidden) the entry point takes


def _args(net_=0, nh_=2, **kw):
    from gymrl_amd import _lib
    a = _lib.MountainCarNetEvalArgs()
    a.P, a.E, a.cap, a.net, a.n_hidden, a.H = 1, 10, 200, net_, nh_, 64
    for k in range(2):
        a.w[k] = a.b[k] = FAKE if k < nh_ else None
    a.head_w = a.head_b = FAKE
    a.value_w = a.value_b = FAKE if net_ else None
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


def _call(net_=0, nh_=2, **kw):
    from gymrl_amd import _lib
    return _lib.lib().gymrl_mountaincar_net_eval(ctypes.byref(_args(net_, nh_, **kw)), None)


def test_header_declares_and_binding_mirrors_the_entry_point():
    from gymrl_amd import _lib
    functions, structs = _parse_header()
    mirrors = _mirrors()
    L = _lib.lib()
    name, size = "gymrl_mountaincar_net_eval", "gymrl_mountaincar_net_eval_args_bytes"
    assert name in functions and size in functions and hasattr(L, name) and hasattr(L, size)
    ret, params = functions[name]
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 2
    for ct, htype in zip(argtypes, params):
        assert _agrees(ct, htype, mirrors)
    assert [f for f, _ in structs["gymrl_mountaincar_net_eval_args"]] == [f for f, _ in _lib.MountainCarNetEvalArgs._fields_] == FIELDS
    assert _lib.MountainCarNetEvalArgs._c_name_ == "gymrl_mountaincar_net_eval_args"
    assert getattr(L, size)() == ctypes.sizeof(_lib.MountainCarNetEvalArgs)
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION          # an addition
    # a section of its own: directly behind gymrl_ndqn_update, in front of the classic-control episode entry points
    names = list(functions)
    at = names.index("gymrl_ndqn_update")
    assert names[at + 1:at + 4] == [size, name, "gymrl_classic_eval_args_bytes"]
    assert names[-1] == "gymrl_mountaincar_rule_eval"
    table = list(_lib.SIGNATURES)
    at = table.index("gymrl_ndqn_update")
    assert table[at + 1:at + 3] == [size, name]


def test_the_defaults_of_this_file_are_accepted_shapes():
    """Every refusal below changes ONE field of an argument block that passes every check (it is never sent as it is: its pointers
    are fakes): the ops-side shape test agrees with its defaults."""
    from gymrl_amd import ops
    ok = ops.mountaincar_net_eval_shape_ok
    for net, nh in NETS:
        assert ok(net, nh, 2, 3, 64) and ok(net, nh, 2, 3, 256) and ok(net, nh, 2, 3, 36), (net, nh)
        assert not ok(net, nh, 2, 3, 260) and not ok(net, nh, 2, 3, 62) and not ok(net, nh, 2, 3, 0)
        assert not ok(net, nh, 4, 2, 64) and not ok(net, nh, 2, 2, 64) and not ok(net, nh, 3, 3, 64) and not ok(net, nh, 2, 4, 64)
    assert not ok(0, 1, 2, 3, 64) and not ok(3, 2, 2, 3, 64) and not ok(-1, 2, 2, 3, 64)
    assert not ok(1, 0, 2, 3, 64) and not ok(2, 3, 2, 3, 64)
    assert (ops.MOUNTAINCAR_NET_MLP, ops.MOUNTAINCAR_NET_DUEL_MEAN, ops.MOUNTAINCAR_NET_DUEL_ROW) == (0, 1, 2)
    # the old entry points keep refusing the kind
    assert not ops.classic_eval_shape_ok(ops.MOUNTAINCAR, 0, 2, 3, 64) and not ops.classic_duel_eval_shape_ok(ops.MOUNTAINCAR, 2, 2, 3, 64)


def test_eval_refuses_bad_arguments_before_any_launch():
    from gymrl_amd import _lib
    L = _lib.lib()
    assert L.gymrl_mountaincar_net_eval(None, None) == -22                                         # NULL args
    for net, nh in NETS:
        c = lambda **kw: _call(net, nh, **kw)     # noqa: E731
        required = (["w0", "b0", "head_w", "head_b", "returns", "lengths", "terminated"] + (["w1", "b1"] if nh == 2 else []) +
                    (["value_w", "value_b"] if net else []))
        for req in required:
            assert c(**{req: None}) == -22, f"NULL {req}"
        assert c(P=0) == -22 and c(P=-1) == -22
        assert c(E=0) == -22 and c(E=-5) == -22
        assert c(cap=0) == -22 and c(cap=-1) == -22 and c(cap=201) == -22 and c(cap=500) == -22       # MountainCar's TimeLimit
        assert c(stream_id0=-1) == -22
        misaligned = ([("w0", 264), ("b0", 258), ("head_w", 260), ("head_b", 258), ("start", 260), ("returns", 258), ("lengths", 258),
                       ("final_obs", 258)] + ([("w1", 260), ("b1", 258), ("images", 264)] if nh == 2 else []) +
                      ([("value_w", 264), ("value_b", 257)] if net else []))
        for name, bad in misaligned:
            assert c(**{name: bad}) == -22, f"misaligned {name}"
        assert c(P=3) == -22                                                                      # stride 0 is ONE policy
        assert c(P=3, policy_stride=4098) == -22 and c(policy_stride=6) == -22                    # % 4
        assert c(P=3, policy_stride=-4096) == -22
        assert c(P=1 << 16, E=1 << 15, policy_stride=4096) == -22                                 # P * E = 2^31
        assert c(P=46341, E=46341, policy_stride=4096) == -22                                     # just above INT32_MAX
        for H in (0, 2, 62, 260, 512, -64):
            assert c(H=H) == -22, f"H = {H}"
        for bad in (3, -1, 7):
            assert c(net=bad) == -22
        for bad in (0, 3, -1):
            assert c(n_hidden=bad) == -22
        assert c(P=3, policy_stride=4096, images=FAKE) == -22                                     # an image is of ONE policy
        if nh == 2:
            assert c(H=36, images=FAKE) == -22                                                    # an image needs H % 16 == 0
    # the three-layer network: two hidden layers, no value head
    assert _call(0, 2, n_hidden=1) == -22 and _call(0, 1) == -22
    assert _call(0, 2, value_w=FAKE) == -22 and _call(0, 2, value_b=FAKE) == -22 and _call(0, 2, value_w=FAKE, value_b=FAKE) == -22
    # a dueling network: the value head is required
    for net in (1, 2):
        assert _call(net, 2, value_w=None) == -22 and _call(net, 1, value_b=None) == -22
        # what belongs to a second layer only
        assert _call(net, 1, w1=FAKE) == -22 and _call(net, 1, b1=FAKE) == -22 and _call(net, 1, w1=FAKE, b1=FAKE) == -22
        assert _call(net, 1, images=FAKE) == -22
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_mountaincar_net_eval(ctypes.byref(_lib.ClassicDuelEvalArgs()), None)               # another struct's pointer


def test_the_old_entry_points_keep_refusing_the_kind():
    from gymrl_amd import _lib
    L = _lib.lib()
    a = _lib.ClassicEvalArgs()
    a.P, a.E, a.cap, a.env_kind, a.head, a.D, a.A, a.H = 1, 10, 200, 3, 0, 2, 3, 64
    for k in range(3):
        a.w[k] = a.b[k] = FAKE
    a.stream_id0, a.returns, a.lengths, a.terminated = 1 << 40, FAKE, FAKE, FAKE
    assert L.gymrl_classic_policy_eval(ctypes.byref(a), None) == -22
    d = _lib.ClassicDuelEvalArgs()
    d.P, d.E, d.cap, d.env_kind, d.n_hidden, d.D, d.A, d.H = 1, 10, 200, 3, 1, 2, 3, 64
    d.w[0] = d.b[0] = d.value_w = d.value_b = d.adv_w = d.adv_b = FAKE
    d.stream_id0, d.returns, d.lengths, d.terminated = 1 << 40, FAKE, FAKE, FAKE
    assert L.gymrl_classic_duel_eval(ctypes.byref(d), None) == -22


def _pairs(H=64, A=3, D=2):
    import torch
    lin = lambda n, k: (torch.zeros(n, k), torch.zeros(n))     # noqa: E731
    return [lin(H, D), lin(H, H)], lin(A, H), lin(1, H)


def test_ops_wrapper_refuses_wrong_shapes_and_cpu_tensors():
    import torch
    from gymrl_amd import ops
    trunk, head, value = _pairs()
    kw = dict(n_episodes=4, seed=42, stream_id0=1 << 40, cap=200)
    ev = ops.mountaincar_net_eval
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev(0, trunk, head, **kw)
    for net in (1, 2):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ev(net, trunk, head, value=value, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ev(net, trunk[:1], head, value=value, **kw)
        with pytest.raises(ValueError):                                                            # a dueling network needs its value head
            ev(net, trunk, head, **kw)
        for bad_value in (head, _pairs(32)[2], (value[0], torch.zeros(2)), (value[0].view(-1), value[1])):
            with pytest.raises(ValueError):                                                        # the value head is not H -> 1
                ev(net, trunk, head, value=bad_value, **kw)
    with pytest.raises(ValueError):                                                                # three layers have no value head
        ev(0, trunk, head, value=value, **kw)
    with pytest.raises(ValueError):                                                                # and two hidden layers
        ev(0, trunk[:1], head, **kw)
    for bad_head in (_pairs(32)[1], _pairs(A=2)[1], (head[0], torch.zeros(2)), (head[0].view(-1), head[1])):
        with pytest.raises(ValueError):                                                            # the head is not H -> 3
            ev(0, trunk, bad_head, **kw)
    for bad_trunk in ([], trunk + trunk[1:], [trunk[0], _pairs(32)[0][1]], [trunk[0], trunk[0]], [(trunk[0][0],)], _pairs(D=4)[0]):
        with pytest.raises(ValueError):                                                            # a trunk of the wrong shape
            ev(1, bad_trunk, head, value=value, **kw)
    # a population: params narrower than flat, no flat at all, a single row
    flat = torch.zeros(64 * 3 + 64 * 65 + 3 * 65)
    with pytest.raises(ValueError, match="stack"):
        ev(0, trunk, head, flat=flat, params=torch.zeros(2, 100), **kw)
    with pytest.raises(ValueError, match="stack"):
        ev(0, trunk, head, params=torch.zeros(2, flat.numel()), **kw)
    with pytest.raises(ValueError, match="views"):                                                 # tensors of their own
        ev(0, trunk, head, flat=flat, params=torch.zeros(2, flat.numel()), **kw)


def test_the_six_configs_carry_the_switch_off_and_the_trainers_declare_their_combine():
    from gymrl_amd import (ddqn_per_cartpole, ddqn_per_duel_cartpole, dqn_cartpole, noisy_dqn_cartpole, rainbow_dqn_cartpole,
                           sac_cartpole)
    from gymrl_amd.policy_eval import PolicyEval
    for mod in (dqn_cartpole, ddqn_per_cartpole, sac_cartpole, rainbow_dqn_cartpole, ddqn_per_duel_cartpole, noisy_dqn_cartpole):
        assert mod.Config().fused_eval is False, mod.__name__
    assert PolicyEval.EVAL_DUEL_COMBINE == 1
    assert rainbow_dqn_cartpole.RainbowDQNTrainer.EVAL_DUEL_COMBINE == 2
    assert ddqn_per_duel_cartpole.DDQNPERDuelTrainer.EVAL_DUEL_COMBINE == 1
    assert noisy_dqn_cartpole.NoisyDQNTrainer.EVAL_DUEL_COMBINE == 1
