"""CPU-side checks of the Acrobot-v1 boundary: env kind 5 in the size queries (4 stays nobody's), gymrl_acrobot_net_eval declared,
exported and mirrored, its argument struct the size the library reports, and every pointer, size or shape error of the stepper
and of the evaluator refused with -22 before anything is launched (no GPU here)."""
import ctypes
import re

import pytest

from test_abi import _agrees, _header_text, _mirrors, _parse_header

ACROBOT = 5
FAKE = 256                                             # never dereferenced: validation fails first
FIELDS = ["P", "E", "cap", "net", "n_hidden", "H", "w", "b", "head_w", "head_b", "value_w", "value_b", "policy_stride", "images",
          "seed", "stream_id0", "start", "returns", "lengths", "terminated", "final_obs"]
NETS = ((0, 2), (1, 1), (1, 2), (2, 1), (2, 2))        # (net, n_hidden) the entry point takes


def test_enum_dims_and_env_kinds():
    from gymrl_amd import _lib, ops
    L = _lib.lib()
    assert ops.ACROBOT == ACROBOT and ops.ENV_KINDS["Acrobot-v1"] == ACROBOT and ops.ACROBOT_MAX_STEPS == 500
    assert sorted(ops.ENV_KINDS.values()) == [0, 1, 2, 3, 5]
    assert re.search(r"GYMRL_ENV_ACROBOT\s*=\s*5\b", _header_text())
    assert (L.gymrl_env_obs_dim(5), L.gymrl_env_act_dim(5), L.gymrl_env_is_discrete(5), L.gymrl_env_max_steps(5)) == (6, 3, 1, 500)
    assert ops.env_dims(ops.ACROBOT) == (6, 3, True, 500)
    # seven SoA fields (five f64, two 32-bit), each padded to 256 bytes
    assert L.gymrl_env_state_bytes(5, 1) == 7 * 256
    assert L.gymrl_env_state_bytes(5, 65) == 5 * 768 + 2 * 512
    assert L.gymrl_env_state_bytes(5, 4096) == 4096 * (5 * 8 + 2 * 4)
    assert L.gymrl_env_state_bytes(5, 0) == 0 and L.gymrl_env_state_bytes(5, -3) == 0
    # 4 is left free and 6 is nobody's
    for kind in (4, 6, -1):
        assert L.gymrl_env_obs_dim(kind) == -22 and L.gymrl_env_act_dim(kind) == -22 and L.gymrl_env_is_discrete(kind) == -22
        assert L.gymrl_env_max_steps(kind) == -22 and L.gymrl_env_state_bytes(kind, 8) == 0
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION          # an addition
    define = re.search(r"^#define\s+GYMRL_ACROBOT_WRAP_TRIPS\s+(\d+)", _header_text(), flags=re.M)
    import acrobot_ref
    assert define and int(define.group(1)) == acrobot_ref.WRAP_TRIPS == 8


def test_stepper_entry_points_refuse_bad_arguments():
    from gymrl_amd import _lib
    L = _lib.lib()
    null, fake, k = None, FAKE, ACROBOT
    assert L.gymrl_env_step(k, null, 8, 42, 0, fake, fake, null, fake, fake, fake, null, null, null, null, null) == -22
    assert L.gymrl_env_step(k, fake, 8, 42, 0, null, fake, null, fake, fake, fake, null, null, null, null, null) == -22
    assert L.gymrl_env_step(k, fake, 8, 42, 0, fake, null, null, fake, fake, fake, null, null, null, null, null) == -22
    assert L.gymrl_env_step(k, fake, 8, 42, 0, fake, fake, null, null, fake, fake, null, null, null, null, null) == -22
    assert L.gymrl_env_step(k, fake, 8, 42, 0, fake, fake, null, fake, null, fake, null, null, null, null, null) == -22
    assert L.gymrl_env_step(k, fake, 8, 42, 0, fake, fake, null, fake, fake, null, null, null, null, null, null) == -22
    assert L.gymrl_env_step(k, fake, -1, 42, 0, fake, fake, null, fake, fake, fake, null, null, null, null, null) == -22
    assert L.gymrl_env_step(k, 260, 8, 42, 0, fake, fake, null, fake, fake, fake, null, null, null, null, null) == -22    # misaligned state
    assert L.gymrl_env_step(k, fake, 8, 42, 0, fake, 264, null, fake, fake, fake, null, null, null, null, null) == -22     # ... observations
    assert L.gymrl_env_step(k, fake, 8, 42, 0, fake, fake, 264, fake, fake, fake, null, null, null, null, null) == -22     # ... terminal ones
    assert L.gymrl_env_step(k, fake, 0, 42, 0, fake, fake, null, fake, fake, fake, null, null, null, null, null) == 0      # no envs
    assert L.gymrl_env_reset(k, null, 8, 42, 0, fake, null) == -22 and L.gymrl_env_reset(k, fake, 8, 42, 0, null, null) == -22
    assert L.gymrl_env_reset(k, 260, 8, 42, 0, fake, null) == -22 and L.gymrl_env_reset(k, fake, 8, 42, 0, 264, null) == -22
    assert L.gymrl_env_reset(k, fake, -1, 42, 0, fake, null) == -22 and L.gymrl_env_reset(k, fake, 0, 42, 0, fake, null) == 0
    assert L.gymrl_env_abandon(k, null, 8, 42, 0, 50, fake, null, null, null, null, null) == -22
    assert L.gymrl_env_abandon(k, fake, 8, 42, 0, 50, null, null, null, null, null, null) == -22
    assert L.gymrl_env_abandon(k, fake, 8, 42, 0, 0, fake, null, null, null, null, null) == -22           # cap
    assert L.gymrl_env_abandon(k, 260, 8, 42, 0, 50, fake, null, null, null, null, null) == -22
    assert L.gymrl_env_abandon(k, fake, 0, 42, 0, 50, fake, null, null, null, null, null) == 0
    assert L.gymrl_env_refill(k, fake, 8, 42, 0, null) == 0 and L.gymrl_env_refill(k, null, 8, 42, 0, null) == -22
    # kind 4 keeps being refused everywhere, with arguments that kind 5 takes
    assert L.gymrl_env_step(4, fake, 8, 42, 0, fake, fake, null, fake, fake, fake, null, null, null, null, null) == -22
    assert L.gymrl_env_reset(4, fake, 8, 42, 0, fake, null) == -22 and L.gymrl_env_refill(4, fake, 8, 42, 0, null) == -22
    assert L.gymrl_env_abandon(4, fake, 8, 42, 0, 50, fake, null, null, null, null, null) == -22
    assert L.gymrl_env_abandon(4, fake, 0, 42, 0, 50, fake, null, null, null, null, null) == -22
    assert L.gymrl_env_step(6, fake, 8, 42, 0, fake, fake, null, fake, fake, fake, null, null, null, null, null) == -22


def test_learner_kernels_refuse_the_kind():
    """Config.fused_step stays CartPole's and Pendulum's: the fused acting kernels keep returning -22 for kind 5."""
    from gymrl_amd import _lib
    L = _lib.lib()
    for cls, fn in ((_lib.SacActArgs, L.gymrl_sac_act_step), (_lib.Td3ActArgs, L.gymrl_td3_act_step), (_lib.DsacActArgs, L.gymrl_dsac_act_step),
                    (_lib.DqnActArgs, L.gymrl_dqn_act_step), (_lib.DqnActArgs, L.gymrl_ddqn_duel_act_step),
                    (_lib.RainbowActArgs, L.gymrl_rainbow_act_step), (_lib.NdqnActArgs, L.gymrl_ndqn_act_step)):
        a = cls()
        a.N, a.D, a.A, a.H, a.env_kind = 8, 6, 3, 64, ACROBOT
        a.env_state = a.obs = a.obs_out = FAKE
        assert fn(ctypes.byref(a), None) == -22, fn.__name__


def _args(net_=0, nh_=2, **kw):
    from gymrl_amd import _lib
    a = _lib.AcrobotNetEvalArgs()
    a.P, a.E, a.cap, a.net, a.n_hidden, a.H = 1, 10, 500, net_, nh_, 64
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
    return _lib.lib().gymrl_acrobot_net_eval(ctypes.byref(_args(net_, nh_, **kw)), None)


def test_header_declares_and_binding_mirrors_the_entry_point():
    from gymrl_amd import _lib
    functions, structs = _parse_header()
    mirrors = _mirrors()
    L = _lib.lib()
    name, size = "gymrl_acrobot_net_eval", "gymrl_acrobot_net_eval_args_bytes"
    assert name in functions and size in functions and hasattr(L, name) and hasattr(L, size)
    ret, params = functions[name]
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 2
    for ct, htype in zip(argtypes, params):
        assert _agrees(ct, htype, mirrors)
    assert [f for f, _ in structs["gymrl_acrobot_net_eval_args"]] == [f for f, _ in _lib.AcrobotNetEvalArgs._fields_] == FIELDS
    assert structs["gymrl_acrobot_net_eval_args"] == structs["gymrl_mountaincar_net_eval_args"]      # one block, two entry points
    assert _lib.AcrobotNetEvalArgs._c_name_ == "gymrl_acrobot_net_eval_args"
    assert getattr(L, size)() == ctypes.sizeof(_lib.AcrobotNetEvalArgs) == ctypes.sizeof(_lib.MountainCarNetEvalArgs)
    # the header and the table keep one order, and the header still ends where it did
    names, table = list(functions), list(_lib.SIGNATURES)
    for order in (names, table):
        at = order.index(size)
        assert order[at + 1] == name
    assert names[-1] == "gymrl_mountaincar_rule_eval"


def test_shape_rule_of_the_binding():
    from gymrl_amd import ops
    ok = ops.acrobot_net_eval_shape_ok
    for net, nh in NETS:
        assert ok(net, nh, 6, 3, 64) and ok(net, nh, 6, 3, 256) and ok(net, nh, 6, 3, 8), (net, nh)
        assert not ok(net, nh, 6, 3, 260) and not ok(net, nh, 6, 3, 62) and not ok(net, nh, 6, 3, 0)
        assert not ok(net, nh, 2, 3, 64) and not ok(net, nh, 4, 2, 64) and not ok(net, nh, 6, 2, 64) and not ok(net, nh, 6, 4, 64)
        assert not ops.mountaincar_net_eval_shape_ok(net, nh, 6, 3, 64)
    assert not ok(0, 1, 6, 3, 64) and not ok(3, 2, 6, 3, 64) and not ok(-1, 2, 6, 3, 64) and not ok(1, 0, 6, 3, 64) and not ok(2, 3, 6, 3, 64)
    # the CartPole entry points keep refusing the kind
    assert not ops.classic_eval_shape_ok(ops.ACROBOT, 0, 6, 3, 64) and not ops.classic_duel_eval_shape_ok(ops.ACROBOT, 2, 6, 3, 64)


def test_eval_refuses_bad_arguments_before_any_launch():
    from gymrl_amd import _lib
    L = _lib.lib()
    assert L.gymrl_acrobot_net_eval(None, None) == -22                                             # NULL args
    for net, nh in NETS:
        c = lambda **kw: _call(net, nh, **kw)     # noqa: E731
        required = (["w0", "b0", "head_w", "head_b", "returns", "lengths", "terminated"] + (["w1", "b1"] if nh == 2 else []) +
                    (["value_w", "value_b"] if net else []))
        for req in required:
            assert c(**{req: None}) == -22, f"NULL {req}"
        assert c(P=0) == -22 and c(P=-1) == -22
        assert c(E=0) == -22 and c(E=-5) == -22
        assert c(cap=0) == -22 and c(cap=-1) == -22 and c(cap=501) == -22 and c(cap=1000) == -22      # Acrobot's TimeLimit
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
        L.gymrl_acrobot_net_eval(ctypes.byref(_lib.MountainCarNetEvalArgs()), None)                # another struct's pointer


def test_the_cartpole_entry_points_keep_refusing_the_kind():
    from gymrl_amd import _lib
    L = _lib.lib()
    a = _lib.ClassicEvalArgs()
    a.P, a.E, a.cap, a.env_kind, a.head, a.D, a.A, a.H = 1, 10, 500, ACROBOT, 0, 6, 3, 64
    for k in range(3):
        a.w[k] = a.b[k] = FAKE
    a.stream_id0, a.returns, a.lengths, a.terminated = 1 << 40, FAKE, FAKE, FAKE
    assert L.gymrl_classic_policy_eval(ctypes.byref(a), None) == -22
    d = _lib.ClassicDuelEvalArgs()
    d.P, d.E, d.cap, d.env_kind, d.n_hidden, d.D, d.A, d.H = 1, 10, 500, ACROBOT, 1, 6, 3, 64
    d.w[0] = d.b[0] = d.value_w = d.value_b = d.adv_w = d.adv_b = FAKE
    d.stream_id0, d.returns, d.lengths, d.terminated = 1 << 40, FAKE, FAKE, FAKE
    assert L.gymrl_classic_duel_eval(ctypes.byref(d), None) == -22


def _pairs(H=64, A=3, D=6):
    import torch
    lin = lambda n, k: (torch.zeros(n, k), torch.zeros(n))     # noqa: E731
    return [lin(H, D), lin(H, H)], lin(A, H), lin(1, H)


def test_ops_wrapper_refuses_wrong_shapes_and_cpu_tensors():
    import torch
    from gymrl_amd import ops
    trunk, head, value = _pairs()
    kw = dict(n_episodes=4, seed=42, stream_id0=1 << 40, cap=500)
    ev = ops.acrobot_net_eval
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
    for bad_trunk in ([], trunk + trunk[1:], [trunk[0], _pairs(32)[0][1]], [trunk[0], trunk[0]], [(trunk[0][0],)], _pairs(D=2)[0],
                      _pairs(D=4)[0]):
        with pytest.raises(ValueError):                                                            # a trunk of the wrong shape
            ev(1, bad_trunk, head, value=value, **kw)
    with pytest.raises(ValueError, match="Acrobot-v1 has 6 observations"):
        ev(0, _pairs(D=2)[0], head, **kw)                                                          # MountainCar's network
    with pytest.raises(ValueError, match="start"):                                                 # a start state has four fields
        ev(0, trunk, head, start=torch.zeros(1, 4, 2, dtype=torch.float64), **kw)
    with pytest.raises(ValueError):
        ev(0, trunk, head, kind=ops.MOUNTAINCAR, **kw)
    flat = torch.zeros(64 * 7 + 64 * 65 + 3 * 65)
    with pytest.raises(ValueError, match="stack"):
        ev(0, trunk, head, flat=flat, params=torch.zeros(2, 100), **kw)
    with pytest.raises(ValueError, match="views"):                                                 # tensors of their own
        ev(0, trunk, head, flat=flat, params=torch.zeros(2, flat.numel()), **kw)
    from gymrl_amd.envs import VecEnv
    with pytest.raises(ValueError, match="Acrobot-v1"):
        VecEnv("Acrobot-v0", 1, device="cpu")                                                      # the message lists what there is
