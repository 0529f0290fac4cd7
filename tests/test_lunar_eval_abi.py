"""CPU-side checks of the one-launch LunarLander evaluation's boundary (csrc/eval_lunar.hip): gymrl_lunar_policy_eval and
gymrl_lunar_mhc_eval declared in front of the MountainCar section, exported and mirrored, and every pointer, size or descriptor
error refused with -22 before anything is launched (no GPU here)."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

FAKE = 256                                             # never dereferenced: validation fails first
# PPO's ActorCritic at hidden 64: (out, in, act, src, dst)
STAGES = ((64, 8, 1, -1, 0), (64, 64, 1, 0, 1), (64, 64, 1, 1, 0), (64, 64, 1, 1, 2), (4, 64, 0, 0, -1), (1, 64, 0, 2, -1))


def _args(**kw):
    from gymrl_amd import _lib
    a = _lib.LunarEvalArgs()
    a.P, a.E, a.cap, a.seed, a.stream_id0, a.policy_stride = 1, 10, 1000, 42, 1 << 40, 0
    a.returns = a.lengths = a.terminated = FAKE
    a.terminal_obs = None
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def _desc(stages=STAGES, **first):
    from gymrl_amd import _lib
    d = _lib.MlpDesc()
    d.n_stages = len(stages)
    for e, (out_dim, in_dim, act, src, dst) in zip(d.stage, stages):
        e.W, e.b, e.out_dim, e.in_dim, e.act, e.src, e.dst = FAKE, FAKE, out_dim, in_dim, act, src, dst
    for k, v in first.items():
        assert hasattr(d.stage[0], k), k
        setattr(d.stage[0], k, v)
    return d


def _mhc(**kw):
    from gymrl_amd import _lib
    d = _lib.MhcPolicy()
    d.obs_dim, d.n_sub, d.n_act, d.sk_it = 8, 2, 4, 10
    d.in_w = d.in_b = d.final_norm_w = FAKE
    for s in range(2):
        for f in ("norm_w", "w", "alpha", "beta", "lin_w", "lin_b"):
            setattr(d.sub[s], f, FAKE)
    for h in range(2):
        for f in ("w1", "b1", "norm_w", "w2", "b2"):
            setattr(d.head[h], f, FAKE)
    for k, v in kw.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    return d


def _mlp(desc=None, **kw):
    from gymrl_amd import _lib
    return _lib.lib().gymrl_lunar_policy_eval(ctypes.byref(_args(**kw)), ctypes.byref(_desc() if desc is None else desc), None)


def _mhc_call(desc=None, **kw):
    from gymrl_amd import _lib
    return _lib.lib().gymrl_lunar_mhc_eval(ctypes.byref(_args(**kw)), ctypes.byref(_mhc() if desc is None else desc), None)


def test_args_size_and_abi_version():
    from gymrl_amd import _lib
    L = _lib.lib()
    assert L.gymrl_lunar_eval_args_bytes() == ctypes.sizeof(_lib.LunarEvalArgs)
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION                  # additions only


def test_header_declares_the_entry_points_in_front_of_mountaincar_and_the_binding_mirrors_them():
    from gymrl_amd import _lib
    functions, structs = _parse_header()
    mirrors = _mirrors()
    order = list(functions)
    assert order[-1] == "gymrl_mountaincar_rule_eval"
    for name, n_params in (("gymrl_lunar_eval_args_bytes", 0), ("gymrl_lunar_policy_eval", 3), ("gymrl_lunar_mhc_eval", 3)):
        assert name in functions and hasattr(_lib.lib(), name)
        assert order.index("gymrl_rollout_lunar_mhc") < order.index(name) < order.index("gymrl_mountaincar_rule_eval")
        ret, params = functions[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(params) == n_params
        for ct, htype in zip(argtypes, params):
            assert _agrees(ct, htype, mirrors)
        assert list(_lib.SIGNATURES).count(name) == 1
    assert _lib.SIGNATURES["gymrl_lunar_policy_eval"][0] is ctypes.c_int and _lib.SIGNATURES["gymrl_lunar_mhc_eval"][0] is ctypes.c_int
    assert [f for f, _ in structs["gymrl_lunar_eval_args"]] == [f for f, _ in _lib.LunarEvalArgs._fields_] == \
        ["P", "E", "cap", "seed", "stream_id0", "policy_stride", "returns", "lengths", "terminated", "terminal_obs"]


@pytest.mark.parametrize("call", [_mlp, _mhc_call], ids=["mlp", "mhc"])
def test_both_entry_points_refuse_bad_arguments_before_any_launch(call):
    from gymrl_amd import _lib
    L = _lib.lib()
    fn = L.gymrl_lunar_policy_eval if call is _mlp else L.gymrl_lunar_mhc_eval
    policy = _desc() if call is _mlp else _mhc()
    assert fn(None, ctypes.byref(policy), None) == -22                     # NULL args
    assert fn(ctypes.byref(_args()), None, None) == -22                    # NULL policy
    for out in ("returns", "lengths", "terminated"):
        assert call(**{out: None}) == -22, f"NULL {out}"
    assert call(E=0) == -22 and call(E=-3) == -22
    assert call(P=0) == -22 and call(P=-1) == -22
    assert call(cap=0) == -22 and call(cap=1001) == -22 and call(cap=-1) == -22
    assert call(policy_stride=6) == -22 and call(policy_stride=-4) == -22 and call(policy_stride=1001) == -22
    assert call(P=2, policy_stride=0) == -22                               # two policies in one place
    assert call(stream_id0=-1) == -22
    for name, bad in (("returns", 260), ("lengths", 258), ("terminal_obs", 264)):
        assert call(**{name: bad}) == -22, f"misaligned {name}"


def test_mlp_entry_refuses_what_the_rollout_refuses_in_a_descriptor():
    from gymrl_amd import _lib
    assert _mlp(P=1 << 16, E=1 << 15, policy_stride=4) == -22              # P * E = 2^31
    swap = lambda k, row: STAGES[:k] + (row,) + STAGES[k + 1:]             # noqa: E731
    d = _desc()
    d.n_stages = 0
    assert _mlp(d) == -22
    d.n_stages = 9
    assert _mlp(d) == -22
    assert _mlp(_desc(W=None)) == -22 and _mlp(_desc(W=260)) == -22        # missing / not 16-byte aligned
    assert _mlp(_desc(in_dim=4)) == -22 and _mlp(_desc(in_dim=0)) == -22   # the input layer reads 8 observations
    assert _mlp(_desc(out_dim=0)) == -22 and _mlp(_desc(out_dim=257)) == -22
    assert _mlp(_desc(act=3)) == -22 and _mlp(_desc(act=-1)) == -22
    assert _mlp(_desc(src=3)) == -22 and _mlp(_desc(src=-2)) == -22 and _mlp(_desc(dst=3)) == -22
    assert _mlp(_desc(swap(1, (64, 64, 1, 0, 0)))) == -22                  # a stage onto its own input
    assert _mlp(_desc(swap(1, (64, 257, 1, 0, 1)))) == -22                 # wider than the LDS buffers
    assert _mlp(_desc(swap(4, (2, 64, 0, 0, -1)))) == -22                  # the first head is not four logits
    assert _mlp(_desc(swap(5, (2, 64, 0, 2, -1)))) == -22                  # the second is not one value
    assert _mlp(_desc(STAGES[:5])) == -22                                  # one head
    assert _mlp(_desc(STAGES + ((1, 64, 0, 2, -1),))) == -22               # three heads
    with pytest.raises(ctypes.ArgumentError):
        _lib.lib().gymrl_lunar_policy_eval(ctypes.byref(_args()), ctypes.byref(_lib.MhcPolicy()), None)      # another struct's pointer
    # the same descriptors through the rollout's own gate
    r = _lib.RolloutLunarArgs()
    r.env_state = r.obs = r.act = r.logp = r.val = r.rew = r.done = r.next_value = FAKE
    r.n_envs, r.T, r.t0, r.nsteps = 16, 4, 0, 4
    for bad in (_desc(W=260), _desc(in_dim=4), _desc(swap(4, (2, 64, 0, 0, -1))), _desc(STAGES[:5])):
        assert _lib.lib().gymrl_rollout_lunar(ctypes.byref(r), ctypes.byref(bad), None) == -22


def test_mhc_entry_refuses_a_population_and_the_descriptors_the_rollout_refuses():
    assert _mhc_call(P=2, policy_stride=1024) == -22                       # one policy only
    assert _mhc_call(_mhc(obs_dim=4)) == -22 and _mhc_call(_mhc(n_act=2)) == -22       # not LunarLander's 8 / 4
    assert _mhc_call(_mhc(n_sub=9)) == -22 and _mhc_call(_mhc(sk_it=-1)) == -22
    assert _mhc_call(_mhc(in_w=None)) == -22 and _mhc_call(_mhc(final_norm_w=None)) == -22
    assert _mhc_call(_mhc(image=260)) == -22                               # the image is read 16 bytes at a time
    d = _mhc()
    d.sub[1].lin_w = None
    assert _mhc_call(d) == -22
    d = _mhc()
    d.head[0].w2 = None
    assert _mhc_call(d) == -22


def test_ops_wrappers_refuse_cpu_tensors_and_bad_stacks():
    import torch
    from gymrl_amd import ops
    from gymrl_amd.nn import FusedMLP
    from gymrl_amd.ppo_lunarlander import ActorCritic
    assert ops.LUNAR_MAX_STEPS == 1000
    net = ActorCritic(8, 4, 64)
    fused = net._act_net()
    assert isinstance(fused, FusedMLP)
    flat = torch.zeros(16)
    with pytest.raises(ValueError, match="stack"):
        ops.LunarPolicyStack(fused, flat, torch.zeros(2, 16))               # not on the device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lunar_mhc_eval(_mhc(), 4, 42, 1 << 40, device=torch.device("cpu"))
