"""CPU-side checks of the one-launch recurrent LunarLander evaluation's boundary (csrc/eval_lunar_rnn.hip):
gymrl_lunar_mlprnn_eval declared behind gymrl_lunar_mhc_eval, exported and mirrored once, and every pointer, size, stride or
table error refused with -22 before anything is launched (no GPU here; the pointers are fakes that are never dereferenced)."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

FAKE = 256                                             # 16-byte aligned, never dereferenced: validation fails first
NAME = "gymrl_lunar_mlprnn_eval"
ALIGNED16 = ("lin_w", "w_ih", "w_hh", "actor_w1", "critic_w1")          # + pscn_w[1..3]: gymrl_mlprnn_act's 16-byte reads
SCALARS = ("lin_w", "lin_b", "w_ih", "b_ih", "w_hh", "b_hh", "actor_w1", "actor_b1", "actor_a", "actor_w2", "actor_b2",
           "critic_w1", "critic_b1", "critic_a", "critic_w2", "critic_b2")


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


def _params(**kw):
    """A table of fake pointers; name=value sets a scalar member, name=(i, value) an array member's element."""
    from gymrl_amd import _lib
    p = _lib.MlprnnParams()
    for i in range(4):
        p.pscn_w[i] = p.pscn_b[i] = p.pscn_a[i] = FAKE
    for name in SCALARS:
        setattr(p, name, FAKE)
    for k, v in kw.items():
        assert hasattr(p, k), k
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def _call(params=None, norm_stats=None, norm_stride=0, h_final=None, **kw):
    from gymrl_amd import _lib
    return _lib.lib().gymrl_lunar_mlprnn_eval(ctypes.byref(_args(**kw)), ctypes.byref(_params() if params is None else params),
                                              norm_stats, norm_stride, h_final, None)


def test_symbol_is_exported_and_the_abi_version_stays():
    from gymrl_amd import _lib
    L = _lib.lib()
    assert hasattr(L, NAME)
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION                  # an addition only
    assert L.gymrl_mlprnn_params_bytes() == ctypes.sizeof(_lib.MlprnnParams) == 28 * ctypes.sizeof(ctypes.c_void_p)


def test_header_declares_it_behind_the_mhc_entry_and_the_binding_mirrors_it_once():
    from gymrl_amd import _lib
    functions, _ = _parse_header()
    mirrors = _mirrors()
    order = list(functions)
    assert NAME in functions
    assert order.index(NAME) == order.index("gymrl_lunar_mhc_eval") + 1
    assert order[-1] == "gymrl_mountaincar_rule_eval"
    ret, params = functions[NAME]
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 6
    for ct, htype in zip(argtypes, params):
        assert _agrees(ct, htype, mirrors), (ct, htype)
    assert argtypes[0]._type_ is _lib.LunarEvalArgs and argtypes[1]._type_ is _lib.MlprnnParams
    assert argtypes[3] is ctypes.c_int64
    assert list(_lib.SIGNATURES).count(NAME) == 1
    names = list(_lib.SIGNATURES)
    assert names.index(NAME) == names.index("gymrl_lunar_mhc_eval") + 1    # the binding keeps the header's order


def test_refuses_what_the_other_lunar_entries_refuse_in_the_args():
    from gymrl_amd import _lib
    fn = _lib.lib().gymrl_lunar_mlprnn_eval
    assert fn(None, ctypes.byref(_params()), None, 0, None, None) == -22   # NULL args
    assert fn(ctypes.byref(_args()), None, None, 0, None, None) == -22     # NULL policy
    for out in ("returns", "lengths", "terminated"):
        assert _call(**{out: None}) == -22, f"NULL {out}"
    assert _call(E=0) == -22 and _call(E=-3) == -22
    assert _call(P=0) == -22 and _call(P=-1) == -22
    assert _call(cap=0) == -22 and _call(cap=1001) == -22 and _call(cap=-1) == -22
    assert _call(policy_stride=6) == -22 and _call(policy_stride=-4) == -22 and _call(policy_stride=1001) == -22
    assert _call(P=2, policy_stride=0) == -22                              # two policies in one place
    assert _call(P=1 << 16, E=1 << 15, policy_stride=4) == -22             # P * E = 2^31
    assert _call(stream_id0=-1) == -22
    for name, bad in (("returns", 260), ("lengths", 258), ("terminal_obs", 264)):
        assert _call(**{name: bad}) == -22, f"misaligned {name}"


def test_refuses_a_null_member_and_a_misaligned_16_byte_weight():
    for i in range(4):
        for name in ("pscn_w", "pscn_b", "pscn_a"):
            assert _call(_params(**{name: (i, None)})) == -22, (name, i)
    for name in SCALARS:
        assert _call(_params(**{name: None})) == -22, name
    for name in ALIGNED16:
        assert _call(_params(**{name: FAKE + 4})) == -22 and _call(_params(**{name: FAKE + 8})) == -22, name
    for i in (1, 2, 3):
        assert _call(_params(pscn_w=(i, FAKE + 4))) == -22, i
    # the same tables through the acting step's own gate
    from gymrl_amd import _lib
    act = _lib.lib().gymrl_mlprnn_act
    for bad in (_params(w_hh=FAKE + 4), _params(pscn_w=(2, FAKE + 8)), _params(critic_b2=None)):
        assert act(FAKE, FAKE, ctypes.byref(bad), 16, 8, 4, None, None, 0, 0, 0, 1, FAKE, FAKE, FAKE, FAKE, None, None) == -22


def test_refuses_bad_norm_strides_and_misaligned_stats_or_hidden_state():
    assert _call(norm_stats=FAKE, norm_stride=-1) == -22 and _call(norm_stats=FAKE, norm_stride=-26) == -22
    for stride in (1, 8, 25):
        assert _call(norm_stats=FAKE, norm_stride=stride) == -22, stride
        assert _call(norm_stride=stride) == -22, stride                     # the stride is checked with or without stats
    assert _call(norm_stats=FAKE + 4, norm_stride=0) == -22                 # f64: 8 bytes
    assert _call(norm_stats=FAKE + 4, norm_stride=26) == -22
    for bad in (FAKE + 4, FAKE + 8, FAKE + 12):
        assert _call(h_final=bad) == -22, bad                               # float4 stores: 16 bytes


def test_ops_wrappers_refuse_cpu_tensors_and_bad_stacks():
    import torch
    from gymrl_amd import ops
    from gymrl_amd.ppg_rnn_lunarlander import ActorCriticPPG
    assert ops.LUNAR_NORM_STATS == 26
    net = ActorCriticPPG(8, 4)
    with pytest.raises(ValueError, match="stack"):
        ops.MlprnnPolicyStack(net, torch.zeros(16), torch.zeros(2, 16))     # not on the device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lunar_mlprnn_eval(_params(), 4, 42, 1 << 40, norm_stats=torch.zeros(26, dtype=torch.float64))
