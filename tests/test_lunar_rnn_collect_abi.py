"""CPU-side checks of the one-launch recurrent LunarLander collection's boundary (csrc/collect_lunar_rnn.hip):
gymrl_lunar_mlprnn_collect declared directly behind gymrl_lunar_mlprnn_eval, exported and mirrored once, its argument struct
the size the library reports, and every size, pointer or table error refused with -22 before anything is launched (no GPU
here; the pointers are fakes that are never dereferenced)."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

FAKE = 256                                             # 16-byte aligned, never dereferenced: validation fails first
NAME, QUERY = "gymrl_lunar_mlprnn_collect", "gymrl_lunar_collect_args_bytes"
F64 = ("norm_stats", "reward_stats", "R")
W32 = ("act", "logp", "value", "rew", "ep_ret", "lengths")
U8 = ("done", "dw", "live")
SCALARS = ("lin_w", "lin_b", "w_ih", "b_ih", "w_hh", "b_hh", "actor_w1", "actor_b1", "actor_a", "actor_w2", "actor_b2",
           "critic_w1", "critic_b1", "critic_a", "critic_w2", "critic_b2")
ALIGNED16 = ("lin_w", "w_ih", "w_hh", "actor_w1", "critic_w1")          # + pscn_w[1..3]: the forward's 16-byte reads


def _args(**kw):
    from gymrl_amd import _lib
    a = _lib.LunarCollectArgs()
    a.N, a.cap, a.seed, a.env_id0, a.counter0, a.gamma = 4, 1000, 42, 0, 0, 0.995
    for name in F64 + W32 + U8 + ("states",):
        setattr(a, name, FAKE)
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


def _call(params=None, **kw):
    from gymrl_amd import _lib
    return _lib.lib().gymrl_lunar_mlprnn_collect(ctypes.byref(_args(**kw)), ctypes.byref(_params() if params is None else params),
                                                 None)


def test_symbol_is_exported_the_abi_version_stays_and_the_struct_has_the_library_s_size():
    from gymrl_amd import _lib
    L = _lib.lib()
    assert hasattr(L, NAME) and hasattr(L, QUERY)
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION                  # an addition only
    assert L.gymrl_lunar_collect_args_bytes() == ctypes.sizeof(_lib.LunarCollectArgs)
    assert L.gymrl_mlprnn_params_bytes() == ctypes.sizeof(_lib.MlprnnParams)


def test_header_declares_it_behind_the_recurrent_evaluation_and_the_binding_mirrors_it_once():
    from gymrl_amd import _lib
    functions, structs = _parse_header()
    mirrors = _mirrors()
    order = list(functions)
    assert NAME in functions and QUERY in functions
    assert order.index("gymrl_lunar_mlprnn_eval") == order.index("gymrl_lunar_mhc_eval") + 1
    assert order.index(NAME) == order.index("gymrl_lunar_mlprnn_eval") + 1
    assert order[-1] == "gymrl_mountaincar_rule_eval"
    ret, params = functions[NAME]
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 3
    for ct, htype in zip(argtypes, params):
        assert _agrees(ct, htype, mirrors), (ct, htype)
    assert argtypes[0]._type_ is _lib.LunarCollectArgs and argtypes[1]._type_ is _lib.MlprnnParams
    assert list(_lib.SIGNATURES).count(NAME) == 1
    names = list(_lib.SIGNATURES)
    assert names.index("gymrl_lunar_mlprnn_eval") == names.index("gymrl_lunar_mhc_eval") + 1
    assert names.index(NAME) == names.index("gymrl_lunar_mlprnn_eval") + 1  # the binding keeps the header's order
    assert names[-1] == "gymrl_mountaincar_rule_eval"
    fields = structs["gymrl_lunar_collect_args"]
    assert [f for f, _ in _lib.LunarCollectArgs._fields_] == [f for f, _ in fields]
    for (fname, ct), (_, htype) in zip(_lib.LunarCollectArgs._fields_, fields):
        assert _agrees(ct, htype, mirrors), fname


def test_refuses_null_arguments_and_sizes_outside_one_workgroup():
    from gymrl_amd import _lib
    fn = _lib.lib().gymrl_lunar_mlprnn_collect
    assert fn(None, ctypes.byref(_params()), None) == -22                  # NULL args
    assert fn(ctypes.byref(_args()), None, None) == -22                    # NULL policy
    for out in F64 + W32 + U8 + ("states",):
        assert _call(**{out: None}) == -22, f"NULL {out}"
    assert _call(N=0) == -22 and _call(N=-1) == -22 and _call(N=17) == -22 and _call(N=1 << 20) == -22
    assert _call(cap=0) == -22 and _call(cap=-1) == -22 and _call(cap=1001) == -22
    assert _call(env_id0=-1) == -22


def test_refuses_misaligned_pointers():
    for name in F64:
        assert _call(**{name: FAKE + 4}) == -22, name                       # float64: 8 bytes
    for bad in (FAKE + 4, FAKE + 8, FAKE + 12):
        assert _call(states=bad) == -22, bad                                # rows of 8 floats: 16 bytes
    for name in W32:
        assert _call(**{name: FAKE + 2}) == -22, name


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


def test_ops_wrapper_refuses_cpu_tensors():
    import torch
    from gymrl_amd import ops
    assert ops.LUNAR_COLLECT_MAX_ENVS == 16
    f64 = lambda n: torch.zeros(n, dtype=torch.float64)   # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lunar_mlprnn_collect(_params(), 4, 100, 42, 0, 0, f64(26), f64(5), f64(4), 0.995)
