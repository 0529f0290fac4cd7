"""CPU-side checks of the evolution-strategies boundary: gymrl_es_noise / gymrl_es_perturb / gymrl_es_shape_grad declared in
their slot, exported and mirrored, their argument structs the size the library reports, and every pointer, size or shape error
refused with -22 before anything is launched (no GPU here)."""
import ctypes
import math
import re

import pytest

from test_abi import _agrees, _header_text, _mirrors, _parse_header

FAKE = 256                                             # never dereferenced: validation fails first
ENTRY = {"gymrl_es_noise": ("gymrl_es_noise_args", "EsNoiseArgs", ["n", "k0", "K", "seed", "generation", "out"]),
         "gymrl_es_perturb": ("gymrl_es_perturb_args", "EsPerturbArgs",
                              ["n", "P", "stride", "sigma", "seed", "generation", "theta", "params"]),
         "gymrl_es_shape_grad": ("gymrl_es_shape_grad_args", "EsShapeGradArgs",
                                 ["n", "P", "E", "sigma", "seed", "generation", "returns", "grad", "weights"])}
SECTION = ["gymrl_es_pair_chunk", "gymrl_es_noise_args_bytes", "gymrl_es_perturb_args_bytes", "gymrl_es_shape_grad_args_bytes",
           "gymrl_es_noise", "gymrl_es_perturb", "gymrl_es_shape_grad"]


def test_header_declares_and_binding_mirrors_the_entry_points():
    from gymrl_amd import _lib, ops
    functions, structs = _parse_header()
    mirrors = _mirrors()
    L = _lib.lib()
    for name, (struct, cls_name, fields) in ENTRY.items():
        size = name + "_args_bytes"
        assert name in functions and size in functions and hasattr(L, name) and hasattr(L, size)
        ret, params = functions[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params) == 2
        for ct, htype in zip(argtypes, params):
            assert _agrees(ct, htype, mirrors)
        cls = getattr(_lib, cls_name)
        assert [f for f, _ in structs[struct]] == [f for f, _ in cls._fields_] == fields
        assert cls._c_name_ == struct and getattr(L, size)() == ctypes.sizeof(cls)
        assert _lib.SIGNATURES[size] == (ctypes.c_size_t, [])
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION           # an addition
    # a section of its own between the softmax rows and the tabular runs, the table in the header's order
    names, table = list(functions), list(_lib.SIGNATURES)
    for order in (names, table):
        at = order.index("gymrl_softmax_rows_bwd")
        assert order[at + 1:at + 9] == SECTION + ["gymrl_qlearn_state_bytes"]
    assert names[-1] == "gymrl_mountaincar_rule_eval"
    # the chunk of the gradient's sum: header, library and ops say the same
    define = re.search(r"^#define\s+GYMRL_ES_PAIR_CHUNK\s+(\d+)\s*$", _header_text(), flags=re.M)
    assert define and int(define.group(1)) == L.gymrl_es_pair_chunk() == ops.ES_PAIR_CHUNK
    assert ops.ES_MAX_POPULATION == 8192 and 4096 % ops.ES_PAIR_CHUNK == 0


def test_the_domain_tag_is_declared_and_the_old_ones_keep_their_values():
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, "gymrl_amd", "csrc", "gymrl_device.hpp")).read()
    tags = dict(re.findall(r"^\s*(RNG_\w+)\s*=\s*(0x[0-9A-Fa-f]+)u,", src, flags=re.M))
    assert {k: int(v, 16) for k, v in tags.items()} == {
        "RNG_ENV_RESET": 0x10000000, "RNG_ENV_STEP": 0x20000000, "RNG_POLICY": 0x30000000, "RNG_REPLAY": 0x40000000,
        "RNG_NOISE": 0x50000000, "RNG_SHUFFLE": 0x60000000, "RNG_ES": 0x70000000}


def _noise(**kw):
    from gymrl_amd import _lib
    a = _lib.EsNoiseArgs()
    a.n, a.k0, a.K, a.seed, a.generation, a.out = 100, 0, 4, 42, 0, FAKE
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return _lib.lib().gymrl_es_noise(ctypes.byref(a), None)


def _perturb(**kw):
    from gymrl_amd import _lib
    a = _lib.EsPerturbArgs()
    a.n, a.P, a.stride, a.sigma, a.seed, a.generation, a.theta, a.params = 100, 6, 100, 0.1, 42, 0, FAKE, FAKE
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return _lib.lib().gymrl_es_perturb(ctypes.byref(a), None)


def _shape_grad(**kw):
    from gymrl_amd import _lib
    a = _lib.EsShapeGradArgs()
    a.n, a.P, a.E, a.sigma, a.seed, a.generation, a.returns, a.grad, a.weights = 100, 6, 2, 0.1, 42, 0, FAKE, FAKE, FAKE
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return _lib.lib().gymrl_es_shape_grad(ctypes.byref(a), None)


BAD_SIGMA = (0.0, -0.1, math.inf, -math.inf, math.nan)
BAD_P = (0, 1, -2, 3, 7, 8191, 8193, 8194, 1 << 20)


def test_noise_refuses_bad_arguments_before_any_launch():
    from gymrl_amd import _lib
    assert _lib.lib().gymrl_es_noise(None, None) == -22
    assert _noise(out=None) == -22 and _noise(out=258) == -22
    assert _noise(n=0) == -22 and _noise(n=-5) == -22
    assert _noise(K=0) == -22 and _noise(K=-1) == -22 and _noise(K=4097) == -22
    assert _noise(k0=-1) == -22 and _noise(k0=4096) == -22 and _noise(k0=4093) == -22      # 4093 + 4 pairs: past 8192 / 2
    assert _noise(k0=(1 << 31) - 2) == -22                                                 # no wrap-around in k0 + K


def test_perturb_refuses_bad_arguments_before_any_launch():
    from gymrl_amd import _lib
    assert _lib.lib().gymrl_es_perturb(None, None) == -22
    assert _perturb(theta=None) == -22 and _perturb(params=None) == -22
    assert _perturb(theta=260) == -22 and _perturb(params=264) == -22                      # float4 rows
    assert _perturb(n=0, stride=0) == -22 and _perturb(n=-4) == -22
    for P in BAD_P:
        assert _perturb(P=P) == -22, P
    assert _perturb(stride=96) == -22                                                      # < n
    assert _perturb(stride=102) == -22 and _perturb(n=99, stride=99) == -22                # % 4
    assert _perturb(stride=-100) == -22
    for s in BAD_SIGMA:
        assert _perturb(sigma=s) == -22, s


def test_shape_grad_refuses_bad_arguments_before_any_launch():
    from gymrl_amd import _lib
    assert _lib.lib().gymrl_es_shape_grad(None, None) == -22
    for name in ("returns", "grad", "weights"):
        assert _shape_grad(**{name: None}) == -22, name
        assert _shape_grad(**{name: 258}) == -22, name
    assert _shape_grad(n=0) == -22 and _shape_grad(n=-1) == -22
    assert _shape_grad(E=0) == -22 and _shape_grad(E=-3) == -22
    for P in BAD_P:
        assert _shape_grad(P=P) == -22, P
    for s in BAD_SIGMA:
        assert _shape_grad(sigma=s) == -22, s
    with pytest.raises(ctypes.ArgumentError):
        _lib.lib().gymrl_es_shape_grad(ctypes.byref(_lib.EsPerturbArgs()), None)           # another struct's pointer


def test_ops_refuse_cpu_tensors_and_wrong_shapes():
    import torch
    from gymrl_amd import ops
    theta, stack, ret, grad = torch.zeros(100), torch.zeros(6, 100), torch.zeros(6, 2), torch.zeros(100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.es_noise(100, 0, 3, 42, 0, "cpu", out=torch.zeros(3, 100))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.es_perturb(theta, 0.1, 42, 0, stack)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.es_shape_grad(ret, 0.1, 42, 0, grad)
    with pytest.raises(ValueError):
        ops.es_noise(100, 0, 3, 42, 0, "cpu", out=torch.zeros(4, 100))
    with pytest.raises(ValueError):
        ops.es_perturb(stack, 0.1, 42, 0, stack)
    with pytest.raises(ValueError):
        ops.es_shape_grad(ret, 0.1, 42, 0, grad, weights=torch.zeros(5))
    assert [ops.es_stride(n) for n in (1, 4, 5, 4672, 70001)] == [4, 4, 8, 4672, 70004]


def test_the_learner_and_the_trainer_state_their_surface():
    from gymrl_amd import es, es_cartpole
    from gymrl_amd.policy_eval import PolicyEval
    cfg = es_cartpole.Config()
    assert cfg.fused_eval is True and cfg.env_name == "CartPole-v1"
    assert cfg.population % 2 == 0 and 2 <= cfg.population <= 8192 and cfg.sigma > 0 and cfg.lr > 0
    assert cfg.episodes_per_policy >= 1 and cfg.max_generations >= 1 and cfg.log_freq >= 1
    assert issubclass(es_cartpole.ESTrainer, PolicyEval)
    assert es_cartpole.ESTrainer.TRAIN_ENV_ID0 == 1 << 41 > PolicyEval.EVAL_ENV_ID0
    for name in ("ask", "tell", "state_dict", "load_state_dict"):
        assert callable(getattr(es.OpenAIES, name))
