"""CPU-side checks of the separable-NES boundary: gymrl_snes_perturb / gymrl_snes_tell declared, exported and mirrored, their
argument structs the size the library reports, every refusal of include/gymrl.h returned as -22 before anything is launched (no
GPU here), and the wrappers' and the learner's own refusals."""
import ctypes
import math

import pytest

from test_abi import _agrees, _mirrors, _parse_header

FAKE = 256                                             # never dereferenced: validation fails first
ENTRY = {"gymrl_snes_perturb": ("gymrl_snes_perturb_args", "SnesPerturbArgs",
                                ["n", "P", "stride", "seed", "generation", "mu", "sigma", "params"]),
         "gymrl_snes_tell": ("gymrl_snes_tell_args", "SnesTellArgs",
                             ["n", "P", "E", "eta_mu", "eta_sigma", "sigma_min", "sigma_max", "seed", "generation", "returns",
                              "returns64", "mu", "sigma", "weights"])}
SECTION = ["gymrl_snes_perturb_args_bytes", "gymrl_snes_tell_args_bytes", "gymrl_snes_perturb", "gymrl_snes_tell"]
BAD_P = (0, 1, -2, 3, 7, 8191, 8193, 8194, 1 << 20)
NOT_FINITE = (math.inf, -math.inf, math.nan)


def test_header_declares_and_binding_mirrors_the_entry_points():
    from gymrl_amd import _lib
    functions, structs = _parse_header()
    mirrors = _mirrors()
    L = _lib.lib()
    for name, (struct, cls_name, fields) in ENTRY.items():
        size = name + "_args_bytes"
        assert name in functions and size in functions and hasattr(L, name) and hasattr(L, size)
        _, params = functions[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params) == 2
        for ct, htype in zip(argtypes, params):
            assert _agrees(ct, htype, mirrors)
        cls = getattr(_lib, cls_name)
        assert [f for f, _ in structs[struct]] == [f for f, _ in cls._fields_] == fields
        assert cls._c_name_ == struct and getattr(L, size)() == ctypes.sizeof(cls)
        assert _lib.SIGNATURES[size] == (ctypes.c_size_t, [])
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION           # an addition
    # one section, the table in the header's order, not at the header's end
    names, table = list(functions), list(_lib.SIGNATURES)
    for order in (names, table):
        at = order.index(SECTION[0])
        assert order[at:at + 4] == SECTION
    assert names.index("gymrl_es_shape_grad") < names.index(SECTION[0]) < len(names) - 4
    assert names[-1] == "gymrl_mountaincar_rule_eval"


def _perturb(**kw):
    from gymrl_amd import _lib
    a = _lib.SnesPerturbArgs()
    a.n, a.P, a.stride, a.seed, a.generation, a.mu, a.sigma, a.params = 100, 6, 100, 42, 0, FAKE, FAKE, FAKE
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return _lib.lib().gymrl_snes_perturb(ctypes.byref(a), None)


def _tell(**kw):
    from gymrl_amd import _lib
    a = _lib.SnesTellArgs()
    a.n, a.P, a.E, a.eta_mu, a.eta_sigma, a.sigma_min, a.sigma_max, a.seed, a.generation = 100, 6, 2, 1.0, 0.1, 1e-5, 1.0, 42, 0
    a.returns, a.returns64, a.mu, a.sigma, a.weights = FAKE, None, FAKE, FAKE, FAKE
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return _lib.lib().gymrl_snes_tell(ctypes.byref(a), None)


def test_perturb_refuses_bad_arguments_before_any_launch():
    from gymrl_amd import _lib
    assert _lib.lib().gymrl_snes_perturb(None, None) == -22
    for name in ("mu", "sigma", "params"):
        assert _perturb(**{name: None}) == -22, name
        for addr in (260, 264, 258):                                 # float4 loads and stores: 16 bytes
            assert _perturb(**{name: addr}) == -22, (name, addr)
    assert _perturb(n=0, stride=0) == -22 and _perturb(n=-4) == -22
    for P in BAD_P:
        assert _perturb(P=P) == -22, P
    assert _perturb(stride=96) == -22                                # < n
    assert _perturb(stride=102) == -22 and _perturb(n=99, stride=99) == -22      # % 4
    assert _perturb(stride=-100) == -22


def test_tell_refuses_bad_arguments_before_any_launch():
    from gymrl_amd import _lib
    assert _lib.lib().gymrl_snes_tell(None, None) == -22
    for name in ("mu", "sigma", "weights"):
        assert _tell(**{name: None}) == -22, name
    for name in ("mu", "sigma"):
        for addr in (260, 264, 258):
            assert _tell(**{name: addr}) == -22, (name, addr)
    assert _tell(weights=258) == -22 and _tell(returns=258) == -22
    # exactly one of the two return pointers
    assert _tell(returns=None) == -22                                # neither
    assert _tell(returns64=FAKE) == -22                              # both
    assert _tell(returns=None, returns64=260) == -22                 # doubles: 8 bytes
    assert _tell(n=0) == -22 and _tell(n=-1) == -22
    assert _tell(E=0) == -22 and _tell(E=-3) == -22
    for P in BAD_P:
        assert _tell(P=P) == -22, P
    for v in NOT_FINITE:
        assert _tell(eta_mu=v) == -22 and _tell(eta_sigma=v) == -22, v
        assert _tell(sigma_min=v) == -22 and _tell(sigma_max=v) == -22, v
    assert _tell(sigma_min=0.0) == -22 and _tell(sigma_min=-1e-3) == -22
    assert _tell(sigma_min=2.0) == -22                               # above sigma_max = 1
    assert _tell(sigma_max=0.0) == -22
    with pytest.raises(ctypes.ArgumentError):
        _lib.lib().gymrl_snes_tell(ctypes.byref(_lib.SnesPerturbArgs()), None)             # another struct's pointer


def test_ops_refuse_wrong_dtypes_shapes_and_cpu_tensors():
    import torch
    from gymrl_amd import ops
    mu, sigma, stack, ret = torch.zeros(100), torch.ones(100), torch.zeros(6, 100), torch.zeros(6, 2)
    with pytest.raises(ValueError):
        ops.snes_tell(ret.to(torch.int64), mu, sigma, 42, 0, 1.0, 0.1, 1e-5, 1.0)
    with pytest.raises(ValueError):
        ops.snes_tell(ret.to(torch.float16), mu, sigma, 42, 0, 1.0, 0.1, 1e-5, 1.0)
    with pytest.raises(ValueError):
        ops.snes_tell(ret[0], mu, sigma, 42, 0, 1.0, 0.1, 1e-5, 1.0)                       # not [P, E]
    with pytest.raises(ValueError):
        ops.snes_tell(ret, mu, sigma[:99], 42, 0, 1.0, 0.1, 1e-5, 1.0)                     # sigma is not mu's shape
    with pytest.raises(ValueError):
        ops.snes_tell(ret, mu, sigma, 42, 0, 1.0, 0.1, 1e-5, 1.0, weights=torch.zeros(5))
    with pytest.raises(ValueError):
        ops.snes_perturb(mu, sigma[:99], 42, 0, stack)
    with pytest.raises(ValueError):
        ops.snes_perturb(stack, stack, 42, 0, stack)
    for dtype in (torch.float32, torch.float64):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.snes_tell(ret.to(dtype), mu, sigma, 42, 0, 1.0, 0.1, 1e-5, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.snes_perturb(mu, sigma, 42, 0, stack)


def test_the_learner_and_the_trainers_state_their_surface():
    import torch
    from gymrl_amd import es, es_cartpole, es_lunarlander
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        es.SeparableNES(torch.zeros(128), 0, 8, 0.1)                 # a CPU buffer
    for population in (7, 0, 8194):                                  # odd, empty, past the cap
        with pytest.raises(ValueError):
            es.SeparableNES(torch.zeros(128), 0, population, 0.1)
    with pytest.raises(ValueError):
        es.SeparableNES(torch.zeros(128, dtype=torch.float64), 0, 8, 0.1)
    for name in ("ask", "tell", "state_dict", "load_state_dict"):
        assert callable(getattr(es.SeparableNES, name))
    cfg = es_cartpole.Config()
    assert cfg.method == "openai" and cfg.eta_mu == 1.0 and cfg.eta_sigma is None
    cfg = es_lunarlander.Config()
    assert (cfg.env_name, cfg.method, cfg.hidden_dim) == ("LunarLander-v3", "snes", 64)
    assert (cfg.population, cfg.episodes_per_policy, cfg.sigma) == (256, 16, 0.1)
    assert es_lunarlander.ESTrainer.TRAIN_ENV_ID0 == 1 << 41 > es_lunarlander.ESTrainer.EVAL_ENV_ID0 == 1 << 40
    with pytest.raises(ValueError):
        es_cartpole.check_method({"method": "openai"}, "snes")
    with pytest.raises(ValueError):
        es_cartpole.check_method({}, "snes")                         # a checkpoint from before there was a choice
    es_cartpole.check_method({}, "openai")
