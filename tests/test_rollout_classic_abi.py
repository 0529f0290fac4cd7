"""CPU-side checks of the boundary of PPO's one-launch kernels on the classic-control envs (csrc/rollout_classic.hip,
csrc/eval_classic_ppo.hip): gymrl_rollout_classic and gymrl_classic_ppo_eval are declared once in include/gymrl.h, exported and
mirrored in gymrl_amd/_lib.py, and every pointer, size, kind or descriptor error is refused with -22 before anything is launched
(fake aligned pointers, no GPU here).  gymrl_rollout_cartpole keeps its refusals."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

FAKE = 256                                             # never dereferenced: validation fails first
CARTPOLE, MOUNTAINCAR, ACROBOT = 0, 3, 5
DIMS = {CARTPOLE: (4, 2), MOUNTAINCAR: (2, 3), ACROBOT: (6, 3)}            # kind -> (observations, actions)
CAPS = {CARTPOLE: 500, MOUNTAINCAR: 200, ACROBOT: 500}                     # kind -> TimeLimit
OTHER_KINDS = (1, 2, 4, 6, -1)                                             # Pendulum, LunarLander, the free slot, past the end, junk
KINDS = pytest.mark.parametrize("kind", [CARTPOLE, MOUNTAINCAR, ACROBOT], ids=["cartpole", "mountaincar", "acrobot"])


def _stages(kind, hidden=64):
    """PPO's ActorCritic on the kind's (D, A): (out, in, act, src, dst)."""
    D, A = DIMS[kind]
    H = hidden
    return ((H, D, 1, -1, 0), (H, H, 1, 0, 1), (H, H, 1, 1, 0), (H, H, 1, 1, 2), (A, H, 0, 0, -1), (1, H, 0, 2, -1))


def _desc(stages, **first):
    from gymrl_amd import _lib
    d = _lib.MlpDesc()
    d.n_stages = len(stages)
    for e, (out_dim, in_dim, act, src, dst) in zip(d.stage, stages):
        e.W, e.b, e.out_dim, e.in_dim, e.act, e.src, e.dst = FAKE, FAKE, out_dim, in_dim, act, src, dst
    for k, v in first.items():
        assert hasattr(d.stage[0], k), k
        setattr(d.stage[0], k, v)
    return d


def _rollout_args(**kw):
    from gymrl_amd import _lib
    r = _lib.RolloutLunarArgs()
    r.env_state = r.obs = r.act = r.logp = r.val = r.rew = r.done = r.next_value = FAKE
    r.n_envs, r.T, r.t0, r.nsteps, r.gamma, r.lam = 16, 4, 0, 4, 0.99, 0.95
    for k, v in kw.items():
        assert hasattr(r, k), k
        setattr(r, k, v)
    return r


def _rollout(kind, desc=None, **kw):
    from gymrl_amd import _lib
    d = _desc(_stages(kind if kind in DIMS else CARTPOLE)) if desc is None else desc
    return _lib.lib().gymrl_rollout_classic(kind, ctypes.byref(_rollout_args(**kw)), ctypes.byref(d), None)


def _eval_args(kind, **kw):
    from gymrl_amd import _lib
    a = _lib.ClassicPpoEvalArgs()
    a.P, a.E, a.cap, a.env_kind, a.seed, a.stream_id0, a.policy_stride = 1, 10, CAPS.get(kind, 200), kind, 42, 1 << 40, 0
    a.returns = a.lengths = a.terminated = FAKE
    a.final_obs = None
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def _eval(kind, desc=None, **kw):
    from gymrl_amd import _lib
    d = _desc(_stages(kind if kind in DIMS else CARTPOLE)) if desc is None else desc
    return _lib.lib().gymrl_classic_ppo_eval(ctypes.byref(_eval_args(kind, **kw)), ctypes.byref(d), None)


def _bad_descriptors(kind):
    """Every descriptor gymrl_rollout_classic refuses for the kind, with what is wrong with it."""
    st = _stages(kind)
    D, A = DIMS[kind]
    swap = lambda k, row: st[:k] + (row,) + st[k + 1:]                      # noqa: E731
    none, nine = _desc(st), _desc(st)
    none.n_stages, nine.n_stages = 0, 9
    other = next(k for k in DIMS if DIMS[k][0] != D)
    yield "no stages", none
    yield "nine stages", nine
    yield "a missing weight", _desc(st, W=None)
    yield "a weight that is not 16-byte aligned", _desc(st, W=260)
    yield "another env's input width", _desc(st, in_dim=DIMS[other][0])
    yield "LunarLander's input width", _desc(st, in_dim=8)
    yield "no input", _desc(st, in_dim=0)
    yield "no output", _desc(st, out_dim=0)
    yield "an output wider than the LDS buffers", _desc(st, out_dim=257)
    yield "an unknown activation", _desc(st, act=3)
    yield "a negative activation", _desc(st, act=-1)
    yield "a source buffer past the third", _desc(st, src=3)
    yield "a source below the input", _desc(st, src=-2)
    yield "a destination past the third", _desc(st, dst=3)
    yield "a stage onto its own input", _desc(swap(1, (64, 64, 1, 0, 0)))
    yield "an input wider than the LDS buffers", _desc(swap(1, (64, 257, 1, 0, 1)))
    yield "another env's logit width", _desc(swap(4, (5 - A, 64, 0, 0, -1)))           # 2 <-> 3
    yield "LunarLander's logit width", _desc(swap(4, (4, 64, 0, 0, -1)))
    yield "a second head that is not one value", _desc(swap(5, (2, 64, 0, 2, -1)))
    yield "one head", _desc(st[:5])
    yield "three heads", _desc(st + ((1, 64, 0, 2, -1),))
    yield "another env's whole network", _desc(_stages(other))


def test_args_size_and_abi_version():
    from gymrl_amd import _lib
    L = _lib.lib()
    assert L.gymrl_classic_ppo_eval_args_bytes() == ctypes.sizeof(_lib.ClassicPpoEvalArgs)
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION                  # additions only


def test_header_declares_the_entry_points_and_the_binding_mirrors_them():
    from gymrl_amd import _lib
    functions, structs = _parse_header()
    mirrors = _mirrors()
    order, table = list(functions), list(_lib.SIGNATURES)
    assert order == table and order[-1] == "gymrl_mountaincar_rule_eval"   # one order, and the header still ends where it did
    for name, n_params in (("gymrl_rollout_classic", 4), ("gymrl_classic_ppo_eval_args_bytes", 0), ("gymrl_classic_ppo_eval", 3)):
        assert name in functions and hasattr(_lib.lib(), name)
        ret, params = functions[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(params) == n_params
        for ct, htype in zip(argtypes, params):
            assert _agrees(ct, htype, mirrors)
        assert table.count(name) == 1
    assert order.index("gymrl_rollout_classic") == order.index("gymrl_rollout_cartpole") + 1     # beside the entry it generalises
    assert order.index("gymrl_classic_ppo_eval") == order.index("gymrl_classic_ppo_eval_args_bytes") + 1
    assert _lib.SIGNATURES["gymrl_rollout_classic"] == (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_lib.RolloutLunarArgs),
                                                                       ctypes.POINTER(_lib.MlpDesc), ctypes.c_void_p])
    assert _lib.SIGNATURES["gymrl_rollout_cartpole"] == (ctypes.c_int, _lib.SIGNATURES["gymrl_rollout_classic"][1][1:])   # unchanged
    assert _lib.SIGNATURES["gymrl_classic_ppo_eval"][0] is ctypes.c_int
    assert _lib.SIGNATURES["gymrl_classic_ppo_eval_args_bytes"] == (ctypes.c_size_t, [])
    assert [f for f, _ in structs["gymrl_classic_ppo_eval_args"]] == [f for f, _ in _lib.ClassicPpoEvalArgs._fields_] == \
        ["P", "E", "cap", "env_kind", "seed", "stream_id0", "policy_stride", "returns", "lengths", "terminated", "final_obs"]


@KINDS
def test_rollout_refuses_what_the_cartpole_entry_refuses(kind):
    from gymrl_amd import _lib
    L = _lib.lib()
    d = _desc(_stages(kind))
    assert L.gymrl_rollout_classic(kind, None, ctypes.byref(d), None) == -22                      # NULL args
    assert L.gymrl_rollout_classic(kind, ctypes.byref(_rollout_args()), None, None) == -22        # NULL policy
    for slab in ("env_state", "obs", "act", "logp", "val", "rew", "done", "next_value"):
        assert _rollout(kind, **{slab: None}) == -22, f"NULL {slab}"
    assert _rollout(kind, n_envs=0) == -22 and _rollout(kind, n_envs=-16) == -22
    assert _rollout(kind, T=0) == -22 and _rollout(kind, T=-4) == -22
    assert _rollout(kind, t0=-1) == -22 and _rollout(kind, nsteps=-1) == -22
    assert _rollout(kind, t0=1, nsteps=4) == -22 and _rollout(kind, t0=5, nsteps=0) == -22        # past the slab's end
    assert _rollout(kind, gae_running=FAKE, gae_workspace=None) == -22                            # the running pair without its workspace
    for what, bad in _bad_descriptors(kind):
        assert _rollout(kind, bad) == -22, what
    # an empty window in front of the rollout's end is nothing to do: accepted, and still no launch
    assert _rollout(kind, t0=2, nsteps=0) == 0


@KINDS
def test_rollout_refuses_a_misaligned_observation_slab(kind):
    align = 16 if kind == CARTPOLE else 8
    for off in (4, 8, 12):
        assert (_rollout(kind, obs=FAKE + off, t0=2, nsteps=0) == -22) == (off % align != 0), (kind, off)
    assert _rollout(kind, obs=FAKE + 16, t0=2, nsteps=0) == 0


def test_rollout_refuses_every_other_kind():
    for kind in OTHER_KINDS:
        for like in DIMS:                                                   # whichever network comes with it
            assert _rollout(kind, _desc(_stages(like)), t0=2, nsteps=0) == -22, (kind, like)


def test_rollout_cartpole_keeps_its_refusals():
    from gymrl_amd import _lib
    L = _lib.lib()
    call = lambda d, **kw: L.gymrl_rollout_cartpole(ctypes.byref(_rollout_args(**kw)), ctypes.byref(d), None)      # noqa: E731
    good = _desc(_stages(CARTPOLE))
    assert call(good, t0=2, nsteps=0) == 0
    assert call(good, obs=None) == -22 and call(good, obs=FAKE + 8, t0=2, nsteps=0) == -22        # its rows are one float4
    assert call(good, t0=1, nsteps=4) == -22 and call(good, gae_running=FAKE) == -22
    for what, bad in _bad_descriptors(CARTPOLE):
        assert call(bad, t0=2, nsteps=0) == -22, what
    for kind in (MOUNTAINCAR, ACROBOT):                                     # the other envs' networks are not CartPole's
        assert call(_desc(_stages(kind)), t0=2, nsteps=0) == -22


@KINDS
def test_eval_refuses_bad_arguments_before_any_launch(kind):
    from gymrl_amd import _lib
    L = _lib.lib()
    d = _desc(_stages(kind))
    assert L.gymrl_classic_ppo_eval(None, ctypes.byref(d), None) == -22                           # NULL args
    assert L.gymrl_classic_ppo_eval(ctypes.byref(_eval_args(kind)), None, None) == -22            # NULL policy
    for out in ("returns", "lengths", "terminated"):
        assert _eval(kind, **{out: None}) == -22, f"NULL {out}"
    assert _eval(kind, E=0) == -22 and _eval(kind, E=-3) == -22
    assert _eval(kind, P=0) == -22 and _eval(kind, P=-1) == -22
    assert _eval(kind, P=1 << 16, E=1 << 15, policy_stride=4) == -22                              # P * E = 2^31
    assert _eval(kind, cap=0) == -22 and _eval(kind, cap=-1) == -22 and _eval(kind, cap=CAPS[kind] + 1) == -22
    assert _eval(kind, stream_id0=-1) == -22
    assert _eval(kind, policy_stride=6) == -22 and _eval(kind, policy_stride=-4) == -22 and _eval(kind, policy_stride=1001) == -22
    assert _eval(kind, P=2, policy_stride=0) == -22                                               # two policies in one place
    for name, bad in (("returns", 260), ("lengths", 258), ("final_obs", 260)):
        assert _eval(kind, **{name: bad}) == -22, f"misaligned {name}"
    for what, bad in _bad_descriptors(kind):
        assert _eval(kind, bad) == -22, what
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_classic_ppo_eval(ctypes.byref(_lib.LunarEvalArgs()), ctypes.byref(d), None)       # another struct's pointer


def test_eval_refuses_every_other_kind():
    for kind in OTHER_KINDS:
        for like in DIMS:
            assert _eval(kind, _desc(_stages(like))) == -22, (kind, like)
    assert _eval(MOUNTAINCAR, cap=201) == -22 and _eval(MOUNTAINCAR, cap=500) == -22              # MountainCar's TimeLimit is 200


def test_ops_wrappers_check_kinds_and_shapes_before_any_pointer():
    import torch
    from gymrl_amd import ops
    from gymrl_amd.ppo_lunarlander import ActorCritic
    assert ops.ROLLOUT_CLASSIC_DIMS == DIMS and ops.CLASSIC_PPO_EVAL_CAPS == CAPS
    N, T = 16, 4
    fused = ActorCritic(6, 3, 32)._act_net()

    def slabs(D):
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)          # noqa: E731  (CPU tensors: a pointer taken would raise RuntimeError)
        return [torch.zeros(4096, dtype=torch.uint8), N, 0, 0, 0, z(T + 1, N, D), z(T, N, dt=torch.int32), z(T, N), z(T, N), z(T, N),
                z(T, N, dt=torch.uint8), z(T, N), z(N), None, T, 0, T, 0.99, 0.95]
    with pytest.raises(ValueError, match="env kind 2"):
        ops.rollout_classic(ops.LUNARLANDER, *slabs(8))
    with pytest.raises(ValueError, match="env kind 1"):
        ops.rollout_classic(ops.PENDULUM, *slabs(3))
    with pytest.raises(ValueError, match="obs is f32"):
        ops.rollout_classic(ops.ACROBOT, *slabs(4))                         # CartPole's rows
    with pytest.raises(ValueError, match="obs is f32"):
        ops.rollout_cartpole(*slabs(6))                                     # the shared body: Acrobot's rows
    bad = slabs(2)
    bad[7] = torch.zeros(T, N + 1)
    with pytest.raises(ValueError, match="logp is"):
        ops.rollout_classic(ops.MOUNTAINCAR, *bad)
    with pytest.raises(ValueError, match="noise_exp is f32"):
        ops.rollout_classic(ops.MOUNTAINCAR, *slabs(2), noise_exp=torch.zeros(T, N, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rollout_classic(ops.ACROBOT, *slabs(6))                         # right shapes, CPU tensors
    with pytest.raises(ValueError, match="env kind 2"):
        ops.classic_ppo_eval(ops.LUNARLANDER, fused, 4, 42, 1 << 40, device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.classic_ppo_eval(ops.ACROBOT, fused, 4, 42, 1 << 40, device=torch.device("cpu"))
