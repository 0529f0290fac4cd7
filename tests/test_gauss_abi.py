"""The Gaussian-policy entry points without a GPU: declarations, exports, signatures, struct mirrors and sizes, and every refusal
(-EINVAL on fake pointers, before any launch); the ops wrappers' ValueError / RuntimeError; the discrete entry points keep
refusing Pendulum-v1."""
import ctypes
import os
import re

import pytest

torch = pytest.importorskip("torch")

from gymrl_amd import _lib, ops  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gymrl.h")
FAKE = 0x10000                   # aligned to everything asked for, never dereferenced on the host
NEW = ["gymrl_gaussian_sample", "gymrl_ppo_gauss_loss_workspace_bytes", "gymrl_ppo_gauss_loss_fwd_bwd", "gymrl_rollout_pendulum_args_bytes",
       "gymrl_rollout_pendulum", "gymrl_pendulum_ppo_eval_args_bytes", "gymrl_pendulum_ppo_eval"]


def _header():
    with open(HEADER) as f:
        return f.read()


def _struct_fields(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [re.sub(r"[\s\*]", "", n).split("[")[0] for n in re.sub(r"^.*?([\w\*]+(\s*,\s*\*?\w+)*)$", r"\1", decl).split(",")]
    return out


def test_declared_exported_and_typed():
    text, L = _header(), _lib.lib()
    assert L.gymrl_abi_version() == 4 and "#define GYMRL_ABI_VERSION 4" in text
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", text), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    order = [m.group(1) for m in re.finditer(r"^(?:int|size_t)\s+(gymrl_\w+)\(", text, flags=re.M)]
    assert order[-1] == "gymrl_mountaincar_rule_eval"
    at = {n: order.index(n) for n in order}
    assert at["gymrl_gaussian_sample"] == at["gymrl_categorical_sample"] + 1              # each beside its sibling
    assert at["gymrl_ppo_gauss_loss_workspace_bytes"] == at["gymrl_ppo_loss_fwd_bwd"] + 1
    assert at["gymrl_ppo_gauss_loss_fwd_bwd"] == at["gymrl_ppo_gauss_loss_workspace_bytes"] + 1
    assert at["gymrl_rollout_pendulum_args_bytes"] == at["gymrl_rollout_classic"] + 1
    assert at["gymrl_rollout_pendulum"] == at["gymrl_rollout_pendulum_args_bytes"] + 1
    assert at["gymrl_pendulum_ppo_eval_args_bytes"] == at["gymrl_classic_ppo_eval"] + 1
    assert at["gymrl_pendulum_ppo_eval"] == at["gymrl_pendulum_ppo_eval_args_bytes"] + 1
    sig = list(_lib.SIGNATURES)
    for name in NEW:                                                                         # the binding keeps the header's order
        assert sig[sig.index(name) - 1] == order[at[name] - 1], name
    assert len(_lib.SIGNATURES["gymrl_gaussian_sample"][1]) == 16 and len(_lib.SIGNATURES["gymrl_ppo_gauss_loss_fwd_bwd"][1]) == 20


def test_struct_mirrors_and_sizes():
    text, L = _header(), _lib.lib()
    for mirror, query in ((_lib.RolloutPendulumArgs, L.gymrl_rollout_pendulum_args_bytes), (_lib.PendulumPpoEvalArgs, L.gymrl_pendulum_ppo_eval_args_bytes)):
        assert [n for n, _ in mirror._fields_] == _struct_fields(text, mirror._c_name_), mirror._c_name_
        assert ctypes.sizeof(mirror) == query(), mirror._c_name_
    lunar = [n for n, _ in _lib.RolloutLunarArgs._fields_]
    mine = [n for n, _ in _lib.RolloutPendulumArgs._fields_]
    assert set(mine) - set(lunar) == {"log_std", "noise_normal", "reward_scale"}             # the lunar block plus what a Gaussian needs
    assert L.gymrl_ppo_gauss_loss_workspace_bytes(1, 1) == 8 and L.gymrl_ppo_gauss_loss_workspace_bytes(257, 3) == 2 * 3 * 8
    assert L.gymrl_ppo_gauss_loss_workspace_bytes(4099, 8) == 17 * 8 * 8
    assert L.gymrl_ppo_gauss_loss_workspace_bytes(10, 0) == 0 and L.gymrl_ppo_gauss_loss_workspace_bytes(10, 9) == 0


def test_sample_and_loss_refuse_bad_arguments():
    L, f, n = _lib.lib(), FAKE, None
    s = lambda mu=f, ls=f, v=f, N=8, A=1, act=f, lp=f, on=None: L.gymrl_gaussian_sample(mu, ls, v, n, 1, 2, 0, N, A, 0, act, lp, n, n, on, n)   # noqa: E731
    assert s(mu=n) == s(ls=n) == s(act=n) == s(lp=n) == s(N=-1) == s(A=0) == s(A=9) == -22
    assert s(N=0) == 0
    on = _lib.GaeOnline(f, f, f, f, f, 3, 8, 0.99, 0.95, 0.0, None)
    assert s(v=n, on=ctypes.byref(on)) == -22                                                # the composition needs the values
    for bad in (dict(rew_prev=None), dict(done_prev=None), dict(val_prev=None), dict(running=None), dict(gae_workspace=None),
                dict(t_prev=-1), dict(t_prev=8), dict(running2=f)):
        o = _lib.GaeOnline(f, f, f, f, f, 3, 8, 0.99, 0.95, 0.0, None)
        for k, v in bad.items():
            setattr(o, k, v)
        assert s(on=ctypes.byref(o)) == -22, bad
    cfg = _lib.PPOCfg(0.2, 3.0, 0.5, 0.01)

    def loss(B=8, A=1, grid=0, cfgp=ctypes.byref(cfg), **ptr):
        p = dict(mu=f, log_std=f, value=f, idx=n, act=f, logp_old=f, adv=f, ret=f, mom=n, dmu=f, dv=f, dls=f, met=n, ws=n, dws=f)
        p.update(ptr)
        return L.gymrl_ppo_gauss_loss_fwd_bwd(p["mu"], p["log_std"], p["value"], p["idx"], p["act"], p["logp_old"], p["adv"], p["ret"], p["mom"],
                                              B, A, cfgp, p["dmu"], p["dv"], p["dls"], p["met"], p["ws"], p["dws"], grid, n)
    for name in ("mu", "log_std", "value", "act", "logp_old", "adv", "ret", "dmu", "dv", "dls", "dws"):
        assert loss(**{name: n}) == -22, name
    assert loss(cfgp=None) == loss(B=-1) == loss(A=0) == loss(A=9) == loss(grid=-1) == -22
    assert loss(met=f) == -22                                                                # metrics_sum without its workspace
    assert loss(dws=f + 4) == -22 and loss(ws=f + 4, met=f) == -22                           # misaligned float64 tables
    assert loss(B=1000, grid=2, ws=f) == -22                                                 # a caller's partials table under a narrower grid
    assert loss(B=0) == 0


def _desc(n_in=3, n_act=1):
    d = _lib.MlpDesc()
    d.n_stages = 3
    for k, (i, o, src, dst, act) in enumerate(((n_in, 64, -1, 0, 1), (64, n_act, 0, -1, 0), (64, 1, 0, -1, 0))):
        e = d.stage[k]
        e.W, e.b, e.in_dim, e.out_dim, e.act, e.src, e.dst = FAKE, FAKE, i, o, act, src, dst
    return d


def _rollout(**kw):
    a = _lib.RolloutPendulumArgs()
    for name in ("env_state", "obs", "act", "logp", "val", "rew", "done", "next_value", "log_std"):
        setattr(a, name, FAKE)
    a.n_envs, a.T, a.t0, a.nsteps, a.reward_scale, a.gamma, a.lam = 8, 16, 0, 16, 0.1, 0.99, 0.95
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_rollout_refuses_bad_arguments():
    L = _lib.lib()
    run = lambda a, d=None: L.gymrl_rollout_pendulum(ctypes.byref(a) if a is not None else None, ctypes.byref(d or _desc()), None)   # noqa: E731
    assert run(None) == -22 and L.gymrl_rollout_pendulum(ctypes.byref(_rollout()), None, None) == -22
    for name in ("env_state", "obs", "act", "logp", "val", "rew", "done", "next_value", "log_std"):
        assert run(_rollout(**{name: None})) == -22, name
    assert run(_rollout(n_envs=0)) == run(_rollout(n_envs=-3)) == run(_rollout(T=0)) == -22
    assert run(_rollout(t0=-1)) == run(_rollout(nsteps=-1)) == run(_rollout(t0=8, nsteps=9)) == run(_rollout(t0=17, nsteps=0)) == -22
    assert run(_rollout(gae_running=FAKE)) == -22                                            # without its workspace
    assert run(_rollout(reward_scale=float("nan"))) == -22
    for name in ("obs", "act", "log_std", "noise_normal"):
        assert run(_rollout(**{name: FAKE + 2})) == -22, name                                # 4-byte alignment
    assert run(_rollout(), _desc(n_in=4)) == run(_rollout(), _desc(n_act=2)) == -22          # not a (3 -> 1, 1) network
    assert run(_rollout(t0=4, nsteps=0)) == 0                                                # nothing to do
    # the discrete entry points keep refusing the kind, and this one takes no other
    lunar = _lib.RolloutLunarArgs()
    for name in ("env_state", "obs", "act", "logp", "val", "rew", "done", "next_value"):
        setattr(lunar, name, FAKE)
    lunar.n_envs, lunar.T, lunar.t0, lunar.nsteps = 8, 16, 0, 16
    assert L.gymrl_rollout_classic(ops.PENDULUM, ctypes.byref(lunar), ctypes.byref(_desc()), None) == -22


def _eval(**kw):
    a = _lib.PendulumPpoEvalArgs()
    a.P, a.E, a.cap, a.seed, a.stream_id0, a.policy_stride = 1, 10, 200, 1, 0, 0
    a.returns, a.lengths, a.terminated = FAKE, FAKE, FAKE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_eval_refuses_bad_arguments():
    L = _lib.lib()
    run = lambda a, d=None: L.gymrl_pendulum_ppo_eval(ctypes.byref(a) if a is not None else None, ctypes.byref(d or _desc()), None)   # noqa: E731
    assert run(None) == -22 and L.gymrl_pendulum_ppo_eval(ctypes.byref(_eval()), None, None) == -22
    for name in ("returns", "lengths", "terminated"):
        assert run(_eval(**{name: None})) == -22, name
    assert run(_eval(P=0)) == run(_eval(E=0)) == run(_eval(cap=0)) == run(_eval(cap=201)) == run(_eval(stream_id0=-1)) == -22
    assert run(_eval(P=1 << 16, E=1 << 15, policy_stride=64)) == -22                         # P * E = 2^31
    assert run(_eval(P=2)) == run(_eval(policy_stride=-4)) == run(_eval(policy_stride=6)) == -22
    assert run(_eval(returns=FAKE + 4)) == run(_eval(lengths=FAKE + 2)) == run(_eval(final_obs=FAKE + 2)) == -22
    assert run(_eval(), _desc(n_in=4)) == run(_eval(), _desc(n_act=3)) == -22
    classic = _lib.ClassicPpoEvalArgs()
    classic.P, classic.E, classic.cap, classic.env_kind = 1, 10, 200, ops.PENDULUM
    classic.returns, classic.lengths, classic.terminated = FAKE, FAKE, FAKE
    assert L.gymrl_classic_ppo_eval(ctypes.byref(classic), ctypes.byref(_desc()), None) == -22


def test_ops_wrappers_refuse_wrong_shapes_and_cpu_tensors():
    z = torch.zeros
    assert ops.gaussian_sample_shape_ok(4, 1) and ops.gaussian_sample_shape_ok(0, 8) and not ops.gaussian_sample_shape_ok(4, 9)
    assert ops.ppo_gauss_loss_shape_ok(65, 3) and not ops.ppo_gauss_loss_shape_ok(65, 0)
    assert ops.rollout_pendulum_shape_ok(8, 16, 4, 12) and not ops.rollout_pendulum_shape_ok(8, 16, 4, 13) and not ops.rollout_pendulum_shape_ok(0, 16, 0, 1)
    assert ops.pendulum_ppo_eval_shape_ok(3, 10, 200) and not ops.pendulum_ppo_eval_shape_ok(3, 10, 201) and not ops.pendulum_ppo_eval_shape_ok(1 << 16, 1 << 15, 7)
    assert sorted(ops.ENV_KINDS.values()) == [0, 1, 2, 3, 5]
    with pytest.raises(ValueError):
        ops.gaussian_sample(z(4, 9), z(9))
    with pytest.raises(ValueError):
        ops.gaussian_sample(z(4, 2), z(3))
    with pytest.raises(ValueError):
        ops.gaussian_sample(z(4, 2), z(2), noise_normal=z(4, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gaussian_sample(z(4, 2), z(2))
    cfg = (0.2, 3.0, 0.5, 0.01)
    with pytest.raises(ValueError):
        ops.ppo_gauss_loss_fwd_bwd(z(4, 2), z(2), z(5), z(4, 2), z(4), z(4), z(4), cfg)
    with pytest.raises(ValueError):
        ops.ppo_gauss_loss_fwd_bwd(z(4, 2), z(2), z(4), z(3, 2), z(3), z(3), z(3), cfg)              # fewer stored rows than B, no idx
    with pytest.raises(ValueError):
        ops.ppo_gauss_loss_fwd_bwd(z(4, 2), z(2), z(4), z(4, 2), z(4), z(4), z(4), cfg, grid_blocks=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ppo_gauss_loss_fwd_bwd(z(4, 2), z(2), z(4), z(4, 2), z(4), z(4), z(4), cfg)
    T, N = 4, 8
    slab = lambda dt=torch.float32: z(T, N, dtype=dt)   # noqa: E731
    good = dict(env_state=z(4096, dtype=torch.uint8), n_envs=N, seed=1, env_id0=0, counter0=0, obs=z(T + 1, N, 3), act=slab(), logp=slab(),
                val=slab(), rew=slab(), done=slab(torch.uint8), ep_ret=None, next_value=z(N), policy_desc=_desc(), log_std=z(1), T=T, t0=0,
                nsteps=T, gamma=0.99, lam=0.95)
    for bad in (dict(obs=z(T + 1, N, 4)), dict(act=z(T, N, 1)), dict(log_std=z(2)), dict(noise_normal=z(T, N)), dict(nsteps=T + 1),
                dict(next_value=z(N + 1)), dict(gae_running=z(2, N, dtype=torch.float64))):
        with pytest.raises(ValueError):
            ops.rollout_pendulum(**dict(good, **bad))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rollout_pendulum(**good)
    with pytest.raises(ValueError):
        ops.rollout_classic(ops.PENDULUM, *[good[k] for k in ("env_state", "n_envs", "seed", "env_id0", "counter0", "obs", "act", "logp", "val", "rew",
                                                               "done", "ep_ret", "next_value", "policy_desc", "T", "t0", "nsteps", "gamma", "lam")])
    from gymrl_amd.ppo_pendulum import GaussianActorCritic
    net = GaussianActorCritic(3, 1, 64)._act_net()
    with pytest.raises(ValueError):
        ops.pendulum_ppo_eval(net, 10, 1, 0, cap=201)
    with pytest.raises(ValueError):
        ops.pendulum_ppo_eval(net, 0, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pendulum_ppo_eval(net, 10, 1, 0)


def test_trainer_module_surface():
    from gymrl_amd import ppo_lunarlander, ppo_pendulum
    cfg = ppo_pendulum.Config()
    assert cfg.env_name == "Pendulum-v1" and cfg.log_std_init == 0.0 and cfg.reward_scale == 0.1
    assert cfg.persistent_rollout is True and cfg.fused_eval is True
    assert issubclass(ppo_pendulum.PPOTrainer, ppo_lunarlander.PPOTrainer)
    m = ppo_pendulum.GaussianActorCritic(3, 1, 64, log_std_init=-0.5)
    assert "log_std" in m.state_dict() and float(m.log_std.detach()[0]) == -0.5 and m.actor[2].out_features == 1
    for name in ("train", "update", "save_checkpoint", "load_checkpoint", "compute_gae"):         # reused, not copied
        assert getattr(ppo_pendulum.PPOTrainer, name) is getattr(ppo_lunarlander.PPOTrainer, name)
