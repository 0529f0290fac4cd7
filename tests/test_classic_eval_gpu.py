"""Whole evaluation episodes in one launch (csrc/eval_classic.hip: gymrl_classic_policy_eval) against the loop they replace: a
VecEnv on the same streams stepped under the trainer's own select_action(deterministic=True) — gymrl_lin_fwd layer by layer, the
stand-alone pick, gymrl_env_step — first episode per env.  The kernel runs the same tiles and the same env core, so every
comparison is torch.equal / array_equal: returns, lengths, terminated flags, terminal observations."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED, ID0 = 1041, 1 << 40
E_MAX, E_CASES = 33, (1, 16, 17, 33)
DEV = "cuda:0"
# CartPole starts (x, x_dot, theta, theta_dot) for the hand-set controller: nine reset-like ones, then starts it cannot hold
_rng = np.random.RandomState(3)
STARTS17 = np.concatenate([_rng.uniform(-0.05, 0.05, (9, 4)),
                           [(2.39, 2.0, 0.0, 0.0), (0.0, 0.0, 0.2, 2.0), (0.0, 0.0, -0.2, -2.0), (1.5, 0.0, 0.05, 0.0),
                            (-2.0, -1.0, 0.0, 0.0), (0.0, 1.0, 0.1, 0.0), (0.0, 0.0, 0.0, 0.0), (2.0, 1.5, 0.0, 0.0)]])
CONTROLLERS = ((0.0, 0.0, 1.0, 1.0), (0.1, 0.3, 1.0, 0.5), (0.05, 0.2, 1.0, 0.3), (0.5, 1.0, 10.0, 2.0))


def _trainer(algo, hidden, seed=5, **more):
    import importlib
    mod = importlib.import_module("gymrl_amd." + algo)
    cfg = mod.Config()
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed, cfg.memory_capacity = 4, 16, hidden, seed, 4096
    cfg.max_episodes = 10 ** 9
    for k, v in more.items():
        setattr(cfg, k, v)
    cls = [v for k, v in vars(mod).items() if k.endswith("Trainer") and not k.startswith("_") and v.__module__ == mod.__name__]
    assert len(cls) == 1, cls
    return cls[0](cfg)


def _write_state(env, start):
    """start f64[n, 4 | 2] into the SoA state buffer of include/gymrl.h: f64 fields of [n], each padded to 256 bytes."""
    n, pitch = env.n, (env.n * 8 + 255) & ~255
    for k in range(start.shape[1]):
        env.state[k * pitch:k * pitch + n * 8].view(torch.float64).copy_(torch.from_numpy(np.ascontiguousarray(start[:, k])).to(DEV))


def _loop(tr, E, cap, seed=SEED, id0=ID0, start=None):
    """The step loop: -> (returns f32, lengths i32, terminated u8, final_obs f32) of the first episode of envs id0 .. id0 + E - 1,
    cut at `cap` steps.  An env's episode does not depend on the vector it is stepped in: E envs are the first E of more."""
    from gymrl_amd.envs import VecEnv
    env = VecEnv(tr.cfg.env_name, E, device=DEV, seed=seed, env_id0=id0)
    cart = env.discrete
    obs = env.reset()
    if start is not None:
        assert cart
        _write_state(env, start)
        obs = torch.from_numpy(start.astype(np.float32)).to(DEV)
    nxt, tobs = torch.empty_like(obs), torch.empty_like(obs)
    rew, ep_ret = torch.empty(E, device=DEV), torch.zeros(E, device=DEV)
    done, termf = torch.zeros(E, dtype=torch.uint8, device=DEV), torch.zeros(E, dtype=torch.uint8, device=DEV)
    ret = torch.full((E,), float("nan"), device=DEV)
    length = torch.zeros(E, dtype=torch.int32, device=DEV)
    term = torch.zeros(E, dtype=torch.uint8, device=DEV)
    fin = torch.zeros_like(obs)
    live = torch.ones(E, dtype=torch.bool, device=DEV)
    for t in range(cap):
        act = tr.select_action(obs, deterministic=True)
        env.step(act.contiguous(), nxt, rew, done_out=done, term_obs_out=tobs, ep_ret_out=ep_ret, terminated_out=termf)
        d = done.bool() & live
        last = d if t < cap - 1 else live
        fin = torch.where(last[:, None], tobs, fin)
        term = torch.where(last, termf * d.to(torch.uint8), term)
        ret = torch.where(d, ep_ret, ret)
        length = torch.where(live, torch.full_like(length, t + 1), length)
        live = live & ~d
        obs, nxt = nxt, obs
        if t % 16 == 15 and not bool(live.any()):
            break
    if cart:                                   # an episode cut below the TimeLimit: a reward of 1 per step so far
        ret = torch.where(torch.isnan(ret), length.float(), ret)
    assert not bool(torch.isnan(ret).any())
    return ret, length, term, fin


def _launch(tr, E, cap, seed=SEED, id0=ID0, **kw):
    from gymrl_amd import ops
    call = tr._eval_call()
    assert call is not None
    call = dict(call, cap=cap, **kw)
    return ops.classic_policy_eval(n_episodes=E, seed=seed, stream_id0=id0, want_final_obs=True, **call)


def _same(got, want, E, what=""):
    for name, g, w in zip(("returns", "lengths", "terminated", "final_obs"), got, want):
        assert g.shape[0] == 1 and torch.equal(g[0], w[:E]), (what, name, g[0], w[:E])


_REFS = {}


def _ref(algo, hidden):
    """One trainer and its loop over E_MAX envs per (algorithm, width), computed once and shared (never modified)."""
    if (algo, hidden) not in _REFS:
        tr = _trainer(algo, hidden)
        cap = 500 if algo == "dqn_cartpole" else 200
        _REFS[algo, hidden] = (tr, cap, _loop(tr, E_MAX, cap))
    return _REFS[algo, hidden]


# hidden 36: no image, not a multiple of 16; 64: with and without the forward image of fc2; 256: the instances built for that width
@pytest.mark.parametrize("algo", ["dqn_cartpole", "td3_pendulum"])
@pytest.mark.parametrize("hidden", [36, 64, 256])
def test_kernel_equals_loop(algo, hidden):
    from gymrl_amd import ops
    tr, cap, want = _ref(algo, hidden)
    fc2 = tr._eval_policy()[0][1]
    variants = [None] + ([ops.lin_fwd_image(fc2.weight)] if hidden % 16 == 0 else [])
    for E in E_CASES:
        for img in variants:
            got = _launch(tr, E, cap, images=img)
            _same(got, want, E, (E, img is not None))
    lengths = want[1].cpu().numpy()
    if algo == "dqn_cartpole":
        assert len(set(lengths[:16].tolist())) >= 2            # one workgroup holds episodes of different lengths
        assert lengths.max() < 500 and want[2].cpu().numpy().all()
    else:
        assert (lengths == 200).all() and not want[2].cpu().numpy().any()      # Pendulum never terminates: the TimeLimit
        assert float(want[0].max()) < 0.0


def test_two_launches_give_the_same_bits():
    for algo in ("dqn_cartpole", "td3_pendulum"):
        tr, cap, _ = _ref(algo, 64)
        a, b = _launch(tr, 33, cap), _launch(tr, 33, cap)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.parametrize("cap", [7, 1])
def test_cap_cuts_the_episodes(cap):
    tr, _, full = _ref("dqn_cartpole", 64)
    want = _loop(tr, 17, cap)
    got = _launch(tr, 17, cap)
    _same(got, want, 17, cap)
    lengths = got[1][0].cpu().numpy()
    assert (lengths == np.minimum(full[1][:17].cpu().numpy(), cap)).all() and (got[0][0].cpu().numpy() == lengths).all()
    assert (got[2][0].cpu().numpy() == ((full[1][:17].cpu().numpy() <= cap) & (full[2][:17].cpu().numpy() == 1))).all()


def _set_controller(tr, k):
    """A linear controller `push right iff k . obs > 0` as a DQN network, through the ReLU pair relu(s), relu(-s):
    fc1 rows 0 / 1 = +k / -k, fc2 passes both on, Q0 = relu(-s), Q1 = relu(s)."""
    fc1, fc2, fc3 = tr._eval_policy()[0]
    with torch.no_grad():
        for layer in (fc1, fc2, fc3):
            layer.weight.zero_()
            layer.bias.zero_()
        kt = torch.tensor(k, dtype=torch.float32, device=DEV)
        fc1.weight[0], fc1.weight[1] = kt, -kt
        fc2.weight[0, 0] = fc2.weight[1, 1] = 1.0
        fc3.weight[0, 1] = fc3.weight[1, 0] = 1.0


def _oracle_lengths(orc, k, starts):
    env = orc.Env(orc.CARTPOLE, len(starts), seed=1, env_id0=0)
    env.reset()
    env.set_classic_state(starts)
    obs, live = starts.astype(np.float32), np.ones(len(starts), bool)
    lengths, term = np.zeros(len(starts), int), np.zeros(len(starts), int)
    for t in range(500):
        r = env.step((obs @ np.asarray(k, np.float32) > 0).astype(np.int32))
        d = r["done"].astype(bool) & live
        lengths[live], term[d] = t + 1, r["terminated"][d]
        live &= ~d
        obs = r["obs"]
    return lengths, term


def test_hand_set_controller_reaches_the_time_limit_and_fails_elsewhere(oracle):
    # the coefficients: the first candidate that, on the CPU oracle's CartPole, holds some of the 17 starts for 500 steps and loses others
    picked = None
    for k in CONTROLLERS:
        lengths, term = _oracle_lengths(oracle, k, STARTS17)
        if ((lengths == 500) & (term == 0)).any() and ((lengths < 500) & (term == 1)).any():
            picked = k
            break
    assert picked is not None
    tr = _trainer("dqn_cartpole", 8)
    _set_controller(tr, picked)
    start = torch.from_numpy(STARTS17).to(DEV).view(1, 17, 4)
    got = _launch(tr, 17, 500, start=start)
    ret, lengths, term = (x[0].cpu().numpy() for x in got[:3])
    assert ((lengths == 500) & (term == 0)).any()              # the TimeLimit, not a termination
    assert ((lengths < 500) & (term == 1)).any()
    assert (ret == lengths).all()
    _same(got, _loop(tr, 17, 500, start=STARTS17), 17)


def test_start_overrides():
    tr = _trainer("dqn_cartpole", 64)
    # past the track's end after one step, whatever the action
    start = np.array([[2.39, 2.0, 0.0, 0.0]])
    got = _launch(tr, 1, 500, start=torch.from_numpy(start).to(DEV).view(1, 1, 4))
    assert got[0].item() == 1.0 and got[1].item() == 1 and got[2].item() == 1
    _same(got, _loop(tr, 1, 500, start=start), 1)
    # from the origin under a zeroed last layer: equal Q values, the first maximum is action 0 throughout
    fc3 = tr._eval_policy()[0][2]
    with torch.no_grad():
        fc3.weight.zero_()
        fc3.bias.zero_()
    start = np.zeros((1, 4))
    got = _launch(tr, 1, 500, start=torch.from_numpy(start).to(DEV).view(1, 1, 4))
    want = _loop(tr, 1, 500, start=start)
    _same(got, want, 1)
    assert got[2].item() == 1 and 1 < got[1].item() < 30 and got[3][0, 0, 0].item() < 0.0      # pushed left until the pole fell


def test_a_population_equals_its_members_and_the_loop():
    from gymrl_amd import ops
    trs = [_trainer("dqn_cartpole", 64, seed=s) for s in (1, 2, 3)]
    params = torch.stack([t.flat_params for t in trs])
    tr, call = trs[0], trs[0]._eval_call()
    kw = dict(n_episodes=17, seed=SEED, stream_id0=ID0, want_final_obs=True)
    tight = ops.classic_policy_eval(params=params, **kw, **call)
    padded = torch.full((3, params.shape[1] + 68), float("nan"), device=DEV)
    padded[:, :params.shape[1]] = params
    loose = ops.classic_policy_eval(params=padded, **kw, **call)
    ragged = ops.classic_policy_eval(params=padded[:, :params.shape[1] + 3].contiguous(), **kw, **call)      # padded by the binding
    for a, b, c in zip(tight, loose, ragged):
        assert a.shape[0] == 3 and torch.equal(a, b) and torch.equal(a, c)
    for p, t in enumerate(trs):
        one = _launch(t, 17, 500)
        want = _loop(t, 17, 500)
        for a, b, w in zip(tight, one, want):
            assert torch.equal(a[p], b[0]) and torch.equal(a[p], w)
    assert not torch.equal(tight[1][0], tight[1][1])           # three different policies on the same starts
    # the trainer's surface: numpy [P, E] on eval()'s streams
    r, n, f = tr.evaluate(17, params=params)
    assert r.shape == n.shape == f.shape == (3, 17) and r.dtype == np.float32 and n.dtype == np.int32 and f.dtype == np.uint8
    own = tr.evaluate(17)
    assert np.array_equal(own[0][0], r[0]) and np.array_equal(own[1][0], n[0])
    shifted = tr.evaluate(16, stream_offset=1)
    assert np.array_equal(shifted[1][0], own[1][0, 1:])


TRAINERS = ["dqn_cartpole", "ddqn_per_cartpole", "sac_cartpole", "td3_pendulum", "ddpg_pendulum"]


def _count_launches(monkeypatch):
    from gymrl_amd import ops
    calls, real = [], ops.classic_policy_eval
    monkeypatch.setattr(ops, "classic_policy_eval", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("algo", TRAINERS)
def test_trainer_eval_is_the_same_list(algo, monkeypatch):
    tr = _trainer(algo, 64)
    tr.train(max_vector_steps=20)
    assert len(tr.memory) == 80
    calls = _count_launches(monkeypatch)
    before = (tr._act_counter, tr.memory.cursor, tr.memory.size, tr.env.state.clone(), [t.clone() for t in tr.memory.ring])
    for n in (10, 5):
        tr.cfg.fused_eval = False
        want = tr.eval(n)
        assert not calls
        tr.cfg.fused_eval = True
        got = tr.eval(n)
        assert len(calls) == 1 and calls.pop()
        assert len(got) == n and got == want, (got, want)
    assert (tr._act_counter, tr.memory.cursor, tr.memory.size) == before[:3] and torch.equal(tr.env.state, before[3])
    for x, y in zip(tr.memory.ring, before[4]):
        assert torch.equal(x, y)
    assert tr.test() == tr.eval(5) and len(calls) == 2


@pytest.mark.parametrize("algo", TRAINERS)
def test_refused_shape_falls_back_to_the_loop(algo, monkeypatch):
    tr = _trainer(algo, 260)
    calls = _count_launches(monkeypatch)
    tr.cfg.fused_eval = False
    want = tr.eval(5)
    tr.cfg.fused_eval = True
    assert tr._eval_call() is None and tr.eval(5) == want and not calls
    with pytest.raises(RuntimeError):
        tr.evaluate(5)


def test_dueling_trainer_keeps_the_loop(monkeypatch):
    tr = _trainer("ddqn_per_duel_cartpole", 64, fused_eval=True)
    calls = _count_launches(monkeypatch)
    assert tr._eval_policy() is None and len(tr.eval(3)) == 3 and not calls
