"""Whole evaluation episodes of Acrobot-v1 in one launch (csrc/eval_net.hip: gymrl_acrobot_net_eval) against the loop they
replace: a VecEnv("Acrobot-v1") on the same streams stepped under the trainer's own select_action(deterministic=True), first
episode per env.  Four trainers cover the networks: DQN (net 0), dueling DDQN+PER (net 1, one hidden layer), NoisyNet dueling DQN
(net 1, two) and Rainbow (net 2, two); net 2 on one hidden layer has no trainer and is checked against the two-layer launch with an
identity second layer.  The kernels run the layer path's tiles, the trainers' combines and the stepper's env core, so every
comparison is torch.equal / array_equal: returns, lengths, terminated flags, terminal observations.  Expected episodes of the
hand-set pump policy come from the plain-Python restatement tests/acrobot_ref.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import acrobot_ref as ref  # noqa: E402
from test_classic_eval_gpu import _trainer as _any_trainer, _write_state  # noqa: E402
from test_duel_eval_gpu import _untouched  # noqa: E402

SEED, ID0 = 42, 1 << 40
E_MAX = 17
CAP = 500                                                      # Acrobot-v1's TimeLimit
DEV = "cuda:0"
ENV = "Acrobot-v1"
NET = {"dqn_cartpole": (0, 2), "ddqn_per_duel_cartpole": (1, 1), "noisy_dqn_cartpole": (1, 2), "rainbow_dqn_cartpole": (2, 2)}   # (net, n_hidden)
ALL4 = list(NET)
# (th1, th2, dth1, dth2): over the line on the first step whatever the action; one step below the line — over it under every
# action; over it under action 2 only (22 and 31 steps under actions 0 and 1); hanging at rest
STARTS = np.array([(3.0, 0.0, 0.0, 0.0), (2.0, 0.0, 1.0, 0.0), (2.0, 0.0, 0.8, 0.0), (0.0, 0.0, 0.0, 0.0)])


def _trainer(algo, hidden, seed=5, **more):
    return _any_trainer(algo, hidden, seed=seed, env_name=ENV, **more)


def _loop(tr, E, cap, seed=SEED, id0=ID0, start=None):
    """The step loop: -> (returns f32, lengths i32, terminated u8, final_obs f32) of the first episode of envs id0 .. id0 + E - 1,
    cut at `cap` steps.  An env's episode does not depend on the vector it is stepped in: E envs are the first E of more."""
    from gymrl_amd.envs import VecEnv
    env = VecEnv(ENV, E, device=DEV, seed=seed, env_id0=id0)
    obs = env.reset()
    if start is not None:
        _write_state(env, start)                               # (th1, th2, dth1, dth2) are the state buffer's first four float64 fields
        obs = torch.from_numpy(np.stack([ref.obs_of(tuple(y)) for y in start])).to(DEV)
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
    ret = torch.where(torch.isnan(ret), -length.float(), ret)      # an episode cut below the TimeLimit never terminated: -1 per step
    return ret, length, term, fin


def _launch(tr, E, cap, seed=SEED, id0=ID0, **kw):
    call = tr._eval_call()
    assert call is not None and "net" in call and call["kind"] == 5 and call["cap"] == CAP
    return tr._eval_launch(dict(call, cap=cap, **kw), n_episodes=E, seed=seed, stream_id0=id0, want_final_obs=True)


def _same(got, want, E, what=""):
    for name, g, w in zip(("returns", "lengths", "terminated", "final_obs"), got, want):
        assert g.shape[0] == 1 and g.dtype == w.dtype and torch.equal(g[0], w[:E]), (what, name, g[0], w[:E])


def _np(out):
    return tuple(x[0].cpu().numpy() for x in out)


_REFS = {}


def _ref(algo, hidden):
    """One trainer and its loop over E_MAX envs per (algorithm, width), computed once and shared (never modified)."""
    if (algo, hidden) not in _REFS:
        tr = _trainer(algo, hidden)
        _REFS[algo, hidden] = (tr, _loop(tr, E_MAX, CAP))
    return _REFS[algo, hidden]


# ---- (1) freshly initialised networks: nets 0 / 1 / 2, one and two hidden layers, H = 8 / 64 / 256, E = 1 / 17, drawn starts -----
@pytest.mark.parametrize("algo", ALL4)
@pytest.mark.parametrize("hidden", [8, 64, 256])
def test_kernel_equals_loop(algo, hidden):
    from gymrl_amd import ops
    tr, want = _ref(algo, hidden)
    call = tr._eval_call()
    assert (call["net"], len(call["trunk"])) == NET[algo] and (call["value"] is None) == (algo == "dqn_cartpole")
    assert tuple(call["trunk"][0][0].shape) == (hidden, 6) and tuple(call["head"][0].shape) == (3, hidden)
    fc2 = call["trunk"][1][0] if len(call["trunk"]) == 2 else None
    variants = [None] + ([ops.lin_fwd_image(fc2)] if fc2 is not None and hidden % 16 == 0 else [])
    for E in (1, E_MAX):
        for img in variants:
            _same(_launch(tr, E, CAP, images=img), want, E, (E, img is not None))
    lengths, term = want[1].cpu().numpy(), want[2].cpu().numpy()
    print(f"{algo} hidden {hidden}: lengths {sorted(set(lengths.tolist()))}, terminated {int(term.sum())} of {E_MAX}")
    a, b = _launch(tr, E_MAX, CAP), _launch(tr, E_MAX, CAP)      # two launches give the same bits
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- (2) the hand-set pump policy: episodes that end before the TimeLimit, beside ones still running --------------------------------
def _set_pump(tr):
    """acrobot_ref.pump — action 0 while dth1 >= 0, else 2 — through the ReLU pair relu(s), relu(-s) with s = dth1 (observation 4):
    fc1 rows 0 / 1 = +-e4, a second trunk layer passes both on, Q0 (advantage 0) = relu(s), Q1 = 0, Q2 = relu(-s); a dueling
    network's value head is zero.  Equal Q at s = 0 gives action 0."""
    call = tr._eval_call()
    trunk, head, value = call["trunk"], call["head"], call["value"]
    with torch.no_grad():
        for w, b in list(trunk) + [head] + ([value] if value is not None else []):
            w.zero_()
            b.zero_()
        trunk[0][0][0, 4], trunk[0][0][1, 4] = 1.0, -1.0
        if len(trunk) == 2:
            trunk[1][0][0, 0] = trunk[1][0][1, 1] = 1.0
        head[0][0, 0] = head[0][2, 1] = 1.0


_PUMP = []


def _pump_population(cap=CAP):
    if not _PUMP:
        _PUMP.append(ref.eval_population(SEED, ID0, E_MAX, [ref.pump]))
    ret, length, term, fin = _PUMP[0]
    assert length[0, :16].tolist() == [76, 78, 79, 97, 82, 79, 82, 77, 74, 127, 77, 76, 99, 95, 79, 88] and term.all()
    return _PUMP[0] if cap == CAP else ref.eval_population(SEED, ID0, E_MAX, [ref.pump], cap=cap)


@pytest.mark.parametrize("algo", ALL4)
def test_pump_policy_swings_up(algo):
    want = _pump_population()
    tr = _trainer(algo, 8)
    _set_pump(tr)
    got = _launch(tr, E_MAX, CAP)
    for g, w, name in zip(_np(got), want, ("returns", "lengths", "terminated", "final_obs")):
        assert g.dtype == w.dtype and np.array_equal(g, w[0]), name        # the CPU restatement: finished lanes idle beside running ones
    assert np.array_equal(_np(got)[0], -(want[1][0] - 1).astype(np.float32))   # -1 per step but the last
    _same(got, _loop(tr, E_MAX, CAP), E_MAX)
    _same(_launch(tr, 1, CAP), _loop(tr, 1, CAP), 1)


# ---- (3) caps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 7])
def test_cap_cuts_the_episodes(cap):
    want = _pump_population(cap)
    assert (want[1] == cap).all() and not want[2].any() and (want[0] == -float(cap)).all()
    for algo in ALL4:
        tr = _trainer(algo, 8)
        _set_pump(tr)
        for E in (1, E_MAX):
            got = _launch(tr, E, cap)
            _same(got, _loop(tr, E, cap), E, (algo, cap, E))
        for g, w in zip(_np(got), want):
            assert np.array_equal(g, w[0])
        fresh = _ref(algo, 64)[0]
        _same(_launch(fresh, E_MAX, cap), _loop(fresh, E_MAX, cap), E_MAX, (algo, cap, "fresh"))


# ---- (4) a start tensor -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALL4)
def test_start_tensor(algo):
    n = len(STARTS)
    assert [bool(ref.height_reached(y[0], y[1])) for y in STARTS] == [True, False, False, False]      # two start below the line
    want = ref.eval_population(SEED, 0, n, [ref.pump], start=STARTS[None])
    assert want[1][0].tolist()[:3] == [1, 1, 22] and want[2][0].tolist() == [1, 1, 1, 1] and want[0][0, 0] == 0.0 and want[0][0, 1] == 0.0
    assert ref.episode(tuple(STARTS[2]), lambda o, t: 2)["len"] == 1                # the same state under the other torque: one step
    tr = _trainer(algo, 8)
    _set_pump(tr)
    start = torch.from_numpy(STARTS).to(DEV).view(1, n, 4)
    for cap in (1, CAP):
        got = _launch(tr, n, cap, start=start)
        _same(got, _loop(tr, n, cap, start=STARTS), n, (algo, cap))
        if cap == CAP:
            for g, w, name in zip(_np(got), want, ("returns", "lengths", "terminated", "final_obs")):
                assert np.array_equal(g, w[0]), name
        else:
            assert _np(got)[1].tolist() == [1] * n and _np(got)[2].tolist() == [1, 1, 0, 0] and _np(got)[0].tolist() == [0.0, 0.0, -1.0, -1.0]
    fresh = _ref(algo, 64)[0]
    _same(_launch(fresh, n, CAP, start=start), _loop(fresh, n, CAP, start=STARTS), n, (algo, "fresh"))
    _same(_launch(fresh, 1, CAP, start=start[:, :1].contiguous()), _loop(fresh, 1, CAP, start=STARTS[:1]), 1, (algo, "1 x 1"))


# ---- (5) net 2 on one hidden layer: no trainer has it -------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [8, 64])
def test_row_mean_on_one_hidden_layer(hidden):
    """Rainbow's network with an identity second layer is its first layer under the same heads: relu(1 * h + 0) = h exactly for a
    ReLU output h.  The two-layer launch is the trainer's loop (above), the one-layer launch must give the same episodes."""
    from gymrl_amd import ops
    tr = _trainer("rainbow_dqn_cartpole", hidden)
    call = tr._eval_call()
    with torch.no_grad():
        call["trunk"][1][0].copy_(torch.eye(hidden))
        call["trunk"][1][1].zero_()
    kw = dict(n_episodes=E_MAX, seed=SEED, stream_id0=ID0, cap=CAP, want_final_obs=True)
    two = _launch(tr, E_MAX, CAP)
    _same(two, _loop(tr, E_MAX, CAP), E_MAX)
    one = ops.acrobot_net_eval(2, call["trunk"][:1], call["head"], value=call["value"], **kw)
    mean = ops.acrobot_net_eval(1, call["trunk"][:1], call["head"], value=call["value"], **kw)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    assert all(m.shape == a.shape for m, a in zip(mean, one))


# ---- (6) populations: P x E = 3 x 16 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["dqn_cartpole", "noisy_dqn_cartpole", "rainbow_dqn_cartpole"])
def test_a_population_equals_its_members_and_the_loop(algo):
    trs = [_trainer(algo, 64, seed=s) for s in (1, 1, 3)]
    _set_pump(trs[1])                                          # member 1 ends its episodes early: lanes of one launch finish apart
    params = torch.stack([t._eval_call()["flat"] for t in trs])
    tr, call = trs[0], trs[0]._eval_call()
    kw = dict(n_episodes=16, seed=SEED, stream_id0=ID0, want_final_obs=True)
    tight = tr._eval_launch(call, params=params, **kw)
    padded = torch.full((3, params.shape[1] + 68), float("nan"), device=DEV)
    padded[:, :params.shape[1]] = params
    loose = tr._eval_launch(call, params=padded, **kw)
    for a, b in zip(tight, loose):
        assert a.shape[0] == 3 and torch.equal(a, b)
    for p, t in enumerate(trs):
        want = _loop(t, 16, CAP)
        for a, w in zip(tight, want):
            assert torch.equal(a[p], w)
    assert tight[1][1, :16].tolist() == _pump_population()[1][0, :16].tolist() and bool(tight[2][1].all())
    r, n, f = tr.evaluate(16, params=params)
    assert r.shape == n.shape == f.shape == (3, 16) and r.dtype == np.float32 and n.dtype == np.int32 and f.dtype == np.uint8


# ---- (7) through the trainers -------------------------------------------------------------------------------------------------------
def _count_launches(monkeypatch):
    from gymrl_amd import ops
    calls, wrong = [], []
    real = ops.acrobot_net_eval
    monkeypatch.setattr(ops, "acrobot_net_eval", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for other in ("classic_policy_eval", "classic_duel_eval", "mountaincar_net_eval"):
        monkeypatch.setattr(ops, other, lambda *a, **k: wrong.append(1))
    return calls, wrong


@pytest.mark.parametrize("algo", ["dqn_cartpole", "ddqn_per_duel_cartpole"])
def test_trainer_trains_on_the_layer_path_and_eval_is_the_same_list(algo, monkeypatch):
    tr = _trainer(algo, 64)
    assert tr.env.name == ENV and (tr.env.obs_dim, tr.env.act_dim) == (6, 3)
    tr.train(max_vector_steps=20)
    assert len(tr.memory) > 0
    calls, wrong = _count_launches(monkeypatch)
    before = _untouched(tr)
    for n in (10, 5):
        tr.cfg.fused_eval = False
        want = tr.eval(n)
        assert not calls
        tr.cfg.fused_eval = True
        got = tr.eval(n)
        assert len(calls) == 1 and calls.pop()                 # exactly one launch
        assert len(got) == n and got == want, (got, want)
        assert all(-500.0 <= x <= 0.0 for x in got)
    assert not wrong
    after = _untouched(tr)
    assert after[0] == before[0], (after[0], before[0])
    for x, y in zip(after[1], before[1]):
        assert torch.equal(x, y)
    wide = _trainer(algo, 260)                                 # a refused shape keeps the loop
    wide.cfg.fused_eval = True
    assert wide._eval_call() is None and len(wide.eval(3)) == 3 and not calls and not wrong
    with pytest.raises(RuntimeError):
        wide.evaluate(3)


def test_es_on_acrobot_replays_from_its_seed():
    from gymrl_amd.es_cartpole import Config, ESTrainer

    def run():
        cfg = Config()
        cfg.env_name, cfg.seed, cfg.population, cfg.episodes_per_policy, cfg.log_freq = ENV, 3, 16, 4, 0
        tr = ESTrainer(cfg)
        assert tr.discrete and tr._call["kind"] == 5 and tr._call["net"] == 0 and tr._call["cap"] == CAP
        first = tr.flat_params.clone()
        tr.train(max_generations=2)
        assert tr.generation == 2 and tuple(tr.last_returns.shape) == (16, 4)
        assert bool(((tr.last_returns >= -500.0) & (tr.last_returns <= 0.0)).all())
        return first, tr.flat_params.clone(), tr.last_returns.clone(), tr.eval(3)

    a, b = run(), run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]
