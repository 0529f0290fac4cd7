"""Whole evaluation episodes of MountainCar-v0 in one launch (csrc/eval_net.hip: gymrl_mountaincar_net_eval) against the
loop they replace: a VecEnv("MountainCar-v0") on the same streams stepped under the trainer's own
select_action(deterministic=True), first episode per env.  Six trainers: three three-layer networks (net 0), two dueling ones
that combine through torch's mean (net 1) and Rainbow, which combines in the layer kernels' DUELING epilogue (net 2).  The
kernels run the layer path's tiles, the trainers' combines and the stepper's env core, so every comparison is torch.equal /
array_equal: returns, lengths, terminated flags, terminal observations.  Expected lengths of the hand-set policies come from the
plain-Python restatement tests/mountaincar_ref.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import mountaincar_ref as ref  # noqa: E402
from test_classic_eval_gpu import _trainer as _any_trainer, _write_state  # noqa: E402
from test_duel_eval_gpu import _untouched  # noqa: E402

SEED, ID0 = 1041, 1 << 40
E_MAX, E_CASES = 33, (1, 16, 17, 33)
CAP = 200                                                      # MountainCar-v0's TimeLimit
DEV = "cuda:0"
ENV = "MountainCar-v0"
MLP3 = ["dqn_cartpole", "ddqn_per_cartpole", "sac_cartpole"]
DUEL = ["rainbow_dqn_cartpole", "ddqn_per_duel_cartpole", "noisy_dqn_cartpole"]
ALL6 = MLP3 + DUEL
NET = {"rainbow_dqn_cartpole": 2, "ddqn_per_duel_cartpole": 1, "noisy_dqn_cartpole": 1}      # the others: 0
ONE_PER_NET = ["dqn_cartpole", "noisy_dqn_cartpole", "rainbow_dqn_cartpole"]


def _trainer(algo, hidden, seed=5, **more):
    return _any_trainer(algo, hidden, seed=seed, env_name=ENV, **more)


def _loop(tr, E, cap, seed=SEED, id0=ID0, start=None):
    """The step loop: -> (returns f32, lengths i32, terminated u8, final_obs f32) of the first episode of envs id0 .. id0 + E - 1,
    cut at `cap` steps.  An env's episode does not depend on the vector it is stepped in: E envs are the first E of more."""
    from gymrl_amd.envs import VecEnv
    env = VecEnv(ENV, E, device=DEV, seed=seed, env_id0=id0)
    obs = env.reset()
    if start is not None:
        _write_state(env, start)                               # (pos, vel) are the state buffer's first two float64 fields
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
    ret = torch.where(torch.isnan(ret), -length.float(), ret)      # an episode cut below the TimeLimit: -1 per step so far
    return ret, length, term, fin


def _launch(tr, E, cap, seed=SEED, id0=ID0, **kw):
    call = tr._eval_call()
    assert call is not None and "net" in call
    return tr._eval_launch(dict(call, cap=cap, **kw), n_episodes=E, seed=seed, stream_id0=id0, want_final_obs=True)


def _same(got, want, E, what=""):
    for name, g, w in zip(("returns", "lengths", "terminated", "final_obs"), got, want):
        assert g.shape[0] == 1 and torch.equal(g[0], w[:E]), (what, name, g[0], w[:E])


def _np(out):
    return tuple(x[0].cpu().numpy() for x in out)


_REFS = {}


def _ref(algo, hidden):
    """One trainer and its loop over E_MAX envs per (algorithm, width), computed once and shared (never modified)."""
    if (algo, hidden) not in _REFS:
        tr = _trainer(algo, hidden)
        _REFS[algo, hidden] = (tr, _loop(tr, E_MAX, CAP))
    return _REFS[algo, hidden]


def _fc2_weight(tr):
    call = tr._eval_call()
    return call["trunk"][1][0] if len(call["trunk"]) == 2 else None


# ---- (1) freshly initialised networks -------------------------------------------------------------------------------------
# hidden 36: no image, not a multiple of 16; 64: with and without the forward image of fc2; 256: the instances built for that width
@pytest.mark.parametrize("algo", ALL6)
@pytest.mark.parametrize("hidden", [36, 64, 256])
def test_kernel_equals_loop(algo, hidden):
    from gymrl_amd import ops
    tr, want = _ref(algo, hidden)
    call = tr._eval_call()
    assert call["net"] == NET.get(algo, 0) and len(call["trunk"]) == (1 if algo == "ddqn_per_duel_cartpole" else 2)
    assert (call["value"] is None) == (algo in MLP3)
    fc2 = _fc2_weight(tr)
    variants = [None] + ([ops.lin_fwd_image(fc2)] if fc2 is not None and hidden % 16 == 0 else [])
    for E in E_CASES:
        for img in variants:
            _same(_launch(tr, E, CAP, images=img), want, E, (E, img is not None))
    ret, lengths, term = (x.cpu().numpy() for x in want[:3])
    print(f"{algo} hidden {hidden}: lengths {sorted(set(lengths.tolist()))}, terminated {int(term.sum())} of {E_MAX}")
    # observed on the MI355X for all eighteen (trainer, width) pairs: a fresh network does not pump the car up the hill, every one
    # of the 33 episodes runs into the TimeLimit — 200 steps, not terminated, -200
    assert (lengths == CAP).all() and not term.any() and (ret == -float(CAP)).all()


# ---- (2) the hand-set pump policy -----------------------------------------------------------------------------------------------
def _set_pump(tr):
    """`push right iff velocity > 0, else left` through the ReLU pair relu(s), relu(-s) with s = vel: fc1 rows 0 / 1 = +-(0, 1), a
    second trunk layer passes both on, Q0 (advantage 0) = relu(-s), Q1 = 0, Q2 = relu(s); a dueling network's value head is zero.
    Equal Q at s = 0 gives action 0."""
    call = tr._eval_call()
    trunk, head, value = call["trunk"], call["head"], call["value"]
    with torch.no_grad():
        for w, b in list(trunk) + [head] + ([value] if value is not None else []):
            w.zero_()
            b.zero_()
        trunk[0][0][0, 1], trunk[0][0][1, 1] = 1.0, -1.0
        if len(trunk) == 2:
            trunk[1][0][0, 0] = trunk[1][0][1, 1] = 1.0
        head[0][0, 1] = head[0][2, 0] = 1.0


_PUMP = []


def _pump_episodes():
    """The 33 episodes of the reset draws under the pump policy, on the CPU restatement."""
    if not _PUMP:
        _PUMP.append([ref.episode(*ref.draw(SEED, ID0 + e), act=ref.pump) for e in range(E_MAX)])
    return _PUMP[0]


@pytest.mark.parametrize("algo", ALL6)
def test_pump_policy_reaches_the_flag(algo):
    eps = _pump_episodes()
    want_len = np.array([o["len"] for o in eps], np.int32)
    assert all(o["reached"] for o in eps)
    assert (want_len[:16].min(), want_len[:16].max(), want_len.min(), want_len.max()) == (88, 169, 86, 173)
    tr = _trainer(algo, 8)
    _set_pump(tr)
    got = _launch(tr, E_MAX, CAP)
    ret, lengths, term, fin = _np(got)
    assert np.array_equal(lengths, want_len)                   # finished lanes idle beside running ones
    assert (term == 1).all() and np.array_equal(ret, -lengths.astype(np.float32))
    assert np.array_equal(fin, np.array([(o["pos"], o["vel"]) for o in eps], np.float64).astype(np.float32))
    _same(got, _loop(tr, E_MAX, CAP), E_MAX)


# ---- (3) start overrides ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ONE_PER_NET)
def test_start_overrides(algo):
    tr = _trainer(algo, 8)
    _set_pump(tr)
    # at the flag after one step, whatever the action
    start = np.array([[0.49, 0.07]])
    got = _launch(tr, 1, CAP, start=torch.from_numpy(start).to(DEV).view(1, 1, 2))
    assert got[0].item() == -1.0 and got[1].item() == 1 and got[2].item() == 1
    _same(got, _loop(tr, 1, CAP, start=start), 1)
    # into the left wall (inelastic: the velocity is zeroed there), then pumped up to the flag
    start = np.array([[-1.19, -0.07]])
    want = ref.episode(-1.19, -0.07, act=ref.pump)
    assert want["len"] == 40 and want["reached"] and want["hit_wall"]
    got = _launch(tr, 1, CAP, start=torch.from_numpy(start).to(DEV).view(1, 1, 2))
    assert got[0].item() == -40.0 and got[1].item() == 40 and got[2].item() == 1
    _same(got, _loop(tr, 1, CAP, start=start), 1)
    # a zeroed last layer: equal Q values, the first maximum is action 0 throughout — pushed left for 200 steps
    head = tr._eval_call()["head"]
    with torch.no_grad():
        for t in head:
            t.zero_()
    start = np.array([[-0.5, 0.0]])
    want = ref.episode(-0.5, 0.0, act=lambda p, v: 0)
    assert want["len"] == CAP and not want["reached"]
    got = _launch(tr, 1, CAP, start=torch.from_numpy(start).to(DEV).view(1, 1, 2))
    assert got[0].item() == -200.0 and got[1].item() == CAP and got[2].item() == 0
    assert np.array_equal(_np(got)[3][0], np.array([want["pos"], want["vel"]]).astype(np.float32))
    _same(got, _loop(tr, 1, CAP, start=start), 1)


# ---- (4) caps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [7, 1])
def test_cap_cuts_the_episodes(cap):
    full = np.array([o["len"] for o in _pump_episodes()], np.int32)[:17]
    for algo in ONE_PER_NET:
        tr = _trainer(algo, 8)
        _set_pump(tr)
        got = _launch(tr, 17, cap)
        _same(got, _loop(tr, 17, cap), 17, (algo, cap))
        ret, lengths, term, _ = _np(got)
        assert (lengths == np.minimum(full, cap)).all() and (ret == -lengths).all() and (term == 0).all()


# ---- (5) determinism ------------------------------------------------------------------------------------------------------------
def test_two_launches_give_the_same_bits():
    for algo in ALL6:
        tr = _ref(algo, 64)[0]
        a, b = _launch(tr, 33, CAP), _launch(tr, 33, CAP)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ---- (6) populations --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ONE_PER_NET)
def test_a_population_equals_its_members_and_the_loop(algo):
    trs = [_trainer(algo, 64, seed=s) for s in (1, 1, 3)]
    with torch.no_grad():                                      # member 1: member 0 with the last layer negated — another action
        for t in trs[1]._eval_call()["head"]:                  # wherever the Q values differ
            t.neg_()
    params = torch.stack([t._eval_call()["flat"] for t in trs])
    tr, call = trs[0], trs[0]._eval_call()
    kw = dict(n_episodes=17, seed=SEED, stream_id0=ID0, want_final_obs=True)
    tight = tr._eval_launch(call, params=params, **kw)
    padded = torch.full((3, params.shape[1] + 68), float("nan"), device=DEV)
    padded[:, :params.shape[1]] = params
    loose = tr._eval_launch(call, params=padded, **kw)
    ragged = tr._eval_launch(call, params=padded[:, :params.shape[1] + 3].contiguous(), **kw)      # padded by the binding
    for a, b, c in zip(tight, loose, ragged):
        assert a.shape[0] == 3 and torch.equal(a, b) and torch.equal(a, c)
    for p, t in enumerate(trs):
        one = _launch(t, 17, CAP)
        want = _loop(t, 17, CAP)
        for a, b, w in zip(tight, one, want):
            assert torch.equal(a[p], b[0]) and torch.equal(a[p], w)
    assert not torch.equal(tight[3][0], tight[3][1])           # different policies on the same starts end elsewhere
    # the trainer's surface: numpy [P, E] on eval()'s streams
    r, n, f = tr.evaluate(17, params=params)
    assert r.shape == n.shape == f.shape == (3, 17) and r.dtype == np.float32 and n.dtype == np.int32 and f.dtype == np.uint8
    own = tr.evaluate(17)
    assert np.array_equal(own[0][0], r[0]) and np.array_equal(own[1][0], n[0])
    # ... and stream_offset, on a policy whose episodes differ in length: eval()'s streams are this file's with seed SEED - 999
    pump = _trainer(algo, 8, seed=SEED - 999)
    _set_pump(pump)
    assert (pump.base_seed + pump.EVAL_SEED_OFFSET, pump.EVAL_ENV_ID0) == (SEED, ID0)
    want_len = np.array([o["len"] for o in _pump_episodes()], np.int32)
    r, n, f = pump.evaluate(17)
    assert np.array_equal(n[0], want_len[:17]) and np.array_equal(r[0], -want_len[:17].astype(np.float32)) and f.all()
    shifted = pump.evaluate(16, stream_offset=1)
    assert np.array_equal(shifted[1][0], n[0, 1:]) and np.array_equal(shifted[0][0], r[0, 1:])


# ---- (7) the six trainers' surface ------------------------------------------------------------------------------------------------
def _count_launches(monkeypatch):
    from gymrl_amd import ops
    calls, wrong = [], []
    real = ops.mountaincar_net_eval
    monkeypatch.setattr(ops, "mountaincar_net_eval", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for other in ("classic_policy_eval", "classic_duel_eval"):
        monkeypatch.setattr(ops, other, lambda *a, **k: wrong.append(1))
    return calls, wrong


@pytest.mark.parametrize("algo", ALL6)
def test_trainer_eval_is_the_same_list(algo, monkeypatch):
    tr = _trainer(algo, 64)
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
        assert all(-200.0 <= x <= -1.0 for x in got)
    assert tr.test() == tr.eval(5) and len(calls) == 2 and not wrong
    after = _untouched(tr)
    assert after[0] == before[0], (after[0], before[0])
    for x, y in zip(after[1], before[1]):
        assert torch.equal(x, y)
    counter = {"noisy_dqn_cartpole": "noise_draws", "rainbow_dqn_cartpole": "total_steps"}.get(algo)
    assert (counter is None or before[0][counter] > 0) and before[0]["training"] is True


@pytest.mark.parametrize("algo", ALL6)
def test_refused_shape_falls_back_to_the_loop(algo, monkeypatch):
    tr = _trainer(algo, 260)
    calls, wrong = _count_launches(monkeypatch)
    tr.cfg.fused_eval = False
    want = tr.eval(5)
    tr.cfg.fused_eval = True
    assert tr._eval_call() is None and tr.eval(5) == want and not calls and not wrong
    with pytest.raises(RuntimeError):
        tr.evaluate(5)
