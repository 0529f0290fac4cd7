"""Whole evaluation episodes of the dueling networks in one launch (csrc/eval_duel.hip: gymrl_classic_duel_eval) and of
SAC-Pendulum's greedy actor (gymrl_classic_policy_eval, head tanh on fc1 / fc2 / mean) against the loop they replace: a VecEnv on
the same streams stepped under the trainer's own select_action(deterministic=True), first episode per env.  The kernels run the
layer path's tiles, the fused steps' combine and the stepper's env core, so every comparison is torch.equal / array_equal:
returns, lengths, terminated flags, terminal observations."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_classic_eval_gpu import CONTROLLERS, STARTS17, _loop, _oracle_lengths, _trainer  # noqa: E402

SEED, ID0 = 1041, 1 << 40
E_MAX, E_CASES = 33, (1, 16, 17, 33)
DEV = "cuda:0"
DUEL = ["ddqn_per_duel_cartpole", "noisy_dqn_cartpole", "rainbow_dqn_cartpole"]
TWO_LAYER = DUEL[1:]
ALL4 = DUEL + ["sac_pendulum"]


def _launch(tr, E, cap, seed=SEED, id0=ID0, **kw):
    call = tr._eval_call()
    assert call is not None
    return tr._eval_launch(dict(call, cap=cap, **kw), n_episodes=E, seed=seed, stream_id0=id0, want_final_obs=True)


def _same(got, want, E, what=""):
    for name, g, w in zip(("returns", "lengths", "terminated", "final_obs"), got, want):
        assert g.shape[0] == 1 and torch.equal(g[0], w[:E]), (what, name, g[0], w[:E])


_REFS = {}


def _ref(algo, hidden):
    """One trainer and its loop over E_MAX envs per (algorithm, width), computed once and shared (never modified)."""
    if (algo, hidden) not in _REFS:
        tr = _trainer(algo, hidden)
        cap = 500
        _REFS[algo, hidden] = (tr, cap, _loop(tr, E_MAX, cap))
    return _REFS[algo, hidden]


# ---- (1) freshly initialised networks -------------------------------------------------------------------------------------
# hidden 36: no image, not a multiple of 16; 64: with and without the forward image of fc2; 256: the instances built for that width
@pytest.mark.parametrize("algo", DUEL)
@pytest.mark.parametrize("hidden", [36, 64, 256])
def test_kernel_equals_loop(algo, hidden):
    from gymrl_amd import ops
    tr, cap, want = _ref(algo, hidden)
    trunk = tr._eval_duel_policy()[0]
    assert tr._eval_policy() is None and len(trunk) == (1 if algo == DUEL[0] else 2)
    variants = [None] + ([ops.lin_fwd_image(trunk[1][0])] if len(trunk) == 2 and hidden % 16 == 0 else [])
    for E in E_CASES:
        for img in variants:
            got = _launch(tr, E, cap, images=img)
            _same(got, want, E, (E, img is not None))
    lengths = want[1].cpu().numpy()
    assert len(set(lengths[:16].tolist())) >= 2                # one workgroup holds episodes of different lengths


# ---- (2) mu only -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", TWO_LAYER)
def test_noise_parameters_are_not_read(algo):
    tr = _trainer(algo, 64)
    before = _launch(tr, 17, 500)
    net = tr.policy_net
    noisy = [m for m in net.modules() if hasattr(m, "weight_sigma")]
    assert len(noisy) == (4 if algo == "noisy_dqn_cartpole" else 2)
    old_eps = [m.weight_epsilon.clone() for m in noisy]
    with torch.no_grad():
        for m in noisy:
            m.weight_sigma.mul_(10.0)
            m.bias_sigma.mul_(10.0)
    for m in noisy:
        m.reset_noise()                                        # a fresh draw into the epsilon buffers
    assert all(not torch.equal(m.weight_epsilon, e) for m, e in zip(noisy, old_eps))
    after = _launch(tr, 17, 500)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    _same(after, _loop(tr, 17, 500), 17)


# ---- (3), (4) a hand-set controller in dueling form ---------------------------------------------------------------------------
def _set_duel_controller(tr, k, value_bias=0.0, adv_scale=1.0):
    """A linear controller `push right iff k . obs > 0` as a dueling network, through the ReLU pair relu(s), relu(-s): fc1 rows
    0 / 1 = +k / -k, a second trunk layer passes both on, advantage 0 = relu(-s), advantage 1 = relu(s), both times adv_scale; the
    value head is a constant, value_bias."""
    trunk, value, adv, _ = tr._eval_duel_policy()
    with torch.no_grad():
        for w, b in list(trunk) + [value, adv]:
            w.zero_()
            b.zero_()
        kt = torch.tensor(k, dtype=torch.float32, device=DEV)
        trunk[0][0][0], trunk[0][0][1] = kt, -kt
        if len(trunk) == 2:
            trunk[1][0][0, 0] = trunk[1][0][1, 1] = 1.0
        adv[0][0, 1] = adv[0][1, 0] = adv_scale
        value[1].fill_(value_bias)


_PICKED = []


def _picked(orc):
    """The coefficients: the first candidate that, on the CPU oracle's CartPole, holds some of the 17 starts for 500 steps and
    loses others."""
    if not _PICKED:
        for k in CONTROLLERS:
            lengths, term = _oracle_lengths(orc, k, STARTS17)
            if ((lengths == 500) & (term == 0)).any() and ((lengths < 500) & (term == 1)).any():
                _PICKED.append(k)
                break
    assert _PICKED
    return _PICKED[0]


@pytest.mark.parametrize("algo", DUEL)                         # a one-layer trunk, then the two two-layer ones
def test_hand_set_controller_reaches_the_time_limit_and_fails_elsewhere(algo, oracle):
    tr = _trainer(algo, 8)
    _set_duel_controller(tr, _picked(oracle))
    start = torch.from_numpy(STARTS17).to(DEV).view(1, 17, 4)
    got = _launch(tr, 17, 500, start=start)
    ret, lengths, term = (x[0].cpu().numpy() for x in got[:3])
    assert ((lengths == 500) & (term == 0) & (ret == 500.0)).any()       # the TimeLimit, not a termination
    assert ((lengths < 500) & (term == 1)).any()
    assert (ret == lengths).all()
    _same(got, _loop(tr, 17, 500, start=STARTS17), 17)


@pytest.mark.parametrize("algo", ["ddqn_per_duel_cartpole", "noisy_dqn_cartpole"])
def test_the_combine_is_applied(algo, oracle):
    """The value head at 2^24 and |advantage| < 0.5: in float32 v + (a - mean a) is 2^24 for both actions (the spacing of floats
    there is 2), a tie, and the first maximum is action 0 in every step — an argmax over the advantages alone would follow the
    controller.  |a| < 0.5: |k . obs| stays below 2.4 |k0| + 0.21 |k2| + 6 (|k1| + |k3|) < 22 over the few steps a cart pushed left
    only survives, times 2^-7."""
    k = _picked(oracle)
    start = torch.from_numpy(STARTS17).to(DEV).view(1, 17, 4)
    tr = _trainer(algo, 8)
    _set_duel_controller(tr, k, value_bias=float(2 ** 24), adv_scale=2.0 ** -7)
    tied = _launch(tr, 17, 500, start=start)
    _same(tied, _loop(tr, 17, 500, start=STARTS17), 17)
    assert (tied[1][0].cpu().numpy() < 100).all() and (tied[2][0].cpu().numpy() == 1).all()      # pushed left until it fell
    _set_duel_controller(tr, k, value_bias=0.0, adv_scale=2.0 ** -7)
    free = _launch(tr, 17, 500, start=start)
    _same(free, _loop(tr, 17, 500, start=STARTS17), 17)
    assert not torch.equal(tied[1], free[1]) and (free[1][0].cpu().numpy() == 500).any()


# ---- (5) caps and start overrides ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [7, 1])
def test_cap_cuts_the_episodes(cap):
    for algo in ("ddqn_per_duel_cartpole", "rainbow_dqn_cartpole"):
        tr, _, full = _ref(algo, 64)
        want = _loop(tr, 17, cap)
        got = _launch(tr, 17, cap)
        _same(got, want, 17, (algo, cap))
        lengths = got[1][0].cpu().numpy()
        assert (lengths == np.minimum(full[1][:17].cpu().numpy(), cap)).all() and (got[0][0].cpu().numpy() == lengths).all()
        assert (got[2][0].cpu().numpy() == ((full[1][:17].cpu().numpy() <= cap) & (full[2][:17].cpu().numpy() == 1))).all()


@pytest.mark.parametrize("algo", ["ddqn_per_duel_cartpole", "noisy_dqn_cartpole"])
def test_start_overrides(algo):
    tr = _trainer(algo, 64)
    # past the track's end after one step, whatever the action
    start = np.array([[2.39, 2.0, 0.0, 0.0]])
    got = _launch(tr, 1, 500, start=torch.from_numpy(start).to(DEV).view(1, 1, 4))
    assert got[0].item() == 1.0 and got[1].item() == 1 and got[2].item() == 1
    _same(got, _loop(tr, 1, 500, start=start), 1)
    # from the origin under zeroed heads: equal Q values, the first maximum is action 0 throughout
    _, value, adv, _ = tr._eval_duel_policy()
    with torch.no_grad():
        for t in (*value, *adv):
            t.zero_()
    start = np.zeros((1, 4))
    got = _launch(tr, 1, 500, start=torch.from_numpy(start).to(DEV).view(1, 1, 4))
    want = _loop(tr, 1, 500, start=start)
    _same(got, want, 1)
    assert got[2].item() == 1 and 1 < got[1].item() < 30 and got[3][0, 0, 0].item() < 0.0      # pushed left until the pole fell


# ---- (6) populations --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", TWO_LAYER)                    # NoisyNet: mu and sigma alternate in the flat buffer; Rainbow: the heads'
def test_a_population_equals_its_members_and_the_loop(algo):
    trs = [_trainer(algo, 64, seed=s) for s in (1, 1, 3)]
    with torch.no_grad():                                      # member 1: member 0 with the advantage head negated — the other action
        for t in trs[1]._eval_duel_policy()[2]:                # wherever the two advantages differ
            t.neg_()
    params = torch.stack([t.flat_params for t in trs])
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
        one = _launch(t, 17, 500)
        want = _loop(t, 17, 500)
        for a, b, w in zip(tight, one, want):
            assert torch.equal(a[p], b[0]) and torch.equal(a[p], w)
    assert not torch.equal(tight[3][0], tight[3][1])           # different policies on the same starts end elsewhere
    # the trainer's surface: numpy [P, E] on eval()'s streams
    r, n, f = tr.evaluate(17, params=params)
    assert r.shape == n.shape == f.shape == (3, 17) and r.dtype == np.float32 and n.dtype == np.int32 and f.dtype == np.uint8
    own = tr.evaluate(17)
    assert np.array_equal(own[0][0], r[0]) and np.array_equal(own[1][0], n[0])
    shifted = tr.evaluate(16, stream_offset=1)
    assert np.array_equal(shifted[1][0], own[1][0, 1:])


# ---- (7) the four trainers' surface -------------------------------------------------------------------------------------------
def _count_launches(monkeypatch, algo):
    from gymrl_amd import ops
    mine = "classic_policy_eval" if algo == "sac_pendulum" else "classic_duel_eval"
    other = "classic_duel_eval" if algo == "sac_pendulum" else "classic_policy_eval"
    calls, wrong, real, real_other = [], [], getattr(ops, mine), getattr(ops, other)
    monkeypatch.setattr(ops, mine, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(ops, other, lambda *a, **k: (wrong.append(1), real_other(*a, **k))[1])
    return calls, wrong


def _untouched(tr):
    """What neither eval() nor evaluate() may move: the replay ring and its cursors, the env, every exploration / noise counter."""
    from gymrl_amd.rainbow_dqn_cartpole import NoisyLinear
    m = tr.memory
    scalars = {k: getattr(m, k) for k in ("cursor", "size", "count", "current_size", "pushes", "draws") if hasattr(m, k)}
    scalars.update({k: getattr(tr, k) for k in ("_act_counter", "noise_draws", "total_steps", "sample_count", "epsilon", "_act_noise",
                                                "_upd_noise") if hasattr(tr, k)})
    scalars["NoisyLinear._counter"] = NoisyLinear._counter
    scalars["training"] = (tr.policy_net if hasattr(tr, "policy_net") else tr.actor).training
    return scalars, [t.clone() for t in m.ring] + [tr.env.state.clone()]


@pytest.mark.parametrize("algo", ALL4)
def test_trainer_eval_is_the_same_list(algo, monkeypatch):
    tr = _trainer(algo, 64)
    tr.train(max_vector_steps=20)
    assert len(tr.memory) > 0
    calls, wrong = _count_launches(monkeypatch, algo)
    # SAC-Pendulum's eval() keeps the loop with the switch on (torch.tanh is not the launch's tanh: test_sac_pendulum_* below)
    per_call = 0 if algo == "sac_pendulum" else 1
    before = _untouched(tr)
    for n in (10, 5):
        tr.cfg.fused_eval = False
        want = tr.eval(n)
        assert not calls
        tr.cfg.fused_eval = True
        got = tr.eval(n)
        assert len(calls) == per_call and (not calls or calls.pop())
        assert len(got) == n and got == want, (got, want)
    assert tr.test() == tr.eval(5) and len(calls) == 2 * per_call and not wrong
    after = _untouched(tr)
    assert after[0] == before[0], (after[0], before[0])
    for x, y in zip(after[1], before[1]):
        assert torch.equal(x, y)
    counter = {"noisy_dqn_cartpole": "noise_draws", "rainbow_dqn_cartpole": "total_steps"}.get(algo)
    assert (counter is None or before[0][counter] > 0) and before[0]["training"] is True


# ---- (8) SAC-Pendulum -----------------------------------------------------------------------------------------------------------
# torch.tanh (Actor.get_action) and the layer kernels' tanh epilogue (the launch) differ in the last place on some means, so the
# launch is compared with a loop that takes the epilogue: ops.lin_fwd of the mean layer with act = tanh, times the bound.
class _EpilogueTanhActor:
    """select_action(deterministic=True) of a SAC-Pendulum trainer with the mean layer's tanh taken inside gymrl_lin_fwd."""

    def __init__(self, tr):
        self.tr, self.cfg = tr, tr.cfg

    def trunk(self, obs):
        return self.tr.actor.fc2(self.tr.actor.fc1(obs))

    @torch.no_grad()
    def select_action(self, obs, deterministic=True):
        from gymrl_amd import ops
        mean = self.tr.actor.mean
        return ops.lin_fwd(self.trunk(obs).contiguous(), mean.weight, mean.bias, ops.LIN_ACT["tanh"]) * self.tr.action_bound


_SAC_REFS = {}


def _sac_ref(hidden):
    if hidden not in _SAC_REFS:
        tr = _trainer("sac_pendulum", hidden, seed=SEED - 999)         # eval()'s streams are this file's: seed SEED, env ids from ID0
        _SAC_REFS[hidden] = (tr, _loop(_EpilogueTanhActor(tr), E_MAX, 200))
    return _SAC_REFS[hidden]


@pytest.mark.parametrize("hidden", [64, 256])
def test_sac_pendulum_equals_the_epilogue_loop(hidden):
    tr, want = _sac_ref(hidden)
    (fc1, fc2, head), flat, kind, bound = tr._eval_policy()
    assert head is tr.actor.mean and flat is tr.actor_flat and bound == 2.0
    got = _launch(tr, 17, 200)
    _same(got, want, 17)
    lengths = want[1].cpu().numpy()
    assert (lengths == 200).all() and not want[2].cpu().numpy().any()          # Pendulum never terminates: the TimeLimit
    assert float(want[0].max()) < 0.0
    assert (tr.base_seed + tr.EVAL_SEED_OFFSET, tr.EVAL_ENV_ID0) == (SEED, ID0)
    r, n, f = tr.evaluate(17)                                                  # the trainer's surface: the same streams
    assert r.shape == n.shape == f.shape == (1, 17) and r.dtype == np.float32 and n.dtype == np.int32 and f.dtype == np.uint8
    assert np.array_equal(r[0], want[0][:17].cpu().numpy()) and (n == 200).all() and not f.any()
    shifted = tr.evaluate(16, stream_offset=1)
    assert np.array_equal(shifted[0][0], r[0, 1:])


@pytest.mark.parametrize("hidden", [64, 256])
def test_sac_pendulum_only_the_tanh_differs(hidden):
    """Why eval() keeps the loop for this trainer: on Pendulum observations the pre-tanh means of Actor.forward (both heads in one
    launch) and of the mean layer on its own agree bit for bit, and torch.tanh of them is not the epilogue's tanh everywhere."""
    from gymrl_amd import ops
    tr, _ = _sac_ref(hidden)
    g = torch.Generator().manual_seed(7)
    theta = (torch.rand(4096, generator=g, dtype=torch.float64) * 2.0 - 1.0) * np.pi
    thdot = (torch.rand(4096, generator=g, dtype=torch.float64) * 2.0 - 1.0) * 8.0
    obs = torch.stack([theta.cos(), theta.sin(), thdot], dim=1).float().to(DEV)
    with torch.no_grad():
        mean_fwd = tr.actor(obs)[0]
        h = _EpilogueTanhActor(tr).trunk(obs).contiguous()
        m = tr.actor.mean
        mean_own = ops.lin_fwd(h, m.weight, m.bias, ops.LIN_ACT["none"])
        epilogue = ops.lin_fwd(h, m.weight, m.bias, ops.LIN_ACT["tanh"])
    assert torch.equal(mean_fwd, mean_own)
    lib_tanh = torch.tanh(mean_fwd)
    differ = int((lib_tanh != epilogue).sum().item())
    print(f"hidden {hidden}: torch.tanh != tanh epilogue on {differ} of {obs.shape[0]} means, "
          f"max |difference| {float((lib_tanh - epilogue).abs().max().item()):.3e}")
    assert differ > 0
    assert float((lib_tanh - epilogue).abs().max().item()) < 1e-6          # the last places of a value in (-1, 1), no more
    assert tr._eval_fused(5) is None and tr.cfg.fused_eval is False


# ---- (9) fallbacks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALL4)
def test_refused_shape_falls_back_to_the_loop(algo, monkeypatch):
    tr = _trainer(algo, 260)
    calls, wrong = _count_launches(monkeypatch, algo)
    tr.cfg.fused_eval = False
    want = tr.eval(5)
    tr.cfg.fused_eval = True
    assert tr._eval_call() is None and tr.eval(5) == want and not calls and not wrong
    with pytest.raises(RuntimeError):
        tr.evaluate(5)


# ---- (10) determinism ---------------------------------------------------------------------------------------------------------
def test_two_launches_give_the_same_bits():
    for algo in ALL4:
        tr, cap = (_ref(algo, 64)[0], 500) if algo in DUEL else (_sac_ref(64)[0], 200)
        a, b = _launch(tr, 33, cap), _launch(tr, 33, cap)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
