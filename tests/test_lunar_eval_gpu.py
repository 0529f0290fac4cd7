"""Whole LunarLander-v3 evaluation episodes in ONE launch (csrc/eval_lunar.hip) against the step loop they replace, bit for bit:
returns (float64), lengths, terminated flags and terminal observations.

The reference steps VecEnv("LunarLander-v3", E, seed, env_id0=stream_id0) under the policy's one-launch forward (PPO:
ActorCritic.act_forward = gymrl_mlp_forward; PPO-full: forward_inference) and gymrl_categorical_sample(deterministic), keeps the
first episode of every env and sums its float32 rewards itself in float64, in step order.  Every case ends at its first crash
(some tens to a few hundred steps) or at its cap."""
import functools

import numpy as np
import pytest
import torch

from gymrl_amd import ops

pytestmark = pytest.mark.gpu

SEED, STREAM0 = 11, 1 << 40
DEV = "cuda:0"


def _loop(forward, E, seed=SEED, stream_id0=STREAM0, cap=1000):
    """-> (returns f64[E], lengths i32[E], terminated u8[E], terminal_obs f32[E, 8]) of the first episode of every env, cut at `cap`."""
    from gymrl_amd.envs import VecEnv
    env = VecEnv("LunarLander-v3", E, device=DEV, seed=seed, env_id0=stream_id0)
    obs = env.reset()
    nxt = torch.empty_like(obs)
    rews, dones, terms, tobs = [], [], [], []
    running = torch.ones(E, dtype=torch.bool, device=DEV)
    for t in range(cap):
        act = ops.categorical_sample(forward(obs), deterministic=True)[0]
        rew = torch.empty(E, device=DEV)
        done, term = (torch.zeros(E, dtype=torch.uint8, device=DEV) for _ in range(2))
        tob = torch.empty(E, 8, device=DEV)
        env.step(act, nxt, rew, done_out=done, term_obs_out=tob, terminated_out=term)
        rews.append(rew), dones.append(done), terms.append(term), tobs.append(tob)
        running &= ~done.bool()
        obs, nxt = nxt, obs
        if t % 32 == 31 and not bool(running.any()):
            break
    rews, dones, terms, tobs = (torch.stack(x).cpu().numpy() for x in (rews, dones, terms, tobs))
    T = rews.shape[0]
    ret, length = np.zeros(E, np.float64), np.zeros(E, np.int32)
    terminated, final = np.zeros(E, np.uint8), np.zeros((E, 8), np.float32)
    for e in range(E):
        hit = np.flatnonzero(dones[:, e])
        last = int(hit[0]) if hit.size else T - 1
        assert hit.size or T == cap                               # every episode ended, or was cut at the cap
        r = 0.0
        for t in range(last + 1):
            r = r + float(rews[t, e])
        ret[e], length[e], final[e] = r, last + 1, tobs[last, e]
        terminated[e] = terms[last, e] if hit.size else 0
    return ret, length, terminated, final


def _model(hidden, seed=0):
    from gymrl_amd.ppo_lunarlander import ActorCritic
    g = torch.random.get_rng_state()
    torch.manual_seed(seed)
    m = ActorCritic(8, 4, hidden)
    torch.random.set_rng_state(g)
    return m.to(DEV)


def _act(model):
    model.refresh_act()
    return lambda obs: model.act_forward(obs, refresh=False)[0]


def _launch(policy, E, **kw):
    return tuple(t.cpu().numpy() for t in ops.lunar_policy_eval(policy, E, kw.pop("seed", SEED), kw.pop("stream_id0", STREAM0), **kw))


def _same(got, want):
    """got: the launch's [P, E] arrays for P == 1, or one policy's rows; want: the loop's."""
    for g, w, name in zip(got, want, ("returns", "lengths", "terminated", "terminal_obs")):
        g = g[0] if g.ndim == w.ndim + 1 else g
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, g, w)


@functools.lru_cache(maxsize=None)
def _fresh(hidden, E):
    """A freshly initialised ActorCritic's loop and launch at (hidden, E), computed once."""
    model = _model(hidden)
    want = _loop(_act(model), E)
    got = _launch(model._act_net(), E)
    return want, got


@pytest.mark.parametrize("hidden,E", [(64, 1), (64, 16), (64, 17), (256, 17)])
def test_fresh_policy_matches_the_loop(hidden, E):
    want, got = _fresh(hidden, E)
    assert got[0].shape == (1, E) and got[0].dtype == np.float64 and got[3].shape == (1, E, 8)
    _same(got, want)
    assert want[1].min() >= 1


def test_quads_of_one_workgroup_end_at_different_steps():
    want, got = _fresh(64, 16)
    assert len(set(want[1].tolist())) >= 2                        # a quad idles while its neighbours step
    _same(got, want)


def _constant(k):
    """The policy that always takes action k (None: four equal logits)."""
    model = _model(64, seed=1)
    with torch.no_grad():
        model.actor[2].weight.zero_()
        model.actor[2].bias.zero_()
        if k is not None:
            model.actor[2].bias[k] = 1.0
    return model


@functools.lru_cache(maxsize=None)
def _constant_loop(k):
    return _loop(_act(_constant(k)), 4)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_constant_action(k):
    """No-op, both side engines and the main engine: each drives the solver through its contacts to the end of the episode."""
    model = _constant(k)
    model.refresh_act()
    _same(_launch(model._act_net(), 4), _constant_loop(k))


def test_equal_logits_take_the_first_action():
    model = _constant(None)
    want = _loop(_act(model), 4)
    got = _launch(model._act_net(), 4)
    _same(got, want)
    _same(got, _constant_loop(0))                                 # the first maximum of four equal logits is action 0, throughout


@pytest.mark.parametrize("cap", [1, 7])
def test_cap_cuts_the_episodes(cap):
    model = _model(64)
    want = _loop(_act(model), 17, cap=cap)
    got = _launch(model._act_net(), 17, cap=cap)
    assert (got[1] == cap).all() and not got[2].any()
    _same(got, want)


def test_population_matches_single_launches_and_loops():
    from gymrl_amd.flat import flatten_module
    model = _model(64, seed=2)
    flat, _ = flatten_module(model, DEV)
    gen = torch.Generator(device="cpu").manual_seed(5)
    params = flat.detach().clone().unsqueeze(0).repeat(3, 1)
    params[1:] += (0.05 * torch.randn(2, flat.numel(), generator=gen)).to(DEV)
    net, E = model._act_net(), 17
    net.refresh()
    tight = ops.LunarPolicyStack(net, flat, params)
    padded = ops.LunarPolicyStack(net, flat, params, stride=tight.stride + 20)
    assert tight.stride % 4 == 0 and padded.stride == tight.stride + 20
    got_tight, got_padded = _launch(tight, E), _launch(padded, E)
    assert got_tight[0].shape == (3, E) and got_tight[3].shape == (3, E, 8)
    keep = flat.detach().clone()
    for p in range(3):
        flat.copy_(params[p])                                     # policy p as the network's own parameters
        want = _loop(_act(model), E)
        single = _launch(model._act_net(), E)
        _same(single, want)
        _same(tuple(x[p] for x in got_tight), want)
        _same(tuple(x[p] for x in got_padded), want)
    flat.copy_(keep)
    assert not np.array_equal(got_tight[0][0], got_tight[0][1])   # the perturbed policies do play other episodes


def test_two_launches_give_the_same_bits():
    model = _model(64)
    model.refresh_act()
    a, b = _launch(model._act_net(), 17), _launch(model._act_net(), 17)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    _same(a, _fresh(64, 17)[0])


# ---------------------------------------------------------------------------------------------------------------- mHC
def _full_config():
    from gymrl_amd.ppo_full_lunarlander import Config
    cfg = Config()
    cfg.mhc_layers, cfg.num_envs, cfg.update_freq, cfg.seed = 1, 16, 8, 3          # the smallest network the one-launch tile carries
    return cfg


@functools.lru_cache(maxsize=None)
def _full_trainer():
    from gymrl_amd.ppo_full_lunarlander import PPOTrainer
    return PPOTrainer(_full_config())


@pytest.mark.parametrize("E", [1, 17])
def test_mhc_policy_matches_the_loop(E):
    tr = _full_trainer()
    desc = tr._eval_desc()
    assert desc is not None and desc.n_sub == 2
    want = _loop(lambda obs: tr.model.forward_inference(obs)[0], E)
    got = tuple(t.cpu().numpy() for t in ops.lunar_mhc_eval(desc, E, SEED, STREAM0, device=tr.device))
    assert got[0].shape == (1, E)
    _same(got, want)
    again = tuple(t.cpu().numpy() for t in ops.lunar_mhc_eval(desc, E, SEED, STREAM0, device=tr.device))
    for x, y in zip(got, again):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------ trainers
def _untouched(tr, call):
    torch.cuda.synchronize()                                      # (the env's own side stream is still preparing spare worlds after a reset)
    before =(tr.step_count, tr.rollout_count, tr.env.state.clone(), tr.flat_params.clone())
    out = call()
    torch.cuda.synchronize()
    assert (tr.step_count, tr.rollout_count) == before[:2]
    assert torch.equal(tr.env.state, before[2]) and torch.equal(tr.flat_params, before[3])
    return out


def _ppo_trainer(hidden=64, fused_eval=True):
    from gymrl_amd.ppo_lunarlander import Config, PPOTrainer
    cfg = Config()
    cfg.num_envs, cfg.update_freq, cfg.hidden_dim, cfg.seed, cfg.fused_eval = 16, 8, hidden, 4, fused_eval
    return PPOTrainer(cfg)


def test_ppo_trainer_eval_is_the_act_forward_loop(capsys):
    tr = _ppo_trainer()
    tr.env.reset()
    got = _untouched(tr, lambda: tr.eval(5))
    assert "Evaluation Results: Mean = " in capsys.readouterr().out
    want = _loop(_act(tr.model), 5, seed=tr.base_seed + 1_000_003)
    assert got == [float(np.float32(r)) for r in want[0]]
    ret, length, term = _untouched(tr, lambda: tr.evaluate(5))
    assert ret.shape == (1, 5) and np.array_equal(ret[0], want[0]) and np.array_equal(length[0], want[1]) and np.array_equal(term[0], want[2])
    # a population through the trainer: the trainer's own vector twice is the same episodes twice, on shifted streams too
    stack = tr.flat_params.detach().clone().unsqueeze(0).repeat(2, 1)
    ret2, length2, _ = _untouched(tr, lambda: tr.evaluate(5, params=stack))
    assert np.array_equal(ret2[0], want[0]) and np.array_equal(ret2[1], want[0]) and np.array_equal(length2[1], want[1])
    shifted = tr.evaluate(3, stream_offset=2)
    assert np.array_equal(shifted[0][0], want[0][2:5])


def test_ppo_trainer_keeps_the_loop_for_a_network_the_forward_refuses():
    from gymrl_amd.nn import FusedMLP
    tr = _ppo_trainer(hidden=260)
    assert tr.model._act_net() is False and tr._eval_net() is None
    assert not FusedMLP.supported([(tr.model.shared[2], "tanh", 0, 1)], 8)
    off = _ppo_trainer(hidden=260, fused_eval=False)
    assert tr.eval(2) == off.eval(2)                              # the loop, whatever the switch says
    with pytest.raises(RuntimeError, match="gymrl_lunar_policy_eval"):
        tr.evaluate(2)


def test_ppo_full_trainer_eval_is_equal_on_and_off():
    tr = _full_trainer()
    tr.env.reset()
    assert tr.cfg.fused_eval is False
    off = _untouched(tr, lambda: tr.eval(5))
    tr.cfg.fused_eval = True
    try:
        on = _untouched(tr, lambda: tr.eval(5))
        ret, length, term = _untouched(tr, lambda: tr.evaluate(5))
    finally:
        tr.cfg.fused_eval = False
    assert on == off and len(on) == 5
    assert [float(np.float32(r)) for r in ret[0]] == off and (length >= 1).all()
    with pytest.raises(ValueError):
        tr.evaluate(5, params=tr.flat_params.view(1, -1))
