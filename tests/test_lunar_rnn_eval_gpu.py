"""Whole LunarLander-v3 evaluation episodes under the recurrent PPG / PPO-RNN network in ONE launch (csrc/eval_lunar_rnn.hip)
against the step loop they replace, bit for bit: lengths, terminated flags, terminal observations, the hidden state at the
episode's end, and returns (float64).

The loop is PPGTrainer.eval()'s: VecEnv("LunarLander-v3", E, seed, env_id0=stream_id0) stepped under
ops.mlprnn_act(deterministic=True, live=...) with ops.running_norm_masked(update=False) on the terminal observation; the first
episode of every env is kept and its float32 rewards are summed here in float64, in step order (the trainer's loop sums them in
float32, so its printed returns may differ from the launch's in the last place — its lengths and actions may not).

The statistics come from running_norm_masked(update=True) over 256 observation rows of a random-action rollout: fresh statistics
have std = 0 and would saturate the network.  Fresh policies end at their first crash, some tens to a few hundred steps."""
import functools

import numpy as np
import pytest
import torch

from gymrl_amd import ops

pytestmark = pytest.mark.gpu

SEED, STREAM0 = 11, 1 << 40
DEV = "cuda:0"
NAMES = ("returns", "lengths", "terminated", "terminal_obs", "h_final")


@functools.lru_cache(maxsize=None)
def _stats(seed=0):
    """RunningMeanStd.stats after 256 observation rows (16 envs x 16 steps under random actions)."""
    from gymrl_amd.envs import VecEnv
    env = VecEnv("LunarLander-v3", 16, device=DEV, seed=100 + seed, env_id0=0)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    obs, rew = env.reset(), torch.empty(16, device=DEV)
    rows = []
    for _ in range(16):
        rows.append(obs.clone())
        env.step(torch.randint(0, 4, (16,), generator=gen, dtype=torch.int32).to(DEV), obs, rew)
    env.close()
    stats = torch.zeros(26, dtype=torch.float64, device=DEV)
    ops.running_norm_masked(torch.cat(rows), torch.ones(256, dtype=torch.uint8, device=DEV), stats, update=True)
    assert stats[0].item() == 256 and (stats[18:24] > 0).all()     # (no leg touches the ground this early: their std stays 0)
    return stats


def _loop(params, E, stats, seed=SEED, stream_id0=STREAM0, cap=1000, zero_hidden=False):
    """-> ((returns f64[E], lengths i32[E], terminated u8[E], terminal_obs f32[E, 8], hidden f32[E, 64]), actions i32[T, E],
    rewards f32[T, E]) of the first episode of every env, cut at `cap`.  zero_hidden: the GRU state is zeroed before every step."""
    from gymrl_amd.envs import VecEnv
    env = VecEnv("LunarLander-v3", E, device=DEV, seed=seed, env_id0=stream_id0)
    raw, term = env.reset(), torch.empty(E, 8, device=DEV)
    rew = torch.empty(E, device=DEV)
    terminated, truncated = (torch.zeros(E, dtype=torch.uint8, device=DEV) for _ in range(2))
    live = torch.ones(E, dtype=torch.uint8, device=DEV)
    hidden = torch.zeros(E, 64, device=DEV)
    s = torch.empty(E, 8, device=DEV)
    act = torch.zeros(E, dtype=torch.int32, device=DEV)

    def observe(x):
        if stats is None:
            s.copy_(torch.where(live.bool().unsqueeze(1), x, s))
        else:
            ops.running_norm_masked(x, live, stats, update=False, out=s)

    observe(raw)
    rews, acts, dones, terms, tobs = [], [], [], [], []
    for t in range(cap):
        if zero_hidden:
            hidden.zero_()
        ops.mlprnn_act(s, hidden, params, 4, live=live, deterministic=True, h_out=hidden, act_out=act)
        env.step(act, raw, rew, term_obs_out=term, terminated_out=terminated, truncated_out=truncated)
        rews.append(rew.clone()), acts.append(act.clone()), dones.append((terminated | truncated).clone())
        terms.append(terminated.clone()), tobs.append(term.clone())
        live.mul_(1 - (terminated | truncated))
        observe(term)
        if t % 16 == 15 and not bool(live.any()):
            break
    env.close()
    rews, acts, dones, terms, tobs = (torch.stack(x).cpu().numpy() for x in (rews, acts, dones, terms, tobs))
    T = rews.shape[0]
    ret, length = np.zeros(E, np.float64), np.zeros(E, np.int32)
    term_flag, final = np.zeros(E, np.uint8), np.zeros((E, 8), np.float32)
    for e in range(E):
        hit = np.flatnonzero(dones[:, e])
        last = int(hit[0]) if hit.size else T - 1
        assert hit.size or T == cap                               # every episode ended, or was cut at the cap
        r = 0.0
        for t in range(last + 1):
            r = r + float(rews[t, e])
        ret[e], length[e], final[e] = r, last + 1, tobs[last, e]
        term_flag[e] = terms[last, e] if hit.size else 0
    return (ret, length, term_flag, final, hidden.cpu().numpy()), acts, rews


def _net(seed=0, ppg=True):
    """A freshly initialised network whose parameters are views of one flat buffer -> (net, flat)."""
    from gymrl_amd.flat import flatten_module
    from gymrl_amd.ppg_rnn_lunarlander import ActorCriticPPG
    from gymrl_amd.ppo_rnn_lunarlander import ActorCritic
    g = torch.random.get_rng_state()
    torch.manual_seed(seed)
    net = (ActorCriticPPG if ppg else ActorCritic)(8, 4)
    torch.random.set_rng_state(g)
    flat, _ = flatten_module(net, DEV)
    return net, flat


def _launch(policy, E, stats, **kw):
    out = ops.lunar_mlprnn_eval(policy, E, kw.pop("seed", SEED), kw.pop("stream_id0", STREAM0), norm_stats=stats,
                                want_h_final=True, **kw)
    return tuple(t.cpu().numpy() for t in out)


def _same(got, want):
    """got: the launch's [P, E] arrays for P == 1, or one policy's rows; want: the loop's."""
    assert len(got) == len(want) == 5
    for g, w, name in zip(got, want, NAMES):
        g = g[0] if g.ndim == w.ndim + 1 else g
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, g, w)


@functools.lru_cache(maxsize=None)
def _fresh(E, normed):
    """A fresh ActorCriticPPG's loop and launch at E episodes, with the statistics or on raw observations, computed once."""
    net, _ = _net()
    params = ops.mlprnn_params(net)
    stats = _stats() if normed else None
    want, acts, _ = _loop(params, E, stats)
    got = _launch(params, E, stats)
    return want, got, acts


@pytest.mark.parametrize("normed", [True, False], ids=["stats", "raw"])
@pytest.mark.parametrize("E", [1, 16, 17])
def test_fresh_policy_matches_the_loop(E, normed):
    want, got, _ = _fresh(E, normed)
    assert got[0].shape == (1, E) and got[0].dtype == np.float64 and got[3].shape == (1, E, 8) and got[4].shape == (1, E, 64)
    _same(got, want)
    assert want[1].min() >= 1


def test_quads_of_one_workgroup_end_at_different_steps():
    want, got, _ = _fresh(16, True)
    assert len(set(want[1].tolist())) >= 2                        # a quad idles while its neighbours step
    _same(got, want)


def test_the_hidden_state_is_on_the_way_to_the_actions():
    """The equalities above are not those of a feed-forward policy: with the GRU state zeroed before every step the loop plays
    other actions somewhere (seed 11, 17 episodes), and the state the launch hands back is not the zero it started from."""
    want, got, acts = _fresh(17, True)
    net, _ = _net()
    amnesic, acts0, _ = _loop(ops.mlprnn_params(net), 17, _stats(), zero_hidden=True)
    differs = False
    for e in range(17):
        n, n0 = int(want[1][e]), int(amnesic[1][e])
        differs |= n != n0 or not np.array_equal(acts[:n, e], acts0[:n0, e])   # (another length: another action before it)
    assert differs
    assert np.abs(got[4]).max() > 0 and (np.abs(got[4][0]).max(axis=1) > 0).all()
    _same(got, want)


@functools.lru_cache(maxsize=None)                             # (kept alive: a parameter table holds raw pointers)
def _constant(k):
    """The policy that always takes action k (None: four equal logits): actor_fc's last weight zero, a one-hot bias."""
    net, _ = _net(seed=1)
    with torch.no_grad():
        net.actor_fc.mlp[2].weight.zero_()
        net.actor_fc.mlp[2].bias.zero_()
        if k is not None:
            net.actor_fc.mlp[2].bias[k] = 1.0
    return net


@functools.lru_cache(maxsize=None)
def _constant_loop(k):
    want, acts, _ = _loop(ops.mlprnn_params(_constant(k)), 4, _stats())
    for e in range(4):
        assert (acts[:want[1][e], e] == k).all()
    return want


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_constant_action(k):
    """No-op, both side engines and the main engine: each drives the solver through its contacts to the end of the episode."""
    _same(_launch(ops.mlprnn_params(_constant(k)), 4, _stats()), _constant_loop(k))


def test_equal_logits_take_the_first_action():
    net = _constant(None)
    want, _, _ = _loop(ops.mlprnn_params(net), 4, _stats())
    got = _launch(ops.mlprnn_params(net), 4, _stats())
    _same(got, want)
    for g, w in zip(got[:4], _constant_loop(0)[:4]):              # the first maximum of four equal probabilities is action 0,
        assert np.array_equal(g[0], w)                            # throughout (the hidden state is another network's)


@pytest.mark.parametrize("cap", [1, 7])
def test_cap_cuts_the_episodes(cap):
    net, _ = _net()
    params = ops.mlprnn_params(net)
    want, _, _ = _loop(params, 17, _stats(), cap=cap)
    got = _launch(params, 17, _stats(), cap=cap)
    assert (got[1] == cap).all() and not got[2].any()
    _same(got, want)


@pytest.mark.parametrize("shared", [False, True], ids=["own_stats", "shared_stats"])
def test_population_matches_single_launches_and_loops(shared):
    net, flat = _net(seed=2)
    gen = torch.Generator(device="cpu").manual_seed(5)
    params = flat.detach().clone().unsqueeze(0).repeat(3, 1)
    params[1:] += (0.05 * torch.randn(2, flat.numel(), generator=gen)).to(DEV)
    stats = _stats() if shared else torch.stack([_stats(p) for p in range(3)])
    E, n = 17, flat.numel()
    tight = ops.MlprnnPolicyStack(net, flat, params, norm_stats=stats)
    padded = ops.MlprnnPolicyStack(net, flat, params, norm_stats=stats, stride=tight.stride + 20)
    assert tight.stride == (n + 3) // 4 * 4 and padded.stride == tight.stride + 20
    got_tight, got_padded = _launch(tight, E, None), _launch(padded, E, None)    # (None: the stack's own statistics)
    assert got_tight[0].shape == (3, E) and got_tight[3].shape == (3, E, 8) and got_tight[4].shape == (3, E, 64)
    keep = flat.detach().clone()
    own = ops.mlprnn_params(net)
    for p in range(3):
        flat.copy_(params[p])                                     # policy p as the network's own parameters
        sp = stats if shared else stats[p].contiguous()
        want, _, _ = _loop(own, E, sp)
        _same(_launch(own, E, sp), want)
        _same(tuple(x[p] for x in got_tight), want)
        _same(tuple(x[p] for x in got_padded), want)
    flat.copy_(keep)
    assert not np.array_equal(got_tight[0][0], got_tight[0][1])   # the perturbed policies do play other episodes


def test_two_launches_give_the_same_bits():
    net, _ = _net()
    params = ops.mlprnn_params(net)
    a, b = _launch(params, 17, _stats()), _launch(params, 17, _stats())
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    _same(a, _fresh(17, True)[0])


# ------------------------------------------------------------------------------------------------------------ trainers
def _trainer(tmp_path, ppg):
    from gymrl_amd import ppg_rnn_lunarlander, ppo_rnn_lunarlander
    mod = ppg_rnn_lunarlander if ppg else ppo_rnn_lunarlander
    cfg = mod.Config()
    assert cfg.fused_eval is False                                # off unless asked for
    cfg.seed, cfg.save_path = 4, str(tmp_path / "ck.pth")
    tr = (mod.PPGTrainer if ppg else mod.PPORNNTrainer)(cfg)
    tr.state_norm.running_ms.stats.copy_(_stats())                # (as after 256 training steps)
    tr.net.rnn_h = torch.full((3, 64), 0.5, device=tr.device)     # a single-env caller's carried state: not eval's business
    return tr


def _untouched(tr, call):
    torch.cuda.synchronize()
    h = tr.net.rnn_h
    before = (tr.round_count, tr.learn_step, tr.flat_params.clone(), tr.state_norm.running_ms.stats.clone(),
              tr.reward_scaler.running_ms.stats.clone(), h.clone(), tr.optimizer.m.clone(), len(tr._batch))
    out = call()
    torch.cuda.synchronize()
    assert (tr.round_count, tr.learn_step, len(tr._batch)) == (before[0], before[1], before[7])
    assert torch.equal(tr.flat_params, before[2]) and torch.equal(tr.state_norm.running_ms.stats, before[3])
    assert torch.equal(tr.reward_scaler.running_ms.stats, before[4]) and torch.equal(tr.optimizer.m, before[6])
    assert tr.net.rnn_h is h and torch.equal(h, before[5])
    return out


@pytest.mark.parametrize("ppg", [False, True], ids=["PPORNNTrainer", "PPGTrainer"])
def test_trainer_eval_and_evaluate_are_the_loop(tmp_path, capsys, ppg):
    tr = _trainer(tmp_path, ppg)
    stats = tr.state_norm.running_ms.stats
    want, _, rews = _loop(tr._act_params, 5, stats, seed=tr.base_seed + 1_000_003)
    off = _untouched(tr, lambda: tr.eval(5))                      # the step loop, float32 sums
    tr.cfg.fused_eval = True
    capsys.readouterr()
    on = _untouched(tr, lambda: tr.eval(5))
    out = capsys.readouterr().out
    assert "Evaluating for 5 episodes" in out and "  Episode 5: Reward = " in out and "Evaluation: Mean = " in out
    assert on == [float(np.float32(r)) for r in want[0]]
    # against the loop's float32 sums: a sum of n float32 terms is off by at most n * 2^-24 * sum |r_t|
    for e in range(5):
        n = int(want[1][e])
        assert abs(on[e] - off[e]) <= (n + 1) * 2.0 ** -24 * float(np.abs(rews[:n, e].astype(np.float64)).sum())
    ret, length, term = _untouched(tr, lambda: tr.evaluate(5))
    assert ret.shape == (1, 5) and ret.dtype == np.float64
    assert np.array_equal(length[0], want[1]) and np.array_equal(ret[0], want[0]) and np.array_equal(term[0], want[2])
    # a population through the trainer: the trainer's own vector twice is the same episodes twice, on shifted streams too
    stack = tr.flat_params.detach().clone().unsqueeze(0).repeat(2, 1)
    ret2, length2, _ = _untouched(tr, lambda: tr.evaluate(5, params=stack))
    assert np.array_equal(ret2[0], want[0]) and np.array_equal(ret2[1], want[0]) and np.array_equal(length2[1], want[1])
    shifted = tr.evaluate(3, stream_offset=2)
    assert np.array_equal(shifted[1][0], want[1][2:5]) and np.array_equal(shifted[0][0], want[0][2:5])
    other = tr.evaluate(5, norm_stats=_stats(1))                  # other statistics: the loop under them
    assert np.array_equal(other[1][0], _loop(tr._act_params, 5, _stats(1), seed=tr.base_seed + 1_000_003)[0][1])
