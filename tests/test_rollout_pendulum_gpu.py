"""gymrl_rollout_pendulum and gymrl_pendulum_ppo_eval on an MI355X against the step loop act_forward (gymrl_mlp_forward) ->
gymrl_gaussian_sample -> gymrl_env_step (-> reward * reward_scale).  Every comparison is torch.equal.

Pendulum-v1 ends at the TimeLimit only, so after the reset a few envs get an episode length close to 200 written into the state
buffer (the SoA layout of include/gymrl.h: float64 th, thd, ep_ret, then int32 ep_len, every [n] field padded to 256 bytes): the
window then holds truncations with their auto-reset, one of them on its last step."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED, ID0, GAMMA, LAM = 17, 1 << 33, 0.95, 0.9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from gymrl_amd import ops
    assert ops.device_ok(), "libgymrl_hip.so did not find a gfx950 device"
    return torch.device("cuda:0")


def _model(hidden, dev, seed=3, log_std=-0.4):
    from gymrl_amd.ppo_pendulum import GaussianActorCritic
    torch.manual_seed(seed)
    m = GaussianActorCritic(3, 1, hidden, log_std).to(dev)
    with torch.no_grad():
        m.actor[2].weight.mul_(60.0)                       # the 0.01-gain head would keep every torque inside +-2: let some be clipped
    m.refresh_act()
    return m


def _slabs(N, T, dev):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)   # noqa: E731
    return dict(obs=z(T + 1, N, 3), act=z(T, N), logp=z(T, N), val=z(T, N), rew=z(T, N), done=z(T, N, dt=torch.uint8),
                ep_ret=z(T, N), next_value=z(N), running=z(2, N, dt=torch.float64))


def _start(N, T, dev):
    """A reset env with planted episode lengths: env 0 truncates on the window's last step, env 1 and the last env inside it."""
    from gymrl_amd.envs import VecEnv
    env = VecEnv("Pendulum-v1", N, device=dev, seed=SEED, env_id0=ID0)
    obs0 = env.reset()
    len_at = 3 * ((N * 8 + 255) & ~255)
    lens = env.state[len_at:len_at + 4 * N].view(torch.int32)
    lens[0] = 200 - T
    if N > 1:
        lens[1], lens[N - 1] = 197, 195
    return env, obs0


def _step_loop(model, N, T, scale, noise, dev):
    from gymrl_amd import ops
    env, obs0 = _start(N, T, dev)
    s = _slabs(N, T, dev)
    ws = ops.gae_workspace(T, N, dev)
    ws.zero_()
    s["obs"][0].copy_(obs0)
    scale_t = torch.tensor(scale, dtype=torch.float32, device=dev)
    ls = model.log_std.detach()
    fuse = N % 4 == 0
    stage = torch.empty(N, 3, device=dev)
    for t in range(T):
        mu, value = model.act_forward(s["obs"][t].clone(), refresh=False)
        on = ops.gae_online(s["rew"][t - 1], s["done"][t - 1], s["val"][t - 1], s["running"], ws, t - 1, T, GAMMA, LAM) if fuse and t else None
        ops.gaussian_sample(mu, ls, value=value.view(-1), noise_normal=None if noise is None else noise[t], seed=env.seed, counter=100 + t,
                            env_id0=ID0, act_out=s["act"][t].view(N, 1), logp_out=s["logp"][t], value_out=s["val"][t], online=on)
        env.step(s["act"][t], stage, s["rew"][t], done_out=s["done"][t], ep_ret_out=s["ep_ret"][t])
        s["obs"][t + 1].copy_(stage)                       # gymrl_env_step stores 16-byte aligned rows: a slab row is one only when 4 | N
        torch.mul(s["rew"][t], scale_t, out=s["rew"][t])
    s["next_value"].copy_(model.act_forward(s["obs"][T].clone(), refresh=False)[1].view(-1))
    if fuse:
        ops.gae_online_flush(ops.gae_online(s["rew"][T - 1], s["done"][T - 1], s["val"][T - 1], s["running"], ws, T - 1, T, GAMMA, LAM),
                             s["next_value"])
    return env, s, ws


def _one_launch(model, N, T, scale, noise, dev, windows):
    from gymrl_amd import ops
    env, obs0 = _start(N, T, dev)
    s = _slabs(N, T, dev)
    ws = ops.gae_workspace(T, N, dev)
    ws.zero_()
    s["obs"][0].copy_(obs0)
    fuse = N % 4 == 0
    desc = model._act_net().descriptor(N, dev)
    for t0, n in windows:
        ops.rollout_pendulum(env.state, N, env.seed, ID0, 100, s["obs"], s["act"], s["logp"], s["val"], s["rew"], s["done"], s["ep_ret"],
                             s["next_value"], desc, model.log_std.detach(), T, t0, n, GAMMA, LAM, reward_scale=scale, noise_normal=noise,
                             gae_running=s["running"] if fuse else None, gae_workspace=ws if fuse else None, ep_stats=env.ep_stats)
    return env, s, ws


def _assert_same(a, b, N):
    (env_a, sa, ws_a), (env_b, sb, ws_b) = a, b
    for name in ("obs", "act", "logp", "val", "rew", "done", "next_value"):
        assert torch.equal(sa[name], sb[name]), name
    d = sa["done"].bool()
    assert torch.equal(sa["ep_ret"][d], sb["ep_ret"][d])
    assert torch.equal(env_a.state, env_b.state) and torch.equal(env_a.ep_stats, env_b.ep_stats)
    if N % 4 == 0:
        assert torch.equal(ws_a, ws_b) and torch.equal(sa["running"], sb["running"])


# (1, 64, 18): one env; (17, 64, 33): a ragged second workgroup, three GAE chunks; (40, 256, 18): the 256-wide forward, online GAE
@pytest.mark.parametrize("N,hidden,T,scale,explicit", [(1, 64, 18, 0.1, False), (17, 64, 33, 0.1, False), (17, 64, 33, 1.0, True),
                                                       (40, 256, 18, 0.1, False), (40, 64, 33, 1.0, False)])
def test_one_launch_equals_the_step_loop(dev, N, hidden, T, scale, explicit):
    model = _model(hidden, dev)
    noise = torch.randn(T, N, 1, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) if explicit else None
    want = _step_loop(model, N, T, scale, noise, dev)
    got = _one_launch(model, N, T, scale, noise, dev, [(0, T)])
    _assert_same(got, want, N)
    s, env = want[1], want[0]
    done = s["done"].cpu().numpy().astype(bool)
    assert done[T - 1, 0] and done[:T - 1, 0].sum() == 0                   # a truncation on the window's last step
    if N > 1:
        assert done[2, 1] and done[4, N - 1] and int(env.ep_stats[0]) == 3  # and two inside it, each followed by an auto-reset
        assert (s["act"].abs() > 2.0).any()                                 # the slab holds the UNCLIPPED draw
    r = s["rew"].cpu().numpy()
    assert (r <= 0).all() and r.min() >= -16.2736044 * scale - 1e-6         # max cost pi^2 + 0.1 * 64 + 0.001 * 4
    split = _one_launch(model, N, T, scale, noise, dev, [(0, 7), (7, T - 7)])
    _assert_same(split, want, N)


# ---------------------------------------------------------------- evaluation ----
E_MAX, EVAL_ID0 = 33, (1 << 40) + 3


def _eval_loop(model, dev, seed, caps=(7, 200)):
    """-> cap -> (returns f64, lengths, final_obs) of the first episode of envs EVAL_ID0 .. + E_MAX - 1 under a = mu, cut at cap.  The
    float64 return is the stepper's own running sum, read from the state buffer; at the TimeLimit the stepper has reset it, and the
    float32 ep_ret_out (its rounding) is what is left to compare."""
    from gymrl_amd.envs import VecEnv
    env = VecEnv("Pendulum-v1", E_MAX, device=dev, seed=seed, env_id0=EVAL_ID0)
    obs = env.reset()
    nxt, tobs = torch.empty_like(obs), torch.empty_like(obs)
    rew, ep_ret = torch.empty(E_MAX, device=dev), torch.zeros(E_MAX, device=dev)
    done = torch.zeros(E_MAX, dtype=torch.uint8, device=dev)
    ret_at = 2 * ((E_MAX * 8 + 255) & ~255)
    out = {}
    for t in range(200):
        act, _, _ = model.get_action(obs, deterministic=True)
        env.step(act, nxt, rew, done_out=done, term_obs_out=tobs, ep_ret_out=ep_ret)
        obs, nxt = nxt, obs
        if t + 1 in caps:
            full = t + 1 == 200
            ret64 = env.state[ret_at:ret_at + 8 * E_MAX].view(torch.float64).clone()
            out[t + 1] = (ep_ret.clone() if full else ret64, tobs.clone(), bool(done.all()) if full else not bool(done.any()))
    return out


@pytest.fixture(scope="module")
def eval_refs(dev):
    models = [_model(64, dev, seed=s) for s in (3, 4, 5)]
    return models, [_eval_loop(m, dev, 23) for m in models]


@pytest.mark.parametrize("cap", [200, 7])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("E", [1, 10, 33])
def test_eval_equals_the_step_loop(dev, eval_refs, E, P, cap):
    from gymrl_amd import ops
    from gymrl_amd.flat import flatten_module
    models, refs = eval_refs
    if P == 1:
        policy = models[0]._act_net()
    else:                                                  # a population: three parameter vectors through one network's layout
        from gymrl_amd.ppo_pendulum import GaussianActorCritic
        host = GaussianActorCritic(3, 1, 64)
        flat, _ = flatten_module(host, dev)
        rows = []
        for m in models:
            host.load_state_dict(m.state_dict())
            rows.append(flat.clone())
        policy = ops.LunarPolicyStack(host._act_net(), flat, torch.stack(rows))
    ret, length, termd, fin = ops.pendulum_ppo_eval(policy, E, 23, EVAL_ID0, cap=cap, want_final_obs=True)
    assert ret.dtype == torch.float64 and ret.shape == (P, E) and fin.shape == (P, E, 3)
    assert (length == cap).all() and not termd.any()       # Pendulum never terminates: every episode runs to the cap
    for p in range(P):
        want_ret, want_obs, as_expected = refs[p][cap]
        assert as_expected
        if cap == 200:
            assert torch.equal(ret[p].to(torch.float32), want_ret[:E])      # the stepper's float32 ep_ret_out
        else:
            assert torch.equal(ret[p], want_ret[:E])                        # the stepper's float64 running return, bit for bit
        assert torch.equal(fin[p], want_obs[:E])
    if P == 3:                                             # a stack equals P single launches
        for p, m in enumerate(models):
            one = ops.pendulum_ppo_eval(m._act_net(), E, 23, EVAL_ID0, cap=cap, want_final_obs=True)
            assert torch.equal(one[0][0], ret[p]) and torch.equal(one[3][0], fin[p])
        assert not torch.equal(ret[0], ret[1])
