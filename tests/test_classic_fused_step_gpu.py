"""The fused DQN, DDQN + PER (non-dueling) and discrete-SAC vector steps on MountainCar-v0 and Acrobot-v1
(gymrl_dqn_act_step_classic / gymrl_dsac_act_step_classic: csrc/dqn_step.hip, csrc/dsac_step.hip, classic_act_tail of
csrc/slab_step_device.hpp) against the layer-by-layer path: the same draws -> actions, observations, rewards, dones, the replay
ring, the env state buffer, every parameter, Adam moment, target, loss sum and host counter equal BIT FOR BIT (torch.equal).

Random play on these two envs ends at the TimeLimit only, so every env.reset() is followed by the same few writes into both
trainers' state buffers (the SoA layout of include/gymrl.h), the way tests/test_rollout_classic_gpu.py plants them: env 0 and the
last env (the ragged workgroup's) start where the next step terminates — MountainCar (0.45, 0.06) crosses 0.5 under any action,
Acrobot (3.0, 0, 0, 0) is above the line after one step —, env 1 starts three steps in front of the TimeLimit."""
import numpy as np
import pytest

import acrobot_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# name -> (TimeLimit, float64 state fields in front of ep_ret, the planted state, its float32 observation)
ENVS = {
    "MountainCar-v0": (200, 2, (0.45, 0.06), lambda y: np.asarray(y, np.float64).astype(np.float32)),
    "Acrobot-v1": (500, 4, (3.0, 0.0, 0.0, 0.0), acrobot_ref.obs_of),
}
ENV_NAMES = list(ENVS)
ACT_ENTRIES = ("gymrl_dqn_act_step", "gymrl_dqn_act_step_classic", "gymrl_ddqn_duel_act_step", "gymrl_dsac_act_step",
               "gymrl_dsac_act_step_classic", "gymrl_ndqn_act_step", "gymrl_rainbow_act_step")


# ---- planted episode ends ---------------------------------------------------------------------------------------------------
def _pitch(n):
    return (n * 8 + 255) & ~255                                             # every [n] field is padded to 256 bytes


def _plant_start(env, obs, i):
    """Env i stands where the next step terminates: its state fields and its observation row."""
    _, _, start, obs_of = ENVS[env.name]
    pitch = _pitch(env.n)
    for k, v in enumerate(start):
        env.state[k * pitch + 8 * i:k * pitch + 8 * i + 8].view(torch.float64).fill_(v)
    obs[i].copy_(torch.from_numpy(obs_of(start)).to(env.device))


def _plant_len(env, i):
    """Env i is three steps in front of the TimeLimit (its observation does not carry the length)."""
    cap, n_state, _, _ = ENVS[env.name]
    len_at = (n_state + 1) * _pitch(env.n)                                  # ep_len i32[n] follows the state fields and ep_ret
    env.state[len_at + 4 * i:len_at + 4 * i + 4].view(torch.int32).fill_(cap - 3)


def _plant(env, obs):
    n = env.n
    for i in {0, n - 1}:
        _plant_start(env, obs, i)
    if n > 2:
        _plant_len(env, 1)


def _plant_after_reset(tr):
    """Every env.reset() of the trainer is followed by the planted starts."""
    env, reset = tr.env, tr.env.reset

    def reset_and_plant(obs_out=None, seed=None):
        out = reset(obs_out, seed=seed)
        _plant(env, out)
        return out
    env.reset = reset_and_plant


def _truncated(env, tobs, rew, done):
    """Which of the finished episodes the TimeLimit ended: Acrobot pays 0 on the terminating step only; MountainCar terminates
    at position >= 0.5, which the terminal observation shows."""
    if env.name == "Acrobot-v1":
        return done.bool() & (rew == -1.0)
    return done.bool() & (tobs[:, 0] < 0.5)


# ---- trainers ---------------------------------------------------------------------------------------------------------------
def _trainer(algo, env_name, N, B, hidden, fused, graphs=None, seed=5, plant=True, **more):
    from gymrl_amd import ddqn_per_cartpole, ddqn_per_duel_cartpole, dqn_cartpole, noisy_dqn_cartpole, rainbow_dqn_cartpole, sac_cartpole
    mod, cls = {"dqn": (dqn_cartpole, "DQNTrainer"), "ddqn_per": (ddqn_per_cartpole, "DDQNPERTrainer"),
                "ddqn_duel": (ddqn_per_cartpole, ddqn_per_duel_cartpole.DDQNPERDuelTrainer), "dsac": (sac_cartpole, "SACTrainer"),
                "ndqn": (noisy_dqn_cartpole, "NoisyDQNTrainer"), "rainbow": (rainbow_dqn_cartpole, "RainbowDQNTrainer")}[algo]
    cfg = mod.Config()
    cfg.env_name = env_name
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed = N, B, hidden, seed
    cfg.max_episodes, cfg.memory_capacity = 10 ** 9, max(4096, 4 * B)
    cfg.fused_step = fused
    if algo == "dsac":
        cfg.kernel_softmax = True                     # the layer path's softmax through csrc/softmax_device.hpp: the fused step's bits
    if graphs is not None:
        cfg.use_graphs = graphs
    for k, v in more.items():
        setattr(cfg, k, v)
    tr = (getattr(mod, cls) if isinstance(cls, str) else cls)(cfg)
    assert tr.env.name == env_name and tr.env.max_steps == ENVS[env_name][0] and tr.action_dim == 3
    if plant:
        _plant_after_reset(tr)
    return tr


def _uniforms(N, steps, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.rand(N, 2, generator=g, device="cuda") for _ in range(steps)]


def _strata(B, steps, seed=11):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.rand(B, generator=g, device="cuda", dtype=torch.float64) for _ in range(steps)]


def _exp_draws(N, A, steps, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.empty(N, A, device="cuda").exponential_(generator=g) for _ in range(steps)]


def _feed(tr, algo, N, B, steps):
    """Explicit draws through the trainers' parity hooks (otherwise the kernels' own Philox)."""
    if algo == "dsac":
        tr._parity_noise = iter(_exp_draws(N, tr.action_dim, steps))
    else:
        tr._parity_u = iter(_uniforms(N, steps))
        if algo == "ddqn_per":
            tr._parity_v = iter(_strata(B, steps))


def _assert_same(algo, a, b, what=""):
    assert (a.memory.cursor, a.memory.size, a.memory.draws) == (b.memory.cursor, b.memory.size, b.memory.draws), what
    for k, (x, y) in enumerate(zip(a.memory.ring, b.memory.ring)):
        assert torch.equal(x, y), (what, "ring", k)          # acting: same actions, same physics, same rows
    assert torch.equal(a.env.state, b.env.state), (what, "env state")
    if algo == "dsac":
        opts = ("actor_optim", "critic1_optim", "critic2_optim")
        for opt in opts:
            assert getattr(a, opt).step_count == getattr(b, opt).step_count, (what, opt)
        assert (a._act_counter, a._alpha_steps) == (b._act_counter, b._alpha_steps), what
        for name in ("actor_flat", "c1_flat", "c2_flat", "c1_target_flat", "c2_target_flat"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
        for opt in opts:
            assert torch.equal(getattr(a, opt).m, getattr(b, opt).m) and torch.equal(getattr(a, opt).v, getattr(b, opt).v), (what, opt)
        for name in ("log_alpha", "_alpha_m", "_alpha_v", "_sums_c", "_sums_a", "_alpha_loss"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (what, name, getattr(a, name), getattr(b, name))
    else:
        assert a.optimizer.step_count == b.optimizer.step_count, what
        assert (a._act_counter, a.sample_count, a.epsilon) == (b._act_counter, b.sample_count, b.epsilon), what
        if algo == "ddqn_per":
            assert a.cfg.beta == b.cfg.beta, what
            assert torch.equal(a.memory.tree.tree, b.memory.tree.tree), (what, "tree")
        for name in ("flat_params", "target_flat", "_loss"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (what, name, getattr(a, name), getattr(b, name))
        assert torch.equal(a.optimizer.m, b.optimizer.m) and torch.equal(a.optimizer.v, b.optimizer.v), what
    assert list(a.episode_rewards) == list(b.episode_rewards), what


def _steps_taken(tr, algo):
    return tr.actor_optim.step_count if algo == "dsac" else tr.optimizer.step_count


# ---- 1. the act launch against the kernels composed by hand -------------------------------------------------------------------
# (N = 40, 17: a ragged last workgroup; 36: no weight image, no 16-column alignment; N = 1: the scalar surface's; 256 x 256: sixteen
#  workgroups of the instance built for that width)
ACT_SHAPES = [(40, 64, 24), (17, 36, 18), (1, 32, 12), (256, 256, 12)]


def _first_max(q):
    best = q.max(dim=1).values
    return torch.where(q[:, 0] == best, 0, torch.where(q[:, 1] == best, 1, 2))


@pytest.mark.parametrize("N,hidden,steps", ACT_SHAPES)
@pytest.mark.parametrize("env_name", ENV_NAMES)
@pytest.mark.parametrize("algo", ["dqn", "dsac"])
def test_act_launch_equals_the_kernels_composed_by_hand(algo, env_name, N, hidden, steps):
    """One launch against policy_net / actor.logits (gymrl_lin_fwd) -> ops.epsilon_greedy / ops.categorical_sample -> env.step ->
    memory.push, step by step, explicit draws and the kernels' own Philox in turn.  DQN with A = 3: epsilon = 0 (greedy whatever
    u0), epsilon = 1 (explore whatever u0), u1 = 0.99999994 (the largest float32 below one: action A - 1 = 2, never 3),
    u0 == epsilon exactly (`u0 < epsilon` is false: greedy), one ulp below it (explores); over the last six steps the last layer is
    zero: equal Q values, and the first maximum is action 0.  N = 1 has one env to plant into: it starts at the terminating state,
    is put three steps in front of the TimeLimit at step 3 and back at the terminating state at step 8."""
    from gymrl_amd import ops
    B = 64
    a, b = _trainer(algo, env_name, N, B, hidden, False, plant=False), _trainer(algo, env_name, N, B, hidden, True, plant=False)
    assert b._fused_ok() and not a._fused_ok()
    dev, D, A = a.device, a.env.obs_dim, a.action_dim
    assert A == 3 and D == {"MountainCar-v0": 2, "Acrobot-v1": 6}[env_name]
    draws = _uniforms(N, steps, seed=3) if algo == "dqn" else _exp_draws(N, A, steps, seed=3)
    obs_a, obs_b = a.env.reset(), torch.empty(N, D, device=dev)
    b.env.reset(obs_b)
    assert torch.equal(obs_a, obs_b)
    _plant(a.env, obs_a), _plant(b.env, obs_b)
    nxt_a, tobs, nxt_b = (torch.empty(N, D, device=dev) for _ in range(3))
    rew_a, rew_b = torch.empty(N, device=dev), torch.empty(N, device=dev)
    done_a, done_b = (torch.zeros(N, dtype=torch.uint8, device=dev) for _ in range(2))
    ret_a, ret_b = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    act_b = torch.empty(N, dtype=torch.int32, device=dev)
    eps_cycle = (0.0, 0.5, 1.0, 0.25, 0.9, 0.05)
    ends, truncations, seen = 0, 0, set()
    for t in range(steps):
        if N == 1 and t == 3:
            _plant_len(a.env, 0), _plant_len(b.env, 0)
        if N == 1 and t == 8:
            _plant_start(a.env, obs_a, 0), _plant_start(b.env, obs_b, 0)
        args = b._fused_args()[0]
        if algo == "dqn":
            eps = eps_cycle[t % len(eps_cycle)]
            u = draws[t].clone() if (t % 2 == 0 or eps in (0.0, 1.0)) else None          # explicit / Philox
            if u is not None:
                u[0::5, 1] = 0.99999994
                if 0.0 < eps < 1.0:
                    u[1::5, 0] = float(np.float32(eps))                # u0 == epsilon: not below it, greedy
                    u[2::5, 0] = float(np.nextafter(np.float32(eps), np.float32(0.0)))   # one ulp below: explores
            if t == steps - 6:                                         # equal Q values from here on
                for tr in (a, b):
                    with torch.no_grad():
                        tr.policy_net.net[4].weight.zero_()
                        tr.policy_net.net[4].bias.zero_()
                args = b._fused_args()[0]
            with torch.no_grad():
                q = a.policy_net(obs_a)
            act_a = ops.epsilon_greedy(q, eps, u=u, seed=a.base_seed, counter=t + 1, env_id0=a.env.env_id0)
            if u is not None and eps == 0.0:                           # greedy: the first maximum, whatever u says
                assert torch.equal(act_a.long(), _first_max(q))
                seen.add("greedy")
            if u is not None and eps == 1.0:                           # explore: (int)(u1 * A), clamped
                assert torch.equal(act_a.long(), (u[:, 1] * 3.0).long().clamp(max=2))
                assert bool((act_a[0::5] == 2).all())
                seen.add("explore")
            if u is not None and 0.0 < eps < 1.0:
                rows = torch.arange(N, device=dev)[1::5]
                assert torch.equal(act_a[rows].long(), _first_max(q[rows]))                          # u0 == eps is greedy
                rows = torch.arange(N, device=dev)[2::5]
                assert torch.equal(act_a[rows].long(), (u[rows, 1] * 3.0).long().clamp(max=2))       # one ulp below explores
                seen.add("edge")
            if t >= steps - 6 and eps == 0.0:
                assert bool((q == 0).all()) and bool((act_a == 0).all())
                seen.add("equal-q")
        else:
            noise = draws[t] if t % 2 == 0 else None                   # explicit / Philox
            with torch.no_grad():
                logits = a.actor.logits(obs_a)
            act_a, _, _, _ = ops.categorical_sample(logits, noise_exp=noise, seed=a.base_seed, counter=t + 1, env_id0=a.env.env_id0)
        a.env.step(act_a, nxt_a, rew_a, done_out=done_a, term_obs_out=tobs, ep_ret_out=ret_a)
        a.memory.push(obs_a, act_a, rew_a, tobs, done_a)
        if algo == "dqn":
            ops.dqn_act_step(args, b.env, obs_b, nxt_b, epsilon=eps, cursor=b.memory.cursor, u=u, seed=b.base_seed, counter=t + 1,
                             action_out=act_b, rew_out=rew_b, done_out=done_b, ep_ret_out=ret_b)
        else:
            ops.dsac_act_step(args, b.env, obs_b, nxt_b, cursor=b.memory.cursor, noise_exp=noise, seed=b.base_seed, counter=t + 1,
                              action_out=act_b, rew_out=rew_b, done_out=done_b, ep_ret_out=ret_b)
        b.memory.advance(N)
        assert bool(((act_a >= 0) & (act_a < 3)).all())
        assert torch.equal(act_a, act_b) and torch.equal(nxt_a, nxt_b) and torch.equal(rew_a, rew_b) and torch.equal(done_a, done_b), t
        assert torch.equal(ret_a, ret_b), t
        assert (a.memory.cursor, a.memory.size) == (b.memory.cursor, b.memory.size)
        for k, (x, y) in enumerate(zip(a.memory.ring, b.memory.ring)):
            assert torch.equal(x, y), (t, "ring", k)
        assert torch.equal(a.env.state, b.env.state), t
        ends += int(done_a.sum().item())
        truncations += int(_truncated(a.env, tobs, rew_a, done_a).sum().item())
        obs_a, nxt_a = nxt_a, obs_a
        obs_b, nxt_b = nxt_b, obs_b
    print("episode ends:", ends, "of them truncations:", truncations)
    if algo == "dqn":
        assert seen == {"greedy", "explore", "edge", "equal-q"}
    assert ends >= 3 and 1 <= truncations < ends


# ---- 2. train() fused against layer by layer ------------------------------------------------------------------------------------
# (B = 24 / 100 / 250: a partial last slab; hidden 36: no images; 256: the instances built for that width)
TRAIN_SHAPES = [(20, 24, 32, 14), (33, 100, 36, 16), (17, 250, 256, 28)]


def _run(algo, env_name, fused, steps, N, B, hidden, explicit, graphs=None):
    tr = _trainer(algo, env_name, N, B, hidden, fused, graphs=graphs)
    assert bool(tr._fused_ok()) == fused               # on the parent the fused trainer's is False on these envs
    if explicit:
        _feed(tr, algo, N, B, steps)
    tr.train(max_vector_steps=steps)
    torch.cuda.synchronize()
    return tr


@pytest.mark.parametrize("case", range(len(TRAIN_SHAPES)))
@pytest.mark.parametrize("env_name", ENV_NAMES)
@pytest.mark.parametrize("algo", ["dqn", "ddqn_per", "dsac"])
def test_fused_step_equals_layer_by_layer(algo, env_name, case):
    N, B, hidden, steps = TRAIN_SHAPES[case]
    explicit = case % 2 == 0                 # explicit draws in two cases, the kernels' own Philox in the third
    a = _run(algo, env_name, False, steps, N, B, hidden, explicit, graphs=False)
    b = _run(algo, env_name, True, steps, N, B, hidden, explicit)
    assert a._fused is None and b._fused is not None and b._fused[0] is not None
    assert _steps_taken(b, algo) >= 10
    assert len(b.episode_rewards) >= 3       # the planted ends: auto-reset and the terminal observation took part
    _assert_same(algo, a, b)


# ---- 3. a StepChunk replay ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_name", ENV_NAMES)
@pytest.mark.parametrize("algo", ["dqn", "ddqn_per", "dsac"])
def test_chunked_graph_equals_eager(algo, env_name):
    """16 vector steps replay as ONE captured graph, every per-step scalar read from the device record of its step."""
    N, B, hidden, steps = 64, 64, 64, 48
    a = _run(algo, env_name, True, steps, N, B, hidden, False, graphs=False)
    b = _run(algo, env_name, True, steps, N, B, hidden, False, graphs=True)
    assert getattr(a, "_chunk", None) is None
    assert b._chunk is not None and b._chunk.graph is not None         # at least one chunk did replay
    assert _steps_taken(b, algo) >= 32 and len(b.episode_rewards) >= 3
    _assert_same(algo, a, b)


# ---- 4. the new entry point on CartPole is the old one ----------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["dqn", "dsac"])
def test_cartpole_through_the_new_entry_is_the_old_entry(algo):
    from gymrl_amd import dqn_cartpole, ops, sac_cartpole
    N, hidden, steps = 33, 36, 12
    out = []
    for entry in ("gymrl_%s_act_step" % algo, "gymrl_%s_act_step_classic" % algo):
        mod = dqn_cartpole if algo == "dqn" else sac_cartpole
        cfg = mod.Config()
        cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed, cfg.fused_step = N, 64, hidden, 5, True
        tr = (mod.DQNTrainer if algo == "dqn" else mod.SACTrainer)(cfg)
        assert tr.env.kind == ops.CARTPOLE and tr._fused_ok()
        dev, D = tr.device, tr.env.obs_dim
        obs, nxt = tr.env.reset(), torch.empty(N, D, device=dev)
        rew, ret = torch.full((N,), -7.0, device=dev), torch.zeros(N, device=dev)
        done, act = torch.zeros(N, dtype=torch.uint8, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
        args, trace = tr._fused_args()[0], []
        for t in range(steps):
            if algo == "dqn":
                ops.dqn_act_step(args, tr.env, obs, nxt, epsilon=0.5, cursor=tr.memory.cursor, seed=tr.base_seed, counter=t + 1,
                                 action_out=act, rew_out=rew, done_out=done, ep_ret_out=ret, entry=entry)
            else:
                ops.dsac_act_step(args, tr.env, obs, nxt, cursor=tr.memory.cursor, seed=tr.base_seed, counter=t + 1,
                                  action_out=act, rew_out=rew, done_out=done, ep_ret_out=ret, entry=entry)
            tr.memory.advance(N)
            trace.append(tuple(x.clone() for x in (act, nxt, rew, done, ret)))
            obs, nxt = nxt, obs
        torch.cuda.synchronize()
        out.append((tr, trace))
    (a, ta), (b, tb) = out
    for t, (xa, xb) in enumerate(zip(ta, tb)):
        for k, (x, y) in enumerate(zip(xa, xb)):
            assert torch.equal(x, y), (t, k)
    assert torch.cat([x[0] for x in ta]).unique().numel() == 2                      # both actions were taken
    for x, y in zip(a.memory.ring, b.memory.ring):
        assert torch.equal(x, y)
    assert torch.equal(a.env.state, b.env.state) and a.memory.cursor == b.memory.cursor == N * steps


# ---- 5. the trainers whose kernels are two-action ones stay on the layer path ------------------------------------------------------
@pytest.mark.parametrize("algo", ["ddqn_duel", "ndqn", "rainbow"])
def test_two_action_trainers_fall_back_on_acrobot(algo, monkeypatch):
    """The dueling combine of gymrl_ddqn_update, NoisyNet and Rainbow is a two-action one: with fused_step = True on Acrobot-v1
    these trainers train layer by layer, and no act-step entry point is called."""
    from gymrl_amd import _lib
    L, calls = _lib.lib(), []
    for name in ACT_ENTRIES:
        real = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, name=name, real=real: (calls.append(name), real(*a))[1])
    tr = _trainer(algo, "Acrobot-v1", 16, 32, 32, True, plant=False)
    assert tr.cfg.fused_step is True
    assert not (tr._fused_act_ok() if algo == "rainbow" else tr._fused_ok())       # (Rainbow's name for the same predicate)
    tr.train(max_vector_steps=8)
    torch.cuda.synchronize()
    assert calls == []
    assert all(bool(torch.isfinite(p).all()) for p in tr.policy_net.parameters())
