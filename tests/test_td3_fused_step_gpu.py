"""The fused TD3 / DDPG vector step (csrc/td3_step.hip: acting + env + replay row in one launch, update() in at most
four) against the layer-by-layer path it replaces (gymrl_lin_* launches + the stand-alone noise / loss / optimiser / replay /
env kernels, which tests/test_trainers_gpu.py pins against the reference's own update()): same noise, same index draws ->
every parameter, Adam moment, both target networks, the loss sums and the replay ring equal BIT FOR BIT."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FLATS = ("actor_flat", "critic_flat", "actor_target_flat", "critic_target_flat")


def _trainer(algo, N, B, hidden, fused, graphs=False, images=True, seed=5):
    """algo: "ddpg", or "td3/<policy_freq>"."""
    from gymrl_amd import ddpg_pendulum, td3_pendulum
    if algo == "ddpg":
        cfg, cls = ddpg_pendulum.Config(), ddpg_pendulum.DDPGTrainer
    else:
        cfg, cls = td3_pendulum.Config(), td3_pendulum.TD3Trainer
        cfg.policy_freq = int(algo.split("/")[1])
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed = N, B, hidden, seed
    cfg.max_episodes, cfg.memory_capacity = 10 ** 9, (1 << 20 if N >= 4096 else max(4096, 4 * B))
    cfg.use_graphs, cfg.fused_step, cfg.fused_images = graphs, fused, images
    return cls(cfg)


def _parity(tr, algo, steps, explicit_update_eps):
    """Explicit f64 exploration draws; update draws explicit or the kernels' own Philox (eps None); indices None: each path draws
    its own (the layer path through gymrl_uniform_indices, the fused path inside R1) from the same (seed, counter, size)."""
    g = torch.Generator(device="cuda").manual_seed(7)
    N, A, B = tr.env.n, tr.env.act_dim, tr.cfg.batch_size
    tr._parity_eps = iter([torch.randn(N, A, generator=g, device="cuda", dtype=torch.float64) for _ in range(steps)])
    ups = [torch.randn(B, A, generator=g, device="cuda", dtype=torch.float64) if explicit_update_eps else None for _ in range(steps)]
    tr._parity_updates = iter([None] * steps) if algo == "ddpg" else iter([(None, e) for e in ups])


def _run(algo, fused, steps, N, B, hidden, explicit=True, images=True):
    tr = _trainer(algo, N, B, hidden, fused, images=images)
    assert tr._fused_ok() == fused
    _parity(tr, algo, steps, explicit)
    tr.train(max_vector_steps=steps)
    torch.cuda.synchronize()
    return tr


def _assert_same(a, b, what=""):
    assert a.critic_optimizer.step_count == b.critic_optimizer.step_count, what
    assert a.actor_optimizer.step_count == b.actor_optimizer.step_count, what
    assert (a.memory.cursor, a.memory.size, a.memory.draws) == (b.memory.cursor, b.memory.size, b.memory.draws), what
    assert (a._act_counter, a._noise_counter, getattr(a, "total_updates", 0)) == (b._act_counter, b._noise_counter, getattr(b, "total_updates", 0)), what
    for k, (x, y) in enumerate(zip(a.memory.ring, b.memory.ring)):
        assert torch.equal(x, y), (what, "ring", k)          # acting: same actions, same physics, same rows
    for name in FLATS:
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    for opt in ("actor_optimizer", "critic_optimizer"):
        assert torch.equal(getattr(a, opt).m, getattr(b, opt).m) and torch.equal(getattr(a, opt).v, getattr(b, opt).v), (what, opt)
    assert torch.equal(a._sum_c, b._sum_c) and torch.equal(a._sum_a, b._sum_a), what
    assert list(a.episode_rewards) == list(b.episode_rewards), what


# (hidden 256: the instances built for that width; 36: no weight images, no 16-column alignment; B = 100 / 250: a partial last
#  slab; 4096 / 128 / 256 is BASELINE config 4's size: 256 acting workgroups, ring of 2^20 rows)
SHAPES = [(64, 128, 256, 16), (20, 24, 32, 14), (33, 100, 36, 16), (17, 250, 256, 28), (4096, 128, 256, 12)]


# (DDPG's update draws no noise: one case per shape covers it)
CASES = [(algo, *shape, explicit) for algo in ("td3/2", "td3/3", "ddpg") for shape in SHAPES for explicit in (True, False)
         if explicit or algo != "ddpg"]


@pytest.mark.parametrize("algo,N,B,hidden,steps,explicit", CASES)
def test_fused_step_equals_layer_by_layer(algo, N, B, hidden, steps, explicit):
    a, b = _run(algo, False, steps, N, B, hidden, explicit), _run(algo, True, steps, N, B, hidden, explicit)
    assert b.critic_optimizer.step_count >= 10
    if algo != "ddpg":       # delayed and non-delayed steps both occurred
        assert 0 < b.actor_optimizer.step_count < b.critic_optimizer.step_count
    _assert_same(a, b)


@pytest.mark.parametrize("algo", ["td3/2", "ddpg"])
def test_images_change_where_a_value_is_read_not_the_value(algo):
    from gymrl_amd import ops
    N, B, hidden, steps = 64, 128, 256, 16
    b, c = _run(algo, True, steps, N, B, hidden), _run(algo, True, steps, N, B, hidden, images=False)
    assert b._fused[4] is not None and c._fused[4] is None
    _assert_same(b, c)
    before = b._fused[4].clone()                       # and they do hold the parameters: rebuilding them changes nothing
    ops.td3_pack_images(b._fused[1])
    torch.cuda.synchronize()
    assert torch.equal(before, b._fused[4])
    assert before.abs().sum().item() > 0


@pytest.mark.parametrize("name", ["ddpg", "td3"])
def test_fused_update_matches_reference(name):
    """tests/test_trainers_gpu.py::test_td3_ddpg_update_matches_reference's scenario (tests/golden/td3_ddpg.npz: one DDPG
    update; two consecutive TD3 updates, the second delayed) through the FUSED update, with that test's tolerances."""
    from conftest import load_golden as lg
    from gymrl_amd import ddpg_pendulum, td3_pendulum
    from test_trainers_gpu import _load_prefixed, _maxdiff
    g = lg("td3_ddpg")
    mod, cls = (ddpg_pendulum, "DDPGTrainer") if name == "ddpg" else (td3_pendulum, "TD3Trainer")
    cfg = mod.Config()
    cfg.batch_size, cfg.hidden_dim, cfg.num_envs, cfg.fused_step = 24, 32, 1, True
    tr = getattr(mod, cls)(cfg)
    assert tr._fused_update_ok()
    dev = tr.device
    for key in ("actor", "critic", "actor_target", "critic_target"):
        _load_prefixed(getattr(tr, key), g, f"{name}_u0_{key}_")
    td = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else a.astype(dt))).to(dev)  # noqa: E731
    tr.memory.push(td(g[f"{name}_states"]), td(g[f"{name}_actions"], np.float32), td(g[f"{name}_rewards"]),
                   td(g[f"{name}_next_states"]), td(g[f"{name}_dones"]))
    for k, order in enumerate(g[f"{name}_orders"]):
        if name == "ddpg":
            al, cl = tr.update(indices=td(order))
        else:
            al, cl = tr.update(indices=td(order), eps=td(g["td3_eps"][k]))
        want = g[f"{name}_losses"][k]
        print(name, k, "losses", (al, cl), "want", tuple(want))
        assert abs(al - want[0]) <= 1e-5 * max(1.0, abs(want[0])) and abs(cl - want[1]) <= 1e-5 * max(1.0, abs(want[1]))
    assert tr._fused is not None                       # the fused update did run
    for key in ("actor", "critic", "actor_target", "critic_target"):
        d = _maxdiff(getattr(tr, key), g, f"{name}_u1_{key}_")
        print(name, key, "max abs diff", d)
        assert d <= 5e-6, key


def _chunk_run(algo, graphs, inject, N=64, B=128, hidden=256):
    tr = _trainer(algo, N, B, hidden, True, graphs=graphs)
    assert tr._fused_ok()
    if inject:                  # fill the ring, then ONE update outside train(): the delayed steps fall elsewhere in the chunks
        tr.train(max_vector_steps=8)
        tr.update()
    tr.train(max_vector_steps=64)
    torch.cuda.synchronize()
    return tr


@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("algo", ["td3/2", "td3/3", "ddpg"])
def test_chunked_graph_equals_eager(algo, inject):
    """16 vector steps replay as ONE captured graph; which of its steps are delayed is read from the device record of each step
    (with policy_freq 3 the pattern moves from one replay to the next, with the injected update it starts elsewhere)."""
    a, b = _chunk_run(algo, False, inject), _chunk_run(algo, True, inject)
    assert getattr(a, "_chunk", None) is None
    assert b._chunk is not None and b._chunk.graph is not None
    assert b.critic_optimizer.step_count >= 48
    _assert_same(a, b)


@pytest.mark.parametrize("algo", ["td3/2", "ddpg"])
def test_switching_between_the_paths(algo):
    """k fused steps, one layer-by-layer update() (which leaves the weight images stale), more fused steps == the same schedule
    on the layer path throughout."""
    out = []
    for fused in (False, True):
        tr = _trainer(algo, 48, 64, 64, fused)
        tr.train(max_vector_steps=9)
        tr.cfg.fused_step = False
        assert not tr._fused_update_ok()
        tr.update()
        tr.soft_update(tr.critic_target_flat, tr.critic_flat)
        tr.cfg.fused_step = fused
        tr.train(max_vector_steps=9)
        torch.cuda.synchronize()
        out.append(tr)
    assert out[1]._fused is not None and out[1]._fused[4] is not None
    _assert_same(out[0], out[1])


@pytest.mark.parametrize("N,hidden,steps", [(4096, 256, 24), (50, 64, 230)])
def test_act_launch_equals_the_kernels_composed_by_hand(N, hidden, steps):
    """gymrl_td3_act_step against actor (gymrl_lin_fwd) -> ops.noisy_action mode 0 -> env.step -> memory.push, kernels that are
    pinned to the oracle one by one; 230 steps cross Pendulum's 200-step episode end (auto-reset, TERMINAL observation)."""
    from gymrl_amd import ops
    from gymrl_amd.envs import VecEnv
    a, b = _trainer("td3/2", N, 128, hidden, False), _trainer("td3/2", N, 128, hidden, True)
    assert torch.equal(a.actor_flat, b.actor_flat)
    dev, D, A = a.device, a.env.obs_dim, a.env.act_dim
    g = torch.Generator(device="cuda").manual_seed(3)
    obs_a, obs_b = a.env.reset(), torch.empty(N, D, device=dev)
    b.env.reset(obs_b)
    assert torch.equal(obs_a, obs_b)
    nxt_a, tobs, nxt_b = (torch.empty(N, D, device=dev) for _ in range(3))
    rew_a, rew_b = torch.empty(N, device=dev), torch.empty(N, device=dev)
    done_a, done_b = (torch.zeros(N, dtype=torch.uint8, device=dev) for _ in range(2))
    act_b = torch.empty(N, A, device=dev)
    args = b._fused_args()[0]
    dones = 0
    for t in range(steps):
        eps = torch.randn(N, A, generator=g, device="cuda", dtype=torch.float64) if t % 2 == 0 else None    # explicit / Philox
        with torch.no_grad():
            mu = a.actor(obs_a).contiguous()
        act_a = ops.noisy_action(mu, a._exploration_std() * a.action_bound, a.action_bound, eps=eps, mode=0, seed=a.base_seed, counter=t + 1)
        a.env.step(act_a, nxt_a, rew_a, done_out=done_a, term_obs_out=tobs)
        a.memory.push(obs_a, act_a, rew_a, tobs, done_a)
        ops.td3_act_step(args, b.env, obs_b, nxt_b, cursor=b.memory.cursor, eps=eps, noise_seed=b.base_seed, noise_counter=t + 1,
                         action_out=act_b, rew_out=rew_b, done_out=done_b)
        b.memory.advance(N)
        assert torch.equal(act_a, act_b) and torch.equal(nxt_a, nxt_b) and torch.equal(rew_a, rew_b) and torch.equal(done_a, done_b), t
        dones += int(done_a.sum().item())
        obs_a, nxt_a = nxt_a, obs_a
        obs_b, nxt_b = nxt_b, obs_b
    assert isinstance(b.env, VecEnv) and (steps < 200 or dones >= N)
    assert (a.memory.cursor, a.memory.size) == (b.memory.cursor, b.memory.size)
    for x, y in zip(a.memory.ring, b.memory.ring):
        assert torch.equal(x, y)


def test_unsupported_batch_is_refused_and_trains_layer_by_layer():
    from gymrl_amd import _lib, ops
    out = []
    for fused in (True, False):
        tr = _trainer("td3/2", 64, 300, 64, fused)
        assert tr._fused_update_ok() is False and not tr._fused_ok()
        tr.train(max_vector_steps=8)
        torch.cuda.synchronize()
        assert tr._fused is None and tr.critic_optimizer.step_count == 4
        out.append(tr)
    _assert_same(out[0], out[1])
    tr = out[0]
    m = tr.memory
    ws = ops.td3_update_workspace(300, 3, 1, 64, tr.device)
    for B, want in ((300, -22), (257, -22)):
        a = ops.td3_update_args(B, 3, 1, 2, tr.actor, tr.actor_target, tr.critic, tr.critic_target, tr.actor_optimizer, tr.critic_optimizer,
                                m.ring, (0.99, 0.005, 2.0, 0.2, 0.5), tr._sums, ws)
        a.idx_size = m.size
        before = tr.critic_flat.clone()
        rc = _lib.lib().gymrl_td3_update(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == want and torch.equal(before, tr.critic_flat)
