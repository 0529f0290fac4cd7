"""The fused DQN vector step (csrc/dqn_step.hip: acting + env + replay row in one launch, update() in two) against the
layer-by-layer path it replaces (gymrl_lin_* launches, the stand-alone epsilon-greedy / TD-loss / clamp + Adam / replay / env
kernels, which tests/test_trainers_gpu.py pins against the reference's own update()): same uniforms, same index draws -> every
parameter, Adam moment, the target, the loss sum, the replay ring and every host counter equal BIT FOR BIT."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _trainer(N, B, hidden, fused, graphs=None, images=True, seed=5, **more):
    from gymrl_amd import dqn_cartpole
    cfg = dqn_cartpole.Config()
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed = N, B, hidden, seed
    cfg.max_episodes, cfg.memory_capacity = 10 ** 9, (1 << 20 if N >= 4096 else max(4096, 4 * B))
    cfg.fused_step, cfg.fused_images = fused, images
    if graphs is not None:
        cfg.use_graphs = graphs
    for k, v in more.items():
        setattr(cfg, k, v)
    return dqn_cartpole.DQNTrainer(cfg)


def _uniforms(N, steps, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.rand(N, 2, generator=g, device="cuda") for _ in range(steps)]


def _run(fused, steps, N, B, hidden, explicit=True, images=True, **more):
    """Trainer A (layer path, eager update) or B (fused_step alone).  explicit: uniforms through _parity_u; otherwise the
    kernels' own Philox.  Each path draws its own indices from the same (seed, counter, size)."""
    tr = _trainer(N, B, hidden, fused, graphs=None if fused else False, images=images, **more)
    assert tr._fused_ok() == fused
    if explicit:
        tr._parity_u = iter(_uniforms(N, steps))
    tr.train(max_vector_steps=steps)
    torch.cuda.synchronize()
    return tr


def _assert_same(a, b, what=""):
    assert a.optimizer.step_count == b.optimizer.step_count, what
    assert (a.memory.cursor, a.memory.size, a.memory.draws) == (b.memory.cursor, b.memory.size, b.memory.draws), what
    assert (a._act_counter, a.sample_count, a.epsilon) == (b._act_counter, b.sample_count, b.epsilon), what
    for k, (x, y) in enumerate(zip(a.memory.ring, b.memory.ring)):
        assert torch.equal(x, y), (what, "ring", k)          # acting: same actions, same physics, same rows
    for name in ("flat_params", "target_flat", "_loss"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name, getattr(a, name), getattr(b, name))
    assert torch.equal(a.optimizer.m, b.optimizer.m) and torch.equal(a.optimizer.v, b.optimizer.v), what
    assert list(a.episode_rewards) == list(b.episode_rewards), what


# (hidden 256: the instances built for that width, weight images; 36: no images, no 16-column alignment; B = 24 / 100 / 250: a
#  partial last slab; N = 1: the scalar surface's; 4096 / 128 / 256: 256 acting workgroups, ring of 2^20 rows)
SHAPES = [(64, 64, 256, 16), (20, 24, 32, 14), (33, 100, 36, 16), (17, 250, 256, 28), (1, 16, 32, 40), (4096, 128, 256, 12)]


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_fused_step_equals_layer_by_layer(case):
    N, B, hidden, steps = SHAPES[case]
    explicit = case % 2 == 0                 # explicit uniforms in half the cases, the kernels' own Philox in the other half
    a, b = _run(False, steps, N, B, hidden, explicit), _run(True, steps, N, B, hidden, explicit)
    assert a._fused is None and b._fused is not None
    assert b.optimizer.step_count >= 10
    assert len(b.episode_rewards) >= 1       # auto-reset and the terminal observation took part
    _assert_same(a, b)


@pytest.mark.parametrize("N,hidden,steps", [(4096, 256, 24), (50, 64, 60)])
def test_act_launch_equals_the_kernels_composed_by_hand(N, hidden, steps):
    """gymrl_dqn_act_step against policy_net (gymrl_lin_fwd) -> ops.epsilon_greedy -> env.step -> memory.push, kernels that
    are pinned to the oracle one by one, step by step.  Through explicit u: epsilon = 0 (greedy whatever u0), epsilon = 1
    (explore whatever u0), u1 = 0.99999994 (the largest float32 below one: the action is clamped to A - 1), u0 == epsilon
    exactly (`u0 < epsilon` is false: greedy).  For the last third of the steps the policy's last layer is zero: equal Q
    values, and the first maximum is action 0."""
    from gymrl_amd import ops
    a, b = _trainer(N, 64, hidden, False), _trainer(N, 64, hidden, True)
    assert torch.equal(a.flat_params, b.flat_params)
    dev, D = a.device, a.env.obs_dim
    draws = _uniforms(N, steps, seed=3)
    obs_a, obs_b = a.env.reset(), torch.empty(N, D, device=dev)
    b.env.reset(obs_b)
    assert torch.equal(obs_a, obs_b)
    nxt_a, tobs, nxt_b = (torch.empty(N, D, device=dev) for _ in range(3))
    rew_a, rew_b = torch.empty(N, device=dev), torch.empty(N, device=dev)
    done_a, done_b = (torch.zeros(N, dtype=torch.uint8, device=dev) for _ in range(2))
    act_b = torch.empty(N, dtype=torch.int32, device=dev)
    eps_cycle = (0.0, 0.5, 1.0, 0.25, 0.9, 0.05)
    dones, seen = 0, set()
    for t in range(steps):
        eps = eps_cycle[t % len(eps_cycle)]
        u = draws[t].clone() if (t % 2 == 0 or eps in (0.0, 1.0)) else None          # explicit / Philox
        if u is not None:
            u[0::5, 1] = 0.99999994                                # (int)(u1 * A) stays below A only by the clamp's side of rounding
            if 0.0 < eps < 1.0:
                u[1::5, 0] = float(np.float32(eps))                # u0 == epsilon: not below it, greedy
                u[2::5, 0] = float(np.nextafter(np.float32(eps), np.float32(0.0)))   # one ulp below: explores
        if t == steps - steps // 3:                                # equal Q values from here on
            for tr in (a, b):
                with torch.no_grad():
                    tr.policy_net.net[4].weight.zero_()
                    tr.policy_net.net[4].bias.zero_()
        args = b._fused_args()[0]
        with torch.no_grad():
            q = a.policy_net(obs_a)
        act_a = ops.epsilon_greedy(q, eps, u=u, seed=a.base_seed, counter=t + 1, env_id0=a.env.env_id0)
        if u is not None and eps == 0.0:                           # greedy: the first maximum, whatever u says
            best = q.argmax(dim=1)
            ties = q[:, 0] == q[:, 1]
            assert torch.equal(act_a[~ties].long(), best[~ties]) and bool((act_a[ties] == 0).all())
            seen.add("greedy")
        if u is not None and eps == 1.0:                           # explore: (int)(u1 * A), clamped
            assert torch.equal(act_a.long(), (u[:, 1] * 2.0).long().clamp(max=1))
            assert bool((act_a[0::5] == 1).all())
            seen.add("explore")
        if u is not None and 0.0 < eps < 1.0:
            rows = torch.arange(1, N, 5, device=dev)
            ties = q[rows, 0] == q[rows, 1]
            assert torch.equal(act_a[rows][~ties].long(), q[rows].argmax(dim=1)[~ties])          # u0 == eps is greedy
            rows = torch.arange(2, N, 5, device=dev)
            assert torch.equal(act_a[rows].long(), (u[rows, 1] * 2.0).long().clamp(max=1))       # one ulp below explores
            seen.add("edge")
        if t >= steps - steps // 3 and eps == 0.0:
            assert bool((q == 0).all()) and bool((act_a == 0).all())
            seen.add("equal-q")
        a.env.step(act_a, nxt_a, rew_a, done_out=done_a, term_obs_out=tobs)
        a.memory.push(obs_a, act_a, rew_a, tobs, done_a)
        ops.dqn_act_step(args, b.env, obs_b, nxt_b, epsilon=eps, cursor=b.memory.cursor, u=u, seed=b.base_seed, counter=t + 1,
                         action_out=act_b, rew_out=rew_b, done_out=done_b)
        b.memory.advance(N)
        assert torch.equal(act_a, act_b) and torch.equal(nxt_a, nxt_b) and torch.equal(rew_a, rew_b) and torch.equal(done_a, done_b), t
        dones += int(done_a.sum().item())
        obs_a, nxt_a = nxt_a, obs_a
        obs_b, nxt_b = nxt_b, obs_b
    print("episode ends:", dones)
    assert seen == {"greedy", "explore", "edge", "equal-q"}
    assert steps < 60 or dones >= N
    assert (a.memory.cursor, a.memory.size) == (b.memory.cursor, b.memory.size)
    for x, y in zip(a.memory.ring, b.memory.ring):
        assert torch.equal(x, y)


def test_target_copies_happen_at_the_same_steps():
    """N = 64, a hard copy every 4 episodes, 48 steps from the default epsilon: the layer loop copies where its tracker flushes
    (every 16 steps), the fused loop collects a chunk's episodes at the chunk boundary and copies there."""
    out = []
    for fused in (False, True):
        tr = _trainer(64, 64, 256, fused, graphs=None if fused else False, target_update_freq=4)
        assert tr._fused_ok() == fused
        initial = tr.target_flat.clone()
        calls, real = [], tr.load_target
        tr.load_target = lambda calls=calls, real=real, tr=tr: (calls.append(tr.optimizer.step_count), real())[1]
        tr.train(max_vector_steps=48)
        torch.cuda.synchronize()
        assert len(calls) >= 2, calls
        assert not torch.equal(tr.target_flat, initial)
        out.append((tr, calls))
    (a, ca), (b, cb) = out
    assert b._chunk is not None and b._chunk.graph is not None         # the fused run did replay chunks
    assert ca == cb                                                    # the copies sit behind the same optimiser steps
    _assert_same(a, b)


def _chunk_run(graphs, inject, N=64, B=64, hidden=256):
    tr = _trainer(N, B, hidden, True, graphs=graphs)
    assert tr._fused_ok()
    if inject:                  # fill the ring, then ONE update outside train(): every counter starts elsewhere in the chunks
        tr.train(max_vector_steps=8)
        tr.update()
    tr.train(max_vector_steps=64)
    torch.cuda.synchronize()
    return tr


@pytest.mark.parametrize("inject", [False, True])
def test_chunked_graph_equals_eager(inject):
    """16 vector steps replay as ONE captured graph, every per-step scalar read from the device record of its step."""
    a, b = _chunk_run(False, inject), _chunk_run(True, inject)
    assert getattr(a, "_chunk", None) is None
    assert b._chunk is not None and b._chunk.graph is not None
    assert b.optimizer.step_count >= 48
    _assert_same(a, b)


def test_stop_rule_that_holds_at_entry_stops_after_one_step():
    """mean(last 100) >= 495 already holds when train() is entered: the layer loop looks at the rule after every step and stops
    after the first; the fused loop must not run a whole chunk before it looks."""
    out = []
    for fused in (False, True):
        tr = _trainer(64, 64, 64, fused, graphs=None if fused else False)
        tr.train(max_vector_steps=16)                      # the ring holds a batch: the fused loop could chunk from step 0
        tr.episode_rewards.clear()
        tr.episode_rewards.extend([500.0] * 100)
        before = tr.optimizer.step_count
        tr.train(max_vector_steps=64)
        torch.cuda.synchronize()
        assert tr.optimizer.step_count == before + 1
        out.append(tr)
    _assert_same(out[0], out[1])


def test_images_change_where_a_value_is_read_not_the_value():
    from gymrl_amd import ops
    N, B, hidden, steps = 64, 64, 256, 16
    # (no hard copy in these 16 steps: since their first build the images are kept by the update's tile kernel alone)
    b = _run(True, steps, N, B, hidden, target_update_freq=10 ** 9)
    c = _run(True, steps, N, B, hidden, images=False, target_update_freq=10 ** 9)
    assert b._fused[4] is not None and c._fused[4] is None
    _assert_same(b, c)
    before = b._fused[4].clone()                       # and they do hold the parameters: rebuilding them changes nothing
    ops.dqn_pack_images(b._fused[1])
    torch.cuda.synchronize()
    assert torch.equal(before, b._fused[4])
    assert before.abs().sum().item() > 0


def _switch_schedule(fused, tmp_path=None):
    tr = _trainer(48, 64, 64, fused, graphs=None if fused else False)
    tr.train(max_vector_steps=9)
    tr.cfg.fused_step = False
    assert not tr._fused_update_ok()
    tr.update()
    tr.load_target()
    tr.cfg.fused_step = fused
    if tmp_path is not None:        # leave the schedule for one more layer-path update, then come back by the checkpoint
        path = str(tmp_path / "dqn.pt")
        tr.save_checkpoint(path)
        tr.cfg.fused_step = False
        tr.update()
        tr.cfg.fused_step = fused
        tr.load_checkpoint(path)
    tr.train(max_vector_steps=9)
    torch.cuda.synchronize()
    return tr


def test_switching_between_the_paths(tmp_path):
    """9 fused steps, one layer-by-layer update() and a load_target() (both leave the weight images stale), 9 more fused steps ==
    the same schedule on the layer path throughout; and a load_checkpoint() of the state saved in the middle, after a further
    update had moved everything, continues exactly like the uninterrupted run."""
    layer, fused, resumed = _switch_schedule(False), _switch_schedule(True), _switch_schedule(True, tmp_path)
    assert fused._fused is not None and fused._fused[4] is not None
    _assert_same(layer, fused, "switch")
    _assert_same(fused, resumed, "checkpoint")


def test_checkpoint_saved_on_one_path_resumes_on_the_other(tmp_path):
    path = str(tmp_path / "dqn_cross.pt")
    src = _trainer(48, 64, 64, True)
    src.train(max_vector_steps=10)
    src.save_checkpoint(path)
    out = []
    for fused in (False, True):
        tr = _trainer(48, 64, 64, fused, graphs=None if fused else False)
        tr.load_checkpoint(path)
        for _ in range(3):
            tr.update()
        torch.cuda.synchronize()
        out.append(tr)
    assert out[0]._fused is None and out[1]._fused is not None
    _assert_same(out[0], out[1])
    assert out[0].optimizer.step_count == src.optimizer.step_count + 3


@pytest.mark.parametrize("B,more", [(300, {}), (64, {"max_steps": 200}), (64, {"updates_per_step": 2})])
def test_what_the_step_cannot_take_trains_layer_by_layer(B, more):
    """B = 300: no fused update at all.  cfg.max_steps = 200 (< the env's 500: the loop needs env.abandon) and
    updates_per_step = 2: the loop stays the layer path's.  Training is not refused, and the switch changes no bit."""
    out = []
    for fused in (True, False):
        tr = _trainer(64, B, 64, fused, graphs=False, **more)
        assert not tr._fused_ok()
        assert tr._fused_update_ok() is (fused and B <= 256)
        tr.train(max_vector_steps=8)
        torch.cuda.synchronize()
        assert tr.optimizer.step_count == (8 - (B + 63) // 64 + 1) * more.get("updates_per_step", 1)
        if B > 256:
            assert tr._fused is None
        out.append(tr)
    _assert_same(out[0], out[1])


def test_unsupported_batch_is_refused_by_the_library():
    from gymrl_amd import _lib, ops
    tr = _trainer(64, 300, 64, True, graphs=False)
    tr.train(max_vector_steps=6)
    m = tr.memory
    ws = ops.dqn_update_workspace(300, 4, 2, 64, tr.device)
    for B in (300, 257):
        a = ops.dqn_update_args(B, 4, 2, tr.policy_net, tr.target_net, tr.optimizer, m.ring, 0.99, tr._loss, ws)
        a.idx_size = m.size
        before = tr.flat_params.clone()
        rc = _lib.lib().gymrl_dqn_update(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == -22 and torch.equal(before, tr.flat_params)


def test_fused_update_matches_reference(monkeypatch):
    """tests/test_trainers_gpu.py::test_dqn_update_matches_reference itself (tests/golden/dqn_update.npz: one reference
    update(); loss <= 1e-5, the policy net <= 2e-6 after its clamped Adam step) with Config.fused_step switched on."""
    from gymrl_amd import dqn_cartpole, ops
    import test_trainers_gpu
    calls = []

    class FusedConfig(dqn_cartpole.Config):
        def __init__(self):
            super().__init__()
            self.fused_step = True

    real = ops.dqn_update
    monkeypatch.setattr(dqn_cartpole, "Config", FusedConfig)
    monkeypatch.setattr(ops, "dqn_update", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    test_trainers_gpu.test_dqn_update_matches_reference()
    assert len(calls) == 1                             # the fused update did run


def test_defaults_never_build_the_fused_step():
    from gymrl_amd import dqn_cartpole
    cfg = dqn_cartpole.Config()
    cfg.num_envs, cfg.hidden_dim, cfg.seed = 32, 32, 1
    tr = dqn_cartpole.DQNTrainer(cfg)
    assert not tr._fused_update_ok() and not tr._fused_ok()
    tr.train(max_vector_steps=6)
    tr.update()
    torch.cuda.synchronize()
    assert tr._fused is None and getattr(tr, "_chunk", None) is None and tr.optimizer.step_count == 6
