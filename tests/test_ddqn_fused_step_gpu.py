"""The fused DDQN + PER update (csrc/ddqn_step.hip: three forward chains, double-Q target, weighted loss gradient and the
input-gradient chain in one row launch, then the tile launch) with gymrl_dqn_act_step for acting, against the layer-by-layer
path it replaces (gymrl_lin_* launches and the stand-alone TD-loss / clamp + Adam / replay / env kernels, which
tests/test_ddqn_trainers_gpu.py pins against the reference's own update()): same uniforms, same draws -> every parameter, Adam
moment, the target, the loss sum, the replay ring, the whole float64 sum tree, beta and every host counter equal BIT FOR BIT."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _trainer(N, B, hidden, cap, fused, graphs=None, images=True, seed=5, duel=False, **more):
    from gymrl_amd import ddqn_per_cartpole, ddqn_per_duel_cartpole
    cfg = ddqn_per_cartpole.Config()
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed, cfg.memory_capacity = N, B, hidden, seed, cap
    cfg.max_episodes, cfg.fused_step, cfg.fused_images = 10 ** 9, fused, images
    if graphs is not None:
        cfg.use_graphs = graphs
    for k, v in more.items():
        setattr(cfg, k, v)
    return (ddqn_per_duel_cartpole.DDQNPERDuelTrainer if duel else ddqn_per_cartpole.DDQNPERTrainer)(cfg)


def _uniforms(N, steps, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.rand(N, 2, generator=g, device="cuda") for _ in range(steps)]


def _strata(B, steps, seed=11):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.rand(B, generator=g, device="cuda", dtype=torch.float64) for _ in range(steps)]


def _run(fused, steps, N, B, hidden, cap, explicit=True, watch=None, **more):
    """Trainer A (layer path, eager update) or B (fused_step).  explicit: uniforms through _parity_u / _parity_v; otherwise the
    kernels' own Philox.  watch: list that receives every sampled row batch (eager loops only)."""
    tr = _trainer(N, B, hidden, cap, fused, graphs=None if fused else False, **more)
    assert tr._fused_ok() == fused
    if explicit:
        tr._parity_u, tr._parity_v = iter(_uniforms(N, steps)), iter(_strata(B, steps))
    if watch is not None:           # every draw with the tree it was made from: (tree, size, beta, leaves)
        real, m = tr.memory.draw, tr.memory

        def draw(*a, **k):
            tree, size = m.tree.tree.clone(), m.size
            out = real(*a, **k)
            watch.append((tree, size, m.cfg.beta, out[2].clone()))
            return out
        m.draw = draw
    tr.train(max_vector_steps=steps)
    torch.cuda.synchronize()
    return tr


def _assert_same(a, b, what=""):
    assert a.optimizer.step_count == b.optimizer.step_count, what
    assert (a.memory.cursor, a.memory.size, a.memory.draws) == (b.memory.cursor, b.memory.size, b.memory.draws), what
    assert (a._act_counter, a.sample_count, a.epsilon, a.cfg.beta) == (b._act_counter, b.sample_count, b.epsilon, b.cfg.beta), what
    for k, (x, y) in enumerate(zip(a.memory.ring, b.memory.ring)):
        assert torch.equal(x, y), (what, "ring", k)          # acting: same actions, same physics, same rows
    assert torch.equal(a.memory.tree.tree, b.memory.tree.tree), (what, "tree")
    for name in ("flat_params", "target_flat", "_loss"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name, getattr(a, name), getattr(b, name))
    assert torch.equal(a.optimizer.m, b.optimizer.m) and torch.equal(a.optimizer.v, b.optimizer.v), what
    assert list(a.episode_rewards) == list(b.episode_rewards), what


# (N, B, hidden, capacity, steps).  hidden 256: the instance built for that width, weight images; 36: no images, no 16-column
# alignment; B = 24 / 100 / 250: a partial last slab; capacity 100: a tree that is no power of two, ring and tree wrap at step 5;
# N = 1: the scalar surface's; 4096 / 128 / 256: 256 acting workgroups, ring and tree of 2^20 rows
SHAPES = [(64, 64, 256, 4096, 16), (20, 24, 32, 100, 14), (33, 100, 36, 4096, 16), (17, 250, 256, 1024, 28), (1, 16, 32, 64, 40),
          (4096, 128, 256, 1 << 20, 12)]


EXPLICIT = (0, 1, 4)          # explicit uniforms in half the cases (the capacity-100 case among them), the kernels' own Philox in the other half


@pytest.mark.parametrize("duel", [False, True])
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_fused_step_equals_layer_by_layer(oracle, case, duel):
    N, B, hidden, cap, steps = SHAPES[case]
    explicit = case in EXPLICIT
    watch = [] if cap == 100 else None
    a = _run(False, steps, N, B, hidden, cap, explicit, watch=watch, duel=duel)
    b = _run(True, steps, N, B, hidden, cap, explicit, duel=duel)
    assert a._fused is None and b._fused is not None and bool(b._fused[1].dueling) == duel
    assert b.optimizer.step_count >= 10
    assert len(b.episode_rewards) >= 1       # auto-reset and the terminal observation took part
    if cap == 100:
        # a leaf drawn twice in one batch (the tree's last writer wins on both paths), established on the CPU: the oracle's
        # descent over the tree each draw was made from, under the same explicit uniforms, gives the GPU's leaves and a duplicate
        dup = False
        for (tree, size, beta, leaves), u in zip(watch, _strata(B, steps)):
            ref = oracle.SumTree(cap)
            ref.tree[:] = tree.cpu().numpy()
            idx, _, _ = ref.sample(B, size, beta, u=u.cpu().numpy(), variant_b=True)
            assert np.array_equal(idx, leaves.cpu().numpy())
            dup = dup or len(set(idx.tolist())) < B
        assert len(watch) >= 10 and dup
    _assert_same(a, b)


@pytest.mark.parametrize("N,hidden,steps", [(4096, 256, 24), (50, 64, 60)])
def test_dueling_act_launch_equals_the_kernels_composed_by_hand(N, hidden, steps):
    """gymrl_ddqn_duel_act_step against policy_net (gymrl_lin_fwd launches + the framework's combine) -> ops.epsilon_greedy ->
    env.step -> memory.push, step by step: actions, observations, rewards, dones and the ring rows, bit for bit.  Explicit u on
    even steps (epsilon 0, 1 and in between), the kernels' own Philox keys on the odd ones."""
    from gymrl_amd import ops
    a, b = _trainer(N, 64, hidden, 1 << 17, False, duel=True), _trainer(N, 64, hidden, 1 << 17, True, duel=True)
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
    dones, explored, greedy = 0, 0, 0
    args = b._fused_args()[0]
    for t in range(steps):
        eps = eps_cycle[t % len(eps_cycle)]
        u = draws[t] if (t % 2 == 0 or eps in (0.0, 1.0)) else None
        with torch.no_grad():
            q = a.policy_net(obs_a)
        act_a = ops.epsilon_greedy(q, eps, u=u, seed=a.base_seed, counter=t + 1, env_id0=a.env.env_id0)
        if eps == 0.0:
            ties = q[:, 0] == q[:, 1]
            assert torch.equal(act_a[~ties].long(), q.argmax(dim=1)[~ties])
            greedy += 1
        if eps == 1.0:
            assert torch.equal(act_a.long(), (u[:, 1] * 2.0).long().clamp(max=1))
            explored += 1
        a.env.step(act_a, nxt_a, rew_a, done_out=done_a, term_obs_out=tobs)
        a.memory.push(obs_a, act_a, rew_a, tobs, done_a)
        ops.ddqn_duel_act_step(args, b.env, obs_b, nxt_b, epsilon=eps, cursor=b.memory.cursor, u=u, seed=b.base_seed, counter=t + 1,
                               action_out=act_b, rew_out=rew_b, done_out=done_b)
        b.memory.advance(N)
        assert torch.equal(act_a, act_b) and torch.equal(nxt_a, nxt_b) and torch.equal(rew_a, rew_b) and torch.equal(done_a, done_b), t
        dones += int(done_a.sum())
        obs_a, nxt_a = nxt_a, obs_a
        obs_b, nxt_b = nxt_b, obs_b
    torch.cuda.synchronize()
    assert dones >= 1 and explored >= 1 and greedy >= 1
    assert (a.memory.cursor, a.memory.size) == (b.memory.cursor, b.memory.size)
    for k, (x, y) in enumerate(zip(a.memory.ring, b.memory.ring)):
        assert torch.equal(x, y), ("ring", k)
    assert torch.equal(a.env.state, b.env.state)


def test_graphed_layer_path_equals_eager():
    """update_async: the draw eager, everything behind it (the tree update included) one captured graph."""
    out = []
    for graphs in (False, True):
        tr = _trainer(64, 64, 64, 4096, False, graphs=graphs)
        tr.train(max_vector_steps=12)
        torch.cuda.synchronize()
        out.append(tr)
    assert out[0]._graph is None and out[1]._graph is not None and out[1]._graph.graph is not None
    _assert_same(out[0], out[1])


def _chunk_run(graphs, target_inside, duel, N=64, B=64, hidden=256):
    tr = _trainer(N, B, hidden, 4096, True, graphs=graphs, duel=duel, target_update_freq=4 if target_inside else 10 ** 9)
    assert tr._fused_ok()
    calls, real = [], tr.load_target
    tr.load_target = lambda: (calls.append(tr.optimizer.step_count), real())[1]
    tr.train(max_vector_steps=49)            # one eager step fills the ring, then three chunks of sixteen
    torch.cuda.synchronize()
    return tr, calls


@pytest.mark.parametrize("duel", [False, True])
@pytest.mark.parametrize("target_inside", [False, True])
def test_chunked_graph_equals_eager(target_inside, duel):
    """16 vector steps replay as ONE captured graph, every per-step scalar (push cursor, act counter, epsilon, the draw's counter /
    size / beta, Adam's bias) read from the device record of its step; the hard target copy fires at the same steps."""
    (a, ca), (b, cb) = _chunk_run(False, target_inside, duel), _chunk_run(True, target_inside, duel)
    assert getattr(a, "_chunk", None) is None
    assert b._chunk is not None and b._chunk.graph is not None
    assert b.optimizer.step_count >= 48
    assert ca == cb and (len(ca) >= 1) == target_inside
    _assert_same(a, b)


@pytest.mark.parametrize("duel", [False, True])
def test_checkpoint_loaded_into_a_trainer_with_a_captured_chunk(tmp_path, duel):
    """load_checkpoint() into a trainer whose chunk graph is already captured: the replay takes the new rows' priority from the
    device maximum, which load_state_dict recomputes (the captured graph holds no launch that would).  32 more train() steps
    equal those of a fresh layer-path trainer that loaded the same file."""
    path = str(tmp_path / "ddqn_chunk.pt")
    x = _trainer(64, 64, 64, 4096, True, duel=duel)
    x.train(max_vector_steps=32)               # sixteen eager steps to the tracker's first flush, then one chunk: the graph exists
    assert x._chunk is not None and x._chunk.graph is not None
    x.save_checkpoint(path)
    x.train(max_vector_steps=16)               # everything moves on, the tree's maximum included
    x.load_checkpoint(path)
    y = _trainer(64, 64, 64, 4096, False, graphs=False, duel=duel)
    y.load_checkpoint(path)
    for tr in (x, y):
        tr.train(max_vector_steps=32)
    torch.cuda.synchronize()
    assert y._fused is None and x.optimizer.step_count == 32 + 32
    _assert_same(x, y, "resume")


def test_explicit_stratified_uniforms_keep_the_loop_eager():
    """_parity_v alone (N > 1, graphs on): a chunk replay would draw from Philox instead, so the loop does not chunk."""
    tr = _trainer(64, 64, 64, 4096, True)
    tr._parity_v = iter(_strata(64, 20))
    tr.train(max_vector_steps=20)
    torch.cuda.synchronize()
    assert getattr(tr, "_chunk", None) is None and tr.optimizer.step_count == 20
    assert next(tr._parity_v, None) is None    # every one of the twenty was used


def test_images_change_where_a_value_is_read_not_the_value():
    from gymrl_amd import ops
    b = _run(True, 16, 64, 64, 256, 4096, target_update_freq=10 ** 9)
    c = _run(True, 16, 64, 64, 256, 4096, images=False, target_update_freq=10 ** 9)
    assert b._fused[4] is not None and c._fused[4] is None
    _assert_same(b, c)
    before = b._fused[4].clone()                       # and they do hold the parameters: rebuilding them changes nothing
    ops.ddqn_pack_images(b._fused[1])
    torch.cuda.synchronize()
    assert torch.equal(before, b._fused[4]) and before.abs().sum().item() > 0


@pytest.mark.parametrize("duel", [False, True])
def test_a_row_outside_the_ring_is_a_zero_row_of_weight_zero(duel):
    """ops.ddqn_update's "a row outside the ring is not read: it counts as a zero row of weight 0", which the trainer never
    reaches (it refuses such rows on the host).  Update X carries idx = cap, -1 and 2^31 - 1 under weight 0.7; update Y, from
    the same parameters, moments and target, carries at those places a ring row that IS all zeros, under weight 0: parameters,
    moments, td_out and the loss sum equal bit for bit.  B = 17: two slabs, the second with one live row (an outside one)."""
    from gymrl_amd import ops
    B, H, D, A, cap, r0 = 17, 32, 4, 2, 64, 41
    tr = _trainer(16, B, H, cap, True, duel=duel)
    dev = tr.device
    g = torch.Generator(device="cuda").manual_seed(23)
    rnd = lambda *shape: torch.randn(*shape, generator=g, device=dev)  # noqa: E731
    state, action, reward, nxt, flag = tr.memory.ring
    state.copy_(rnd(cap, D)), nxt.copy_(rnd(cap, D)), reward.copy_(rnd(cap))
    action.copy_((rnd(cap, 1) > 0).to(action.dtype)), flag.copy_((rnd(cap) > 1).to(flag.dtype))
    for t in (state, action, reward, nxt, flag):
        t[r0] = 0
    tr.target_flat.add_(0.05 * rnd(tr.target_flat.numel()))
    tr.optimizer.m.copy_(0.01 * rnd(tr.optimizer.m.numel())), tr.optimizer.v.copy_((0.01 * rnd(tr.optimizer.v.numel())) ** 2)
    start = [t.clone() for t in (tr.flat_params, tr.target_flat, tr.optimizer.m, tr.optimizer.v)]
    rows = torch.randint(0, cap, (B,), generator=g, device=dev, dtype=torch.int32)
    weight = 0.5 + torch.rand(B, generator=g, device=dev)
    outside = {3: cap, 16: -1, 9: 2 ** 31 - 1}

    def update(values, w):
        for dst, src in zip((tr.flat_params, tr.target_flat, tr.optimizer.m, tr.optimizer.v), start):
            dst.copy_(src)
        idx, isw = rows.clone(), weight.clone()
        for b, row in values.items():
            idx[b], isw[b] = row, w
        td, loss = torch.full((B,), 9.0, device=dev), torch.full((1,), 9.0, dtype=torch.float64, device=dev)
        ws = ops.ddqn_update_workspace(B, D, A, H, dev)
        a = ops.ddqn_update_args(B, D, A, tr._layers(tr.policy_net), tr._layers(tr.target_net), tr.optimizer, tr.memory.ring, 0.9, td,
                                 loss, ws, dueling=duel)
        ops.ddqn_update(a, idx, isw, adam_policy=ops.adam_bias(1e-3, 0.9, 0.999, 1))
        torch.cuda.synchronize()
        return [tr.flat_params.clone(), tr.optimizer.m.clone(), tr.optimizer.v.clone(), td, loss]

    x, y = update(outside, 0.7), update({b: r0 for b in outside}, 0.0)
    for name, p, q in zip(("parameters", "m", "v", "td_out", "loss_sum"), x, y):
        assert torch.equal(p, q), (name, p, q)
    assert not torch.equal(x[0], start[0]) and bool((x[3] != 0).any()) and float(x[4]) > 0.0
    assert torch.equal(tr.target_flat, start[1])
