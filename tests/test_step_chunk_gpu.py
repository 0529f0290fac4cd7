"""Per-step scalars on the device (the `*_dev` arguments of include/gymrl.h) and whole vector steps replayed as one
hipGraph per 16 (gymrl_amd/graphs.py StepChunk): every device-argument launch equals its host-argument twin bit for
bit, and the chunked train loops reproduce the eager loops bit for bit."""
import struct

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _dev_bytes(fmt, *vals):
    return torch.frombuffer(bytearray(struct.pack("=" + fmt, *vals)), dtype=torch.uint8).cuda()


def test_store_scalars_large_block():
    from gymrl_amd import ops
    blk = torch.zeros(3840, dtype=torch.uint8, device="cuda")
    payload = bytes((7 * i + 3) % 251 for i in range(3840))
    ops.store_scalars(blk, payload)
    assert bytes(blk.cpu().numpy().tobytes()) == payload
    ops.store_scalars(blk, payload[:1000])
    assert bytes(blk.cpu().numpy().tobytes()) == payload
    with pytest.raises(RuntimeError):
        ops.store_scalars(torch.zeros(4096, dtype=torch.uint8, device="cuda"), bytes(3844))


def test_ring_ops_read_their_cursors_from_the_device():
    from gymrl_amd import ops
    g = torch.Generator().manual_seed(1)
    cap, D, n = 64, 3, 10
    src = (torch.randn(n, D, generator=g).cuda(), torch.randint(0, 9, (n, 1), generator=g, dtype=torch.int32).cuda(),
           torch.randn(n, generator=g).cuda(), torch.randn(n, D, generator=g).cuda(),
           torch.randint(0, 2, (n,), generator=g, dtype=torch.uint8).cuda())
    rings = []
    for use_dev in (False, True):
        ring = (torch.zeros(cap, D, device="cuda"), torch.zeros(cap, 1, dtype=torch.int32, device="cuda"),
                torch.zeros(cap, device="cuda"), torch.zeros(cap, D, device="cuda"),
                torch.zeros(cap, dtype=torch.uint8, device="cuda"))
        if use_dev:
            ops.replay_append(ring, 0, *src, cursor_dev=_dev_bytes("q", 59))        # wraps; the host cursor (0) is ignored
        else:
            ops.replay_append(ring, 59, *src)
        rings.append(ring)
    for a, b in zip(*rings):
        assert torch.equal(a, b)
    for size, B in ((64, 16), (1000, 128), (37, 37)):
        host = ops.uniform_indices(5, 12345, size, B, "cuda")
        dev = ops.uniform_indices(5, 0, 1 << 20, B, "cuda", dev=_dev_bytes("Qq", 12345, size))
        assert torch.equal(host, dev)
        assert len(set(host.tolist())) == B and int(host.max()) < size


@pytest.mark.parametrize("pushes,cursor", [(0, 0), (2, 0), (7, 24), (9, 56)])
def test_nstep_push_device_cursors_and_inline_terminal(pushes, cursor):
    from gymrl_amd import ops
    g = torch.Generator().manual_seed(pushes + 3)
    n_steps, N, D, cap, limit = 3, 8, 4, 64, 14
    outs = []
    done = torch.randint(0, 2, (N,), generator=g, dtype=torch.uint8).cuda()
    ep_len = torch.randint(12, 15, (N,), generator=g, dtype=torch.int32).cuda()
    terminal = (done.bool() & (ep_len != limit)).to(torch.uint8)
    obs, nxt = torch.randn(N, D, generator=g).cuda(), torch.randn(N, D, generator=g).cuda()
    act = torch.randint(0, 2, (N,), generator=g, dtype=torch.int32).cuda()
    rew = torch.randn(N, generator=g).cuda()
    win0 = (torch.randn(n_steps, N, D, generator=g).cuda(), torch.randint(0, 2, (n_steps, N), generator=g, dtype=torch.int32).cuda(),
            torch.randn(n_steps, N, generator=g).cuda(), torch.randn(n_steps, N, D, generator=g).cuda(),
            torch.randint(0, 2, (n_steps, N), generator=g, dtype=torch.uint8).cuda(),
            torch.randint(0, 2, (n_steps, N), generator=g, dtype=torch.uint8).cuda())
    for use_dev in (False, True):
        win = tuple(t.clone() for t in win0)
        ring = (torch.zeros(cap, D, device="cuda"), torch.zeros(cap, 1, dtype=torch.int32, device="cuda"),
                torch.zeros(cap, device="cuda"), torch.zeros(cap, D, device="cuda"),
                torch.zeros(cap, dtype=torch.uint8, device="cuda"))
        if use_dev:
            ops.nstep_push(win, n_steps, n_steps, 0.99, obs, act, rew, nxt, None, done, ring, 0,
                           dev=_dev_bytes("2q", pushes, cursor), ep_len=ep_len, max_episode_steps=limit)
        else:
            emitted = ops.nstep_push(win, n_steps, pushes, 0.99, obs, act, rew, nxt, terminal, done, ring, cursor)
            assert emitted == (pushes + 1 >= n_steps)
        outs.append(win + ring)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_sum_tree_device_cursor_and_draw_record():
    from gymrl_amd import ops
    cap, N, B = 1 << 10, 64, 32
    g = torch.Generator().manual_seed(2)
    tree0 = torch.zeros(2 * cap - 1, dtype=torch.float64)
    leaves = torch.rand(cap, generator=g, dtype=torch.float64) + 0.1
    tree0[cap - 1:] = leaves
    for i in range(cap - 2, -1, -1):
        tree0[i] = tree0[2 * i + 1] + tree0[2 * i + 2]
    pr = torch.tensor([1.75], dtype=torch.float64, device="cuda")
    for start in (0, 128, cap - N):
        trees = []
        for use_dev in (False, True):
            tree = tree0.clone().cuda()
            ws = ops.per_workspace(N, tree.device)
            if use_dev:
                ops.per_update(tree, cap, N, ws, prio_scalar_dev=pr, idx_start_dev=_dev_bytes("q", start))
            else:
                ops.per_update(tree, cap, N, ws, idx_start=start, prio_scalar_dev=pr)
            trees.append(tree)
        assert torch.equal(*trees), start
    tree = tree0.clone().cuda()
    ws = ops.per_workspace(B, tree.device)
    host = ops.per_sample(tree, cap, B, 700, 0.45, ws, seed=9, counter=77)
    host = [t.clone() for t in host]
    dev = ops.per_sample(tree, cap, B, 1, 0.0, ws, seed=9, dev=_dev_bytes("Qqd", 77, 700, 0.45))
    for a, b in zip(host, dev):
        assert torch.equal(a, b)


def test_noisy_noise_counter_from_device_and_drawn_inside_combine():
    """gymrl_noisy_noise(counter_dev) == (counter); gymrl_noisy_combine with draw builds W = mu + sigma * eps from the
    very values gymrl_noisy_noise writes, leaves them in the module's buffers, and honours per-layer eval."""
    from gymrl_amd import ops
    K, g = 48, torch.Generator().manual_seed(4)
    layers = []
    for n_out, seed, counter in ((3, 11, 5), (1, 12, 6), (2, 13, 1 << 33)):
        w_eps, b_eps = torch.empty(n_out, K, device="cuda"), torch.empty(n_out, device="cuda")
        ops.noisy_noise(K, n_out, w_eps, b_eps, seed=seed, counter=counter)
        w2, b2 = torch.empty_like(w_eps), torch.empty_like(b_eps)
        ops.noisy_noise(K, n_out, w2, b2, seed=seed, counter_dev=_dev_bytes("Q", counter))
        assert torch.equal(w_eps, w2) and torch.equal(b_eps, b2)
        layers.append(dict(w_mu=torch.randn(n_out, K, generator=g).cuda(), w_sigma=torch.rand(n_out, K, generator=g).cuda(),
                           b_mu=torch.randn(n_out, generator=g).cuda(), b_sigma=torch.rand(n_out, generator=g).cuda(),
                           seed=seed, counter=counter, want_w=w_eps, want_b=b_eps))
    read = [dict(L, w_eps=L["want_w"], b_eps=L["want_b"]) for L in layers]
    W0, b0 = ops.noisy_combine(read, training=True)
    copies = [(torch.zeros_like(L["want_w"]), torch.zeros_like(L["want_b"])) for L in layers]
    drawn = [dict(L, draw=True, w_eps_copy=c[0], b_eps_copy=c[1]) for L, c in zip(layers, copies)]
    drawn[2]["counter"], drawn[2]["counter_dev"] = 0, _dev_bytes("Q", layers[2]["counter"])
    W1, b1 = ops.noisy_combine(drawn, training=True)
    assert torch.equal(W0, W1) and torch.equal(b0, b1)
    for L, c in zip(layers, copies):
        assert torch.equal(c[0], L["want_w"]) and torch.equal(c[1], L["want_b"])
    ref = torch.cat([L["w_mu"] + L["w_sigma"] * L["want_w"] for L in layers])
    assert torch.equal(W0, ref)
    mixed = [dict(read[0]), dict(read[1], eval=True), dict(read[2])]
    W2, b2 = ops.noisy_combine(mixed, training=True)
    assert torch.equal(W2[3:4], layers[1]["w_mu"]) and torch.equal(b2[3:4], layers[1]["b_mu"])
    assert torch.equal(W2[:3], W0[:3]) and torch.equal(W2[4:], W0[4:])


def test_dueling_epilogue_greedy_action():
    from gymrl_amd import ops
    g = torch.Generator().manual_seed(6)
    for B, K, A in ((100, 64, 2), (257, 32, 5), (16, 8, 15)):
        x = torch.randn(B, K, generator=g).cuda()
        W = (torch.randn(A + 1, K, generator=g) / K ** 0.5).cuda()
        b = torch.randn(A + 1, generator=g).cuda()
        W[0] = W[1]                                   # ties between the first two actions: argmax keeps the first
        b[0] = b[1]
        act = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        q = ops.lin_fwd(x, W, b, ops.LIN_ACT["dueling"], argmax=act)
        s = x.double() @ W.double().t() + b.double()
        ref = s[:, A:] + s[:, :A] - s[:, :A].mean(1, keepdim=True)
        assert float((q.double() - ref).abs().max()) <= 5e-6 * float(ref.abs().max())
        assert torch.equal(act.long(), q.argmax(1))
        assert int(act.min()) >= 0 and bool((q[:, 0] == q[:, 1]).all())


def _train(mod, cls, steps, **over):
    cfg = mod.Config()
    cfg.num_envs, cfg.max_episodes, cfg.batch_size, cfg.seed = 64, 10**9, 128, 5
    for k, v in over.items():
        setattr(cfg, k, v)
    torch.manual_seed(11)
    tr = getattr(mod, cls)(cfg)
    tr.train(max_vector_steps=steps)
    torch.cuda.synchronize()
    return tr


# (64 / 128 / 256: the default shape; 256 / 128 / 256: sixteen full acting workgroups; 4100 / 256 / 256: a partial last acting
#  workgroup, a full set of slabs at B = 256, and the ring wraps; 40 / 24 / 32: a hidden width without weight images and
#  without the 256-wide instances.  Updates start once the ring holds a batch — after ceil(B / N) <= 2 vector steps here)
@pytest.mark.parametrize("N,B,hidden,steps", [(64, 128, 256, 70), (256, 128, 256, 64), (4100, 256, 256, 64), (40, 24, 32, 64)])
def test_sac_chunked_vector_steps_equal_eager(N, B, hidden, steps):
    from gymrl_amd import sac_pendulum
    shape = dict(num_envs=N, batch_size=B, hidden_dim=hidden, memory_capacity=1 << 14)
    eager = _train(sac_pendulum, "SACTrainer", steps, use_graphs=False, **shape)
    chunk = _train(sac_pendulum, "SACTrainer", steps, use_graphs=True, chunk_steps=16, **shape)
    assert eager._fused_ok() and chunk._fused_ok()
    assert chunk._chunk.graph is not None and getattr(eager, "_chunk", None) is None      # 3-4 chunks of 16 replayed
    assert chunk.critic_optimizer.step_count == eager.critic_optimizer.step_count > steps - 10 >= 48
    for name in ("actor_flat", "critic_flat", "critic_target_flat", "log_alpha", "_alpha_m", "_alpha_v", "_sums"):
        assert torch.equal(getattr(eager, name), getattr(chunk, name)), (N, B, hidden, name)
    assert all(torch.isfinite(getattr(chunk, n)).all() for n in ("actor_flat", "critic_flat", "log_alpha"))
    for a, b in zip(eager.memory.ring, chunk.memory.ring):
        assert torch.equal(a, b)
    assert (eager.memory.cursor, eager.memory.size, eager.memory.draws) == (chunk.memory.cursor, chunk.memory.size, chunk.memory.draws)
    assert list(eager.episode_rewards) == list(chunk.episode_rewards)


def test_rainbow_chunked_vector_steps_equal_eager():
    from gymrl_amd import rainbow_dqn_cartpole as rb
    outs = []
    for over in (dict(use_graphs=False), dict(use_graphs=True, chunk_steps=16), dict(use_graphs=True, chunk_steps=0)):
        rb.NoisyLinear._counter = 0
        outs.append(_train(rb, "RainbowDQNTrainer", 70, memory_capacity=1 << 12, **over))     # the ring wraps once
    eager, chunk, per_update = outs
    assert chunk._chunk.graph is not None and getattr(per_update, "_chunk", None) is None
    for tr in (chunk, per_update):
        assert tr.optimizer.step_count == eager.optimizer.step_count > 60
        assert torch.equal(eager.flat_params, tr.flat_params) and torch.equal(eager.target_flat, tr.target_flat)
        assert torch.equal(eager.memory.sum_tree.tree, tr.memory.sum_tree.tree)
        for a, b in zip(eager.memory.ring, tr.memory.ring):
            assert torch.equal(a, b)
        assert eager.optimizer.param_groups[0]["lr"] == tr.optimizer.param_groups[0]["lr"]
        assert (eager.total_steps, eager.memory.count, eager.memory.draws) == (tr.total_steps, tr.memory.count, tr.memory.draws)
        for name in ("advantage", "value"):
            assert torch.equal(getattr(eager.policy_net, name).weight_epsilon, getattr(tr.policy_net, name).weight_epsilon)
        assert list(eager.episode_rewards) == list(tr.episode_rewards)
