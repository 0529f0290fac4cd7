"""The fused NoisyNet dueling DQN vector step (csrc/noisy_dqn_step.hip: combine, act, rows, tiles, split + Adam) against the
layer-by-layer path it replaces, and its combine kernel alone against gymrl_noisy_noise + torch: same seeds -> every parameter
(mu and sigma), Adam moment, the target, the loss sum, the replay ring, the env state and every host counter equal BIT FOR BIT."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noisy_dqn_update.npz")


def _trainer(N, B, hidden, cap, fused, graphs=None, seed=5, **more):
    from gymrl_amd import noisy_dqn_cartpole as m
    cfg = m.Config()
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed, cfg.memory_capacity = N, B, hidden, seed, cap
    cfg.max_episodes, cfg.fused_step = 10 ** 9, fused
    if graphs is not None:
        cfg.use_graphs = graphs
    for k, v in more.items():
        setattr(cfg, k, v)
    return m.NoisyDQNTrainer(cfg)


def _assert_same(a, b, what=""):
    assert a.optimizer.step_count == b.optimizer.step_count, what
    assert (a.memory.cursor, a.memory.size, a.memory.draws) == (b.memory.cursor, b.memory.size, b.memory.draws), what
    assert (a.learn_step, a.noise_draws) == (b.learn_step, b.noise_draws), what
    for k, (x, y) in enumerate(zip(a.memory.ring, b.memory.ring)):
        assert torch.equal(x, y), (what, "ring", k)          # acting: same noise, same actions, same physics, same rows
    assert torch.equal(a.env.state, b.env.state), (what, "env")
    for name in ("flat_params", "target_flat", "_loss"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    assert torch.equal(a.optimizer.m, b.optimizer.m) and torch.equal(a.optimizer.v, b.optimizer.v), what
    assert list(a.episode_rewards) == list(b.episode_rewards), what


# (N, B, hidden, capacity, steps): one slab each; a partial slab in both phases; the largest batch (16 slabs).  The capacity is
# no multiple of N, so a push wraps the ring; target_update_freq = 3 puts hard copies inside the run.
SHAPES = [(16, 16, 32, 72, 8), (40, 24, 64, 100, 8), (64, 256, 64, 300, 10)]


@pytest.mark.parametrize("N,B,hidden,cap,steps", SHAPES)
def test_fused_step_equals_layer_by_layer(N, B, hidden, cap, steps):
    out = []
    for fused in (False, True):
        tr = _trainer(N, B, hidden, cap, fused, graphs=False, target_update_freq=3)
        assert tr._fused_ok() == fused
        copies, real = [], tr.load_target
        tr.load_target = lambda tr=tr, copies=copies, real=real: (copies.append(tr.learn_step), real())[1]
        tr.train(max_vector_steps=steps)
        torch.cuda.synchronize()
        out.append((tr, copies))
    (a, ca), (b, cb) = out
    assert a._fused is None and b._fused is not None
    assert b.optimizer.step_count >= 3 and ca == cb and len(ca) >= 1
    assert b.memory.size == cap and b.memory.cursor == (N * steps) % cap      # the ring wrapped
    sigma = b.policy_net.fc2.weight_sigma.detach()
    assert not torch.equal(sigma, torch.full_like(sigma, float(sigma.flatten()[0])))      # sigma is learning
    assert not torch.equal(b.flat_params, b.target_flat)
    _assert_same(a, b)


def test_combine_kernel_equals_noisy_noise_plus_torch():
    """One (seed, counter) per layer and set: eps and effective parameters equal gymrl_noisy_noise and mu + sigma * eps formed in
    torch, bit for bit, for all three sets; set A's eps vectors are kept."""
    from gymrl_amd import ops
    tr = _trainer(16, 16, 36, 64, True)
    net = tr.policy_net
    with torch.no_grad():                     # parameters that are no constants: mu + sigma * eps exercises every element
        g = torch.Generator(device="cuda").manual_seed(3)
        tr.flat_params.add_(0.05 * torch.randn(tr.flat_params.shape, generator=g, device="cuda"))
    _, _, ws, _, comb = tr._fused_args()
    counters = (11, 2 ** 33 + 5, 7)
    ops.ndqn_combine(comb, counters=counters)
    torch.cuda.synchronize()
    base = (ws.data_ptr() + 255) // 256 * 256 - ws.data_ptr()
    flat = ws[base:base + (ws.numel() - base) // 4 * 4].view(torch.float32)
    o = 0
    pad = lambda n: (n + 63) // 64 * 64       # noqa: E731  (the workspace hands out 256-byte aligned arrays)
    eps_a = []
    for s in range(3):
        for name in ops.NDQN_LAYERS:
            m = getattr(net, name)
            w_eps, b_eps = torch.empty_like(m.weight_epsilon), torch.empty_like(m.bias_epsilon)
            ops.noisy_noise(m.in_features, m.out_features, w_eps, b_eps, seed=m.seed, counter=counters[s])
            W = m.weight_mu + m.weight_sigma.mul(w_eps)
            b = m.bias_mu + m.bias_sigma.mul(b_eps)
            nw, nb = W.numel(), b.numel()
            assert torch.equal(flat[o:o + nw].view_as(W), W), (s, name)
            o += pad(nw)
            assert torch.equal(flat[o:o + nb], b), (s, name)
            o += pad(nb)
            if s == 1:
                eps_a.append((w_eps, b_eps))
    for name, (w_eps, b_eps) in zip(ops.NDQN_LAYERS, eps_a):
        m = getattr(net, name)
        ein = flat[o:o + m.in_features]
        o += pad(m.in_features)
        eout = flat[o:o + m.out_features]
        o += pad(m.out_features)
        assert torch.equal(eout, b_eps) and torch.equal(torch.outer(eout, ein), w_eps), name
        o += pad(m.in_features * m.out_features) + pad(m.out_features)      # the gradient slots


def test_combine_kernel_on_raw_draws_equals_the_goldens_effective_weights():
    """Raw draws in: W = mu + sigma * f(out) f(in).  Against float64 numpy from the golden's raw vectors the bound is the
    arithmetic's: f is a correctly rounded sqrt (0.5 ulp), the outer product one multiply, then one multiply and one add —
    four roundings of values below |mu| + |sigma| eps^2 <= 4: 4 * 2^-24 * 4 < 1e-6."""
    from gymrl_amd import ops
    g = np.load(GOLDEN)
    H, D = g["p0_fc1.weight_mu"].shape
    tr = _trainer(16, 32, H, 64, True)
    tr.policy_net.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("p0_")})
    _, _, ws, _, comb = tr._fused_args()
    L = ops.ndqn_raw_len(D, 2, H)
    rows = [torch.from_numpy(r.copy()).cuda() for r in (g["act_raw"], g["raw"][0][:L], g["raw"][0][L:])]
    ops.ndqn_combine(comb, raw=rows)
    torch.cuda.synchronize()
    base = (ws.data_ptr() + 255) // 256 * 256 - ws.data_ptr()
    flat = ws[base:base + (ws.numel() - base) // 4 * 4].view(torch.float32).cpu().numpy()
    pad = lambda n: (n + 63) // 64 * 64       # noqa: E731
    f = lambda x: np.sign(x) * np.sqrt(np.abs(x))      # noqa: E731
    o = 0
    for s in range(3):
        raw, ro = rows[s].cpu().numpy().astype(np.float64), 0
        for name in ops.NDQN_LAYERS:
            mu, sg = g[f"p0_{name}.weight_mu"].astype(np.float64), g[f"p0_{name}.weight_sigma"].astype(np.float64)
            n, k = mu.shape
            ei, eo = f(raw[ro:ro + k]), f(raw[ro + k:ro + k + n])
            ro += k + n
            W = mu + sg * np.outer(eo, ei)
            b = g[f"p0_{name}.bias_mu"].astype(np.float64) + g[f"p0_{name}.bias_sigma"].astype(np.float64) * eo
            assert np.abs(flat[o:o + n * k].reshape(n, k) - W).max() < 1e-6, (s, name)
            o += pad(n * k)
            assert np.abs(flat[o:o + n] - b).max() < 1e-6, (s, name)
            o += pad(n)


def _chunk_run(graphs, freq, N=64, B=64, hidden=64):
    tr = _trainer(N, B, hidden, 4096, True, graphs=graphs, target_update_freq=freq)
    assert tr._fused_ok()
    calls, real = [], tr.load_target
    tr.load_target = lambda: (calls.append(tr.learn_step), real())[1]
    tr.train(max_vector_steps=48)
    torch.cuda.synchronize()
    return tr, calls


def test_chunked_graph_equals_eager_with_the_target_copy_inside():
    """16 vector steps replay as ONE captured graph, every per-step scalar (push cursor, the three draw counters, the index
    draw's counter / size, Adam's bias) read from the device record of its step; the hard target copy is a node of the graph."""
    (a, ca), (b, cb) = _chunk_run(False, 5), _chunk_run(True, 5)
    assert not a._chunks and len(b._chunks) >= 2 and all(c.graph is not None for c in b._chunks.values())
    assert b.optimizer.step_count == 48 and len(ca) == 9
    assert len(cb) >= 1                       # (a replayed copy runs no Python: only the captures are counted)
    _assert_same(a, b)


def test_checkpoint_loaded_into_a_trainer_with_a_captured_chunk(tmp_path):
    path = str(tmp_path / "ndqn_chunk.pt")
    x = _trainer(64, 64, 64, 4096, True, target_update_freq=7)
    x.train(max_vector_steps=32)
    assert x._chunks and all(c.graph is not None for c in x._chunks.values())
    x.save_checkpoint(path)
    x.train(max_vector_steps=16)
    x.load_checkpoint(path)
    y = _trainer(64, 64, 64, 4096, False, graphs=False, target_update_freq=7)
    y.load_checkpoint(path)
    for tr in (x, y):
        tr.train(max_vector_steps=32)
    torch.cuda.synchronize()
    assert y._fused is None and x.optimizer.step_count == 32 + 32
    _assert_same(x, y, "resume")


def test_explicit_raw_draws_keep_the_loop_eager():
    from gymrl_amd import ops
    tr = _trainer(64, 64, 64, 4096, True)
    g = torch.Generator(device="cuda").manual_seed(2)
    L = ops.ndqn_raw_len(4, 2, 64)
    tr._parity_raw_act = iter([torch.randn(L, generator=g, device="cuda") for _ in range(20)])
    tr.train(max_vector_steps=20)
    torch.cuda.synchronize()
    assert not tr._chunks and tr.optimizer.step_count == 20 and next(tr._parity_raw_act, None) is None


def test_trainer_falls_back_for_refused_shapes():
    """H % 4 != 0 and A = 3 (a scripted env in the trainer's place of CartPole) are shapes the entry points refuse: the trainer
    stays on the layer path instead of raising."""
    from scripted_env import ScriptedVecEnv
    tr = _trainer(16, 16, 22, 64, True, graphs=False)
    assert not tr._fused_update_ok() and not tr._fused_ok()
    tr.train(max_vector_steps=3)
    torch.cuda.synchronize()
    assert tr._fused is None and tr.optimizer.step_count == 3
    tr = _trainer(16, 16, 32, 64, True)
    assert tr._fused_ok()
    tr.env, tr.action_dim = ScriptedVecEnv(16, tr.device, obs_dim=4, n_actions=3), 3
    assert not tr._fused_update_ok() and not tr._fused_ok()
