"""DDQN + PER and dueling DDQN + PER (gymrl_amd/ddqn_per_cartpole.py, ddqn_per_duel_cartpole.py) on the GPU: two consecutive
update() calls against the reference's own (tests/golden/ddqn_per_update.npz), the tree against the oracle's sequential loop,
the scalar surface, the checkpoint across the two paths, what the fused step cannot take, and the defaults."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, rel_close

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _mod(prefix):
    from gymrl_amd import ddqn_per_cartpole, ddqn_per_duel_cartpole
    return (ddqn_per_cartpole, "DDQNPERTrainer") if prefix == "ddqn_" else (ddqn_per_duel_cartpole, "DDQNPERDuelTrainer")


def _load(module, g, prefix):
    module.load_state_dict({k[len(prefix):]: torch.from_numpy(np.array(g[k])) for k in g.files if k.startswith(prefix)})


def _maxdiff(module, g, prefix):
    return max(float(np.max(np.abs(v.detach().cpu().numpy() - g[prefix + k]))) for k, v in module.state_dict().items())


@pytest.mark.parametrize("prefix,fused", [("ddqn_", False), ("ddqn_", True), ("duel_", False), ("duel_", True)])
def test_update_matches_reference(oracle, prefix, fused):
    """Tolerances of tests/test_trainers_gpu.py::test_dqn_update_matches_reference: loss 1e-5 * max(1, |loss|), parameters 2e-6."""
    mod, name = _mod(prefix)
    g = load_golden("ddqn_per_update")
    G = lambda k: g[prefix + k]  # noqa: E731
    B = cap = G("indices").shape[1]
    cfg = mod.Config()
    cfg.hidden_dim, cfg.batch_size, cfg.memory_capacity, cfg.gamma, cfg.lr = 32, B, cap, float(G("gamma")), float(G("lr"))
    cfg.fused_step = fused
    tr = getattr(mod, name)(cfg)
    assert tr._fused_update_ok() == fused
    _load(tr.policy_net, g, prefix + "p0_")
    _load(tr.target_net, g, prefix + "t0_")
    dev, m = tr.device, tr.memory
    m.push(torch.from_numpy(G("states")).to(dev), torch.from_numpy(G("actions")).to(dev), torch.from_numpy(G("rewards")).to(dev),
           torch.from_numpy(G("next_states")).to(dev), torch.from_numpy(G("dones")).to(dev))
    assert np.array_equal(m.tree.tree.cpu().numpy(), G("tree0"))
    tr._parity_v = iter([torch.from_numpy(u).to(dev) for u in G("u")])
    ref = oracle.SumTree(cap)
    ref.tree[:] = G("tree0")
    for k in range(2):
        loss = tr.update()
        leaves, _, w, rows = (x.cpu().numpy() for x in m._draws[B])
        assert np.array_equal(leaves, G("indices")[k]) and np.array_equal(rows, leaves - (cap - 1))
        assert rel_close(w, G("is_weight")[k], 1e-6) <= 1e-6
        want = float(G("loss")[k])
        print(prefix, fused, k, "loss", loss, want, "params", _maxdiff(tr.policy_net, g, f"{prefix}p{k + 1}_"))
        assert abs(loss - want) <= 1e-5 * max(1.0, abs(want))
        assert _maxdiff(tr.policy_net, g, f"{prefix}p{k + 1}_") <= 2e-6
        td = tr._last_td.cpu().numpy()
        ref.update_many(idx=leaves, prio=oracle.per_priorities(td, cfg.alpha, cfg.eps, cfg.error_max), idx_is_tree=True)
        tree = m.tree.tree.cpu().numpy()
        assert np.array_equal(tree, ref.tree)                             # the oracle's sequential loop on the GPU's own td
        # against the reference's tree: a leaf is (|td| + eps)^0.6 (or the clip), so its relative error is at most that of
        # |td| + eps, plus the float32 rounding of numpy's power (2e-6: test_oracle_golden_offpolicy.py's bound for variant B)
        err, gerr = np.abs(td) + cfg.eps, G("abs_td")[k].astype(np.float64) + cfg.eps
        tol = 2e-6 + float(np.max(np.abs(err - gerr) / gerr))
        print(prefix, fused, k, "td rel", tol - 2e-6, "tree rel", rel_close(tree, G("tree")[k], tol))
        assert rel_close(tree, G("tree")[k], tol) <= tol
        assert cfg.beta == float(G("beta")[k])
    assert (tr._fused is not None) == fused and (tr._fused is None or tr._fused[1].dueling == (prefix == "duel_"))


@pytest.mark.parametrize("prefix", ["ddqn_", "duel_"])
def test_scalar_surface_and_public_buffer(prefix):
    """select_action(np.ndarray) -> int; push(tuple) at num_envs = 1; sample() hands out TREE indices that update_priorities takes."""
    mod, name = _mod(prefix)
    cfg = mod.Config()
    cfg.hidden_dim, cfg.batch_size, cfg.memory_capacity, cfg.seed = 32, 8, 50, 3
    tr = getattr(mod, name)(cfg)
    a = tr.select_action(np.zeros(4, np.float32))
    assert isinstance(a, int) and a in (0, 1)
    m, rng = tr.memory, np.random.default_rng(0)
    for i in range(12):
        m.push((rng.normal(size=4).astype(np.float32), int(i % 2), 1.0, rng.normal(size=4).astype(np.float32), False))
    assert len(m) == 12 and float(m.tree.total_priority()) == 12.0       # max(leaves) = 1.0 from the first push on
    batch, indices, w = m.sample(8)
    assert cfg.beta == 0.401 and indices.dtype == torch.int32 and w.dtype == torch.float32
    idx = indices.cpu().numpy()
    assert idx.min() >= 49 and idx.max() < 49 + 12 and tuple(batch[0].shape) == (8, 4)
    m.update_priorities(idx, np.full(8, 0.5, np.float32))
    leaves = m.tree.tree.cpu().numpy()[49:]
    assert np.allclose(leaves[np.unique(idx) - 49], (0.5 + 1e-4) ** 0.6, rtol=1e-6) and leaves[:12].max() == 1.0
    m.update_priorities(indices, torch.full((8,), 7.0))                  # clipped at error_max = 1
    assert m.tree.tree.cpu().numpy()[49:].max() == 1.0
    assert tr.update() != 0.0 and tr.optimizer.step_count == 1


def _trainer(prefix, N, B, hidden, fused, graphs=False, cap=4096, **more):
    mod, name = _mod(prefix)
    cfg = mod.Config()
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed, cfg.memory_capacity = N, B, hidden, 5, cap
    cfg.max_episodes, cfg.fused_step, cfg.use_graphs = 10 ** 9, fused, graphs
    for k, v in more.items():
        setattr(cfg, k, v)
    return getattr(mod, name)(cfg)


def _assert_same(a, b, what=""):
    assert a.optimizer.step_count == b.optimizer.step_count, what
    assert (a.memory.cursor, a.memory.size, a.memory.draws) == (b.memory.cursor, b.memory.size, b.memory.draws), what
    assert (a._act_counter, a.sample_count, a.epsilon, a.cfg.beta) == (b._act_counter, b.sample_count, b.epsilon, b.cfg.beta), what
    for k, (x, y) in enumerate(zip(a.memory.ring, b.memory.ring)):
        assert torch.equal(x, y), (what, "ring", k)
    assert torch.equal(a.memory.tree.tree, b.memory.tree.tree), what
    for name in ("flat_params", "target_flat", "_loss"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    assert torch.equal(a.optimizer.m, b.optimizer.m) and torch.equal(a.optimizer.v, b.optimizer.v), what
    assert list(a.episode_rewards) == list(b.episode_rewards), what


@pytest.mark.parametrize("prefix,src_fused", [("ddqn_", True), ("ddqn_", False), ("duel_", True), ("duel_", False)])
def test_checkpoint_saved_on_one_path_resumes_on_the_other(tmp_path, prefix, src_fused):
    """Saved mid-run on one path, resumed on the other: after 16 more update steps the tree, ring, parameters, moments and beta
    equal those of the run that was never interrupted."""
    path = str(tmp_path / "ddqn.pt")
    whole = _trainer(prefix, 48, 64, 64, src_fused)
    whole.train(max_vector_steps=10)
    whole.save_checkpoint(path)
    resumed = _trainer(prefix, 48, 64, 64, not src_fused)
    resumed.load_checkpoint(path)
    assert resumed.cfg.beta == whole.cfg.beta > 0.4 and torch.equal(resumed.memory.tree.tree, whole.memory.tree.tree)
    for _ in range(16):
        whole.update()
        resumed.update()
    torch.cuda.synchronize()
    assert (whole._fused is not None) == src_fused and (resumed._fused is not None) != src_fused
    assert whole.optimizer.step_count == 9 + 16
    _assert_same(whole, resumed, "resume")


@pytest.mark.parametrize("B,more", [(300, {}), (64, {"max_steps": 200}), (64, {"updates_per_step": 2})])
def test_what_the_step_cannot_take_trains_layer_by_layer(B, more):
    out = []
    for fused in (True, False):
        tr = _trainer("ddqn_", 64, B, 64, fused, **more)
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
    tr = _trainer("ddqn_", 64, 300, 64, True)
    tr.train(max_vector_steps=6)
    m = tr.memory
    ws = ops.ddqn_update_workspace(300, 4, 2, 64, tr.device)
    for B in (300, 257):
        td = torch.zeros(B, device=tr.device)
        a = ops.ddqn_update_args(B, 4, 2, tr._layers(tr.policy_net), tr._layers(tr.target_net), tr.optimizer, m.ring, 0.9, td, tr._loss, ws)
        rows, w = torch.zeros(B, dtype=torch.int32, device=tr.device), torch.ones(B, device=tr.device)
        before = tr.flat_params.clone()
        with pytest.raises(RuntimeError, match="-22"):
            ops.ddqn_update(a, rows, w, adam_policy=ops.adam_bias(1e-3, 0.9, 0.999, 1))
        rc = _lib.lib().gymrl_ddqn_update(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == -22 and torch.equal(before, tr.flat_params)


@pytest.mark.parametrize("prefix", ["ddqn_", "duel_"])
def test_defaults_never_build_the_fused_step(prefix):
    mod, name = _mod(prefix)
    cfg = mod.Config()
    cfg.num_envs, cfg.hidden_dim, cfg.seed, cfg.memory_capacity = 32, 32, 1, 1024
    tr = getattr(mod, name)(cfg)
    assert not tr._fused_update_ok() and not tr._fused_ok()
    tr.train(max_vector_steps=6)           # the graphed layer path (use_graphs defaults to True)
    tr.update()
    torch.cuda.synchronize()
    assert tr._fused is None and getattr(tr, "_chunk", None) is None and tr.optimizer.step_count == 6


def test_explicit_rows_outside_the_ring_are_refused():
    """update(indices=...) is checked on the host before anything is launched: the ring and the tree are indexed by these rows."""
    tr = _trainer("ddqn_", 48, 16, 32, True, cap=64)
    tr.train(max_vector_steps=1)
    before, steps = tr.memory.tree.tree.clone(), tr.optimizer.step_count
    for bad in (64, -3):
        rows = torch.arange(16, dtype=torch.int32, device=tr.device)
        rows[5] = bad
        with pytest.raises(ValueError):
            tr.update(indices=rows)
    assert tr.optimizer.step_count == steps and torch.equal(before, tr.memory.tree.tree)
