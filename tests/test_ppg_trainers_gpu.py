"""GPU checks of the PPG-RNN / PPO-RNN trainers: _GRUSeq's gradients against a float64 nn.GRU, a real-LunarLander run of
rounds + one update (finite metrics, stored episodes end where the env's did, per-range Adam step counts, a bit-exact
save -> load continuation), and the configuration checks.

Tolerance of the _GRUSeq check: f32 kernels against float64 over episodes of <= 9 steps, H = 64: 1e-4 relative + 1e-5
absolute (the gate sums run in f32; test_gru_seq_gpu.py pins the kernels themselves)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def test_gru_seq_autograd_against_float64_nn_gru():
    from gymrl_amd.ppg_rnn_lunarlander import _Episodes, _GRUSeq
    import torch.nn.functional as F
    torch.manual_seed(0)
    lens = [5, 1, 9]
    M = sum(lens)
    gru = torch.nn.GRU(256, 64)
    x = torch.randn(M, 256)
    R = torch.randn(M, 64)
    # float64 reference, one unbatched episode per call from h = 0
    g64 = torch.nn.GRU(256, 64).double()
    g64.load_state_dict({k: v.double() for k, v in gru.state_dict().items()})
    x64 = x.double().requires_grad_(True)
    outs, o = [], 0
    for n in lens:
        outs.append(g64(x64[o:o + n], torch.zeros(1, 64, dtype=torch.float64))[0])
        o += n
    (torch.cat(outs) * R.double()).sum().backward()
    # the HIP path
    g = gru.cuda()
    xc = x.cuda().requires_grad_(True)
    eps = _Episodes(lens, "cuda")
    gi = eps.to_time_major(F.linear(xc, g.weight_ih_l0, g.bias_ih_l0))
    h = eps.to_flat(_GRUSeq.apply(gi, g.weight_hh_l0, g.bias_hh_l0, eps.lengths))
    (h * R.cuda()).sum().backward()
    tol = dict(rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(h.detach().cpu().numpy(), torch.cat(outs).detach().numpy(), **tol)
    np.testing.assert_allclose(xc.grad.cpu().numpy(), x64.grad.numpy(), **tol)
    for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
        np.testing.assert_allclose(getattr(g, n).grad.cpu().numpy(), getattr(g64, n).grad.numpy(), err_msg=n, **tol)


def _cfg(tmp_path, mod, **kw):
    cfg = mod.Config()
    cfg.num_envs, cfg.batch_size, cfg.episodes_per_minibatch, cfg.epochs = 16, 16, 4, 1
    if hasattr(cfg, "aux_epochs"):
        cfg.aux_epochs = 1
    cfg.seed, cfg.max_episodes = 3, 16
    cfg.save_path = str(tmp_path / "ck.pth")
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_batch_size_must_divide():
    from gymrl_amd import ppg_rnn_lunarlander as ppg
    cfg = ppg.Config()
    cfg.num_envs, cfg.batch_size = 3, 4
    with pytest.raises(ValueError):
        ppg.PPGTrainer(cfg)
    cfg.num_envs, cfg.episodes_per_minibatch = 2, 3
    with pytest.raises(ValueError):
        ppg.PPGTrainer(cfg)


def test_ppg_lunarlander_round_update_and_checkpoint(tmp_path):
    from gymrl_amd import ppg_rnn_lunarlander as ppg
    cfg = _cfg(tmp_path, ppg)
    tr = ppg.PPGTrainer(cfg)
    returns, lengths = tr.collect_round()
    assert len(returns) == 16 and np.isfinite(returns).all()
    b = tr.sample()
    assert b["lengths"] == lengths and sum(lengths) == b["states"].shape[0]
    done = b["done"].cpu().numpy()
    for e, n in enumerate(lengths):            # every stored episode ends at its env's done (or the step cap), not later
        o = b["offsets"][e]
        assert 1 <= n <= 1000
        assert done[o:o + n - 1].sum() == 0
        assert done[o + n - 1] == 1 or n == 1000
    perms = [np.random.RandomState(k).permutation(16) for k in range(4)]
    tr._parity_perms = iter(perms[:2])
    tr.grad_norms = []
    m = tr.update()
    assert all(np.isfinite(v) for v in m.values()), m
    assert len(tr.grad_norms) == 8 and np.isfinite(tr.grad_norms).all()
    # the policy phase stepped critic + trunk (4 times), the aux phase trunk + aux (4 times): the critic did not advance
    assert tr.optimizer.steps == {"critic": 4, "trunk": 8, "aux": 4}
    steps = dict(zip([n for n, _ in tr.net.named_parameters()], tr.param_steps()))
    assert steps["critic_fc.mlp.0.weight"] == 4 and steps["rnn.rnn.weight_hh_l0"] == 8 and steps["aux_critic_fc.mlp.2.bias"] == 4
    tr.save_model()
    ck = torch.load(cfg.save_path, weights_only=False)
    assert set(ck) >= {"net_state_dict", "optimizer_state_dict", "learn_step", "state_norm"} and ck["learn_step"] == 1
    st = ck["optimizer_state_dict"]["state"]
    assert sorted({int(v["step"]) for v in st.values()}) == [4, 8]
    # a fresh trainer loads the checkpoint and continues bit-exactly on the same batch and permutations
    tr2 = ppg.PPGTrainer(_cfg(tmp_path, ppg))
    tr2.load_model()
    assert torch.equal(tr2.flat_params, tr.flat_params) and tr2.optimizer.steps == tr.optimizer.steps
    assert torch.equal(tr2.state_norm.running_ms.stats, tr.state_norm.running_ms.stats)
    tr.collect_round()
    tr2._batch = [dict(c) for c in tr._batch]
    tr._parity_perms, tr2._parity_perms = iter(perms[2:]), iter(perms[2:])
    tr.update()
    tr2.update()
    assert torch.equal(tr2.flat_params, tr.flat_params)
    assert torch.equal(tr2.optimizer.m, tr.optimizer.m) and torch.equal(tr2.optimizer.v, tr.optimizer.v)
    assert tr.eval(3) and len(tr2.eval(3)) == 3


def test_ppo_rnn_lunarlander_trains(tmp_path):
    from gymrl_amd import ppo_rnn_lunarlander as ppo
    cfg = _cfg(tmp_path, ppo, num_envs=4, batch_size=4, episodes_per_minibatch=1, max_episodes=8)
    assert cfg.env_name == "LunarLander-v2"
    tr = ppo.PPORNNTrainer(cfg)
    tr.train()
    assert tr.learn_step == 2 and len(tr.episode_rewards) == 8
    assert tr.optimizer.steps == {"critic": 8, "trunk": 8}
    assert not hasattr(tr.net, "aux_critic_fc")
    assert len(tr.test()) == 5
