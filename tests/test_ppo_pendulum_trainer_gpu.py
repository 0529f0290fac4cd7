"""ppo_pendulum.PPOTrainer on an MI355X: the one-launch rollout and the step loop train the same parameters, a checkpoint resumes
to the bits of an uninterrupted run, and the one-launch evaluation returns the loop's episodes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from gymrl_amd import ops
    assert ops.device_ok(), "libgymrl_hip.so did not find a gfx950 device"
    return torch.device("cuda:0")


def _trainer(iterations=2, **more):
    from gymrl_amd.ppo_pendulum import Config, PPOTrainer
    cfg = Config()
    cfg.num_envs, cfg.update_freq, cfg.hidden_dim, cfg.seed = 32, 32, 64, 7
    cfg.num_epochs, cfg.num_minibatches, cfg.entropy_coef = 2, 4, 0.01
    cfg.max_train_steps = iterations * 32 * 32
    for k, v in more.items():
        setattr(cfg, k, v)
    return PPOTrainer(cfg)


def test_persistent_rollout_and_step_loop_train_the_same_parameters(dev):
    a, b = _trainer(persistent_rollout=True), _trainer(persistent_rollout=False)
    assert a._persistent_ok() and not b._persistent_ok()
    start = a.flat_params.clone()
    assert torch.equal(start, b.flat_params)
    a.train(), b.train()
    assert a.rollout_count == b.rollout_count == 2
    assert torch.equal(a.flat_params, b.flat_params)
    for name in ("states", "actions", "log_probs", "values", "rewards", "dones", "advantages", "returns"):
        assert torch.equal(getattr(a.buffer, name), getattr(b.buffer, name)), name
    assert a.buffer.actions.dtype == torch.float32
    assert not torch.equal(a.flat_params, start)
    assert float(a.model.log_std.detach()[0]) != 0.0                        # log_std sits in the optimiser's flat buffer and moved
    ls = a.model.log_std
    assert a.flat_params.data_ptr() <= ls.data_ptr() < a.flat_params.data_ptr() + 4 * a.flat_params.numel()
    # the stored reward is the env's times reward_scale; the episode statistics are not scaled
    c = _trainer(reward_scale=1.0)
    c.collect_rollout()
    a2 = _trainer()
    a2.collect_rollout()
    assert torch.equal(a2.buffer.rewards, c.buffer.rewards * torch.tensor(0.1, device=dev))
    assert torch.equal(a2.env.ep_stats, c.env.ep_stats)


def test_checkpoint_resume_is_bit_identical(dev, tmp_path):
    whole = _trainer(iterations=3)
    whole.train()
    first = _trainer(iterations=3)
    first.cfg.max_train_steps = 2 * 32 * 32                                  # stop after two of the three iterations ...
    first.cfg.anneal_lr = True
    first_total = 3 * 32 * 32

    def run(tr, until):
        """train()'s body with the learning-rate schedule of the WHOLE run"""
        while tr.step_count < until:
            lr = tr.cfg.lr * (1.0 - tr.step_count / first_total)
            for g in tr.optimizer.param_groups:
                g["lr"] = lr
            tr.update(tr.collect_rollout())
    run(first, 2 * 32 * 32)
    path = str(tmp_path / "ppo_pendulum.pt")
    first.save_checkpoint(path)
    second = _trainer(iterations=3)
    second.load_checkpoint(path)
    assert torch.equal(second.flat_params, first.flat_params) and second.rollout_count == 2
    assert "log_std" in torch.load(path, map_location="cpu", weights_only=False)["model_state_dict"]
    run(second, first_total)
    assert torch.equal(second.flat_params, whole.flat_params)


def test_fused_eval_returns_equal_the_loop(dev):
    tr = _trainer(fused_eval=True)
    tr.update(tr.collect_rollout())
    fused = tr.eval(10)
    loop = tr._eval_loop(10)
    assert fused == loop and len(fused) == 10 and all(-2000.0 < r < 0.0 for r in fused)
    ret, length, termd = tr.evaluate(10)
    assert ret.shape == (1, 10) and (length == 200).all() and not termd.any()
    assert np.array_equal(ret[0].astype(np.float32), np.asarray(fused, np.float32))
    stack = tr.evaluate(4, params=torch.stack([tr.flat_params, tr.flat_params * 0.5]))
    assert stack[0].shape == (2, 4) and np.array_equal(stack[0][0], ret[0, :4]) and not np.array_equal(stack[0][1], ret[0, :4])
