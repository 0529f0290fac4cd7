"""es_lunarlander.ESTrainer on the one packing launch and on the recurrent policy, on the GPU (P = 8, E = 2 throughout): the
feed-forward generations against generations driven by hand with the packing loop the launch replaced, and the recurrent policy's
generation, replay, resume and evaluation."""
import numpy as np
import pytest

from test_pack_stack_gpu import loop_stack_buffer

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

P, E = 8, 2


def trainer(policy, seed=3, method="snes"):
    from gymrl_amd.es_lunarlander import Config, ESTrainer
    cfg = Config()
    cfg.policy, cfg.method, cfg.seed, cfg.population, cfg.episodes_per_policy, cfg.log_freq = policy, method, seed, P, E, 0
    return ESTrainer(cfg)


def test_mlp_generations_are_the_packing_loops_bit_for_bit():
    from gymrl_amd import ops
    from gymrl_amd.es_cartpole import make_learner
    t = trainer("mlp")
    fused, centre = t.model._act_net(), t.flat_params.clone()
    hand = make_learner(t.cfg, centre, t.base_seed)
    stack = None
    for g in range(3):
        # by hand, as the trainer ran before: a fresh stack filled by a launch and a copy per layer and policy
        params = hand.ask()
        by_loop = ops.LunarPolicyStack(fused, t.flat_params, params)
        by_loop.buffer.copy_(loop_stack_buffer(fused, t.flat_params, params))
        returns = ops.lunar_policy_eval(by_loop, E, t.base_seed + 1_000_003, (1 << 41) + g * E, want_terminal_obs=False)[0]
        hand.tell(returns)
        t.step_generation()
        assert torch.equal(t.last_returns, returns) and t.last_returns.dtype == torch.float64
        assert torch.equal(t.es.mu, hand.mu) and torch.equal(t.es.sigma, hand.sigma)
        assert isinstance(t.stack, ops.LunarPolicyStack) and (stack is None or t.stack is stack)      # one stack for the run
        stack = t.stack
    assert t.generation == 3 and len(torch.unique(t.last_returns)) > 1
    assert not torch.equal(hand.sigma, torch.full_like(hand.sigma, t.cfg.sigma))


def test_mlprnn_generation_is_ask_evaluate_tell_by_hand():
    from gymrl_amd import ops
    from gymrl_amd.es_cartpole import make_learner
    from gymrl_amd.ppg_rnn_lunarlander import ActorCriticPPG
    t = trainer("mlprnn")
    assert isinstance(t.model, ActorCriticPPG) and t.stack is None
    centre = t.flat_params.clone()
    hand = make_learner(t.cfg, centre, t.base_seed)
    params = hand.ask()
    n = t.flat_params.numel()
    stack = ops.MlprnnPolicyStack(t.model, t.flat_params, params[:, :n])             # the copying stack, raw observations
    returns = ops.lunar_mlprnn_eval(stack, E, t.base_seed + 1_000_003, 1 << 41, norm_stats=None, want_terminal_obs=False)[0]
    hand.tell(returns)
    t.step_generation()
    assert t.generation == 1 and t.train_stream_id0() == (1 << 41) + E
    assert t.last_returns.dtype == torch.float64 and tuple(t.last_returns.shape) == (P, E)
    assert torch.equal(t.last_returns, returns) and len(torch.unique(returns)) > 1
    assert torch.equal(t.flat_params, centre) and torch.equal(t.es.sigma, hand.sigma) and torch.equal(t.es.weights, hand.weights)
    # no copy between ask() and the launch: the stack IS the learner's buffer, and stays the run's
    assert t.stack.buffer is t.es.stack and t.stack.norm_stats is None
    first = t.stack
    t.step_generation()
    assert t.stack is first


def test_mlprnn_replays_bit_for_bit():
    a, b = trainer("mlprnn"), trainer("mlprnn")
    mu0 = a.es.mu.clone()
    for _ in range(3):
        a.step_generation()
        b.step_generation()
    assert a.generation == b.generation == 3
    assert torch.equal(a.es.mu, b.es.mu) and torch.equal(a.es.sigma, b.es.sigma) and torch.equal(a.last_returns, b.last_returns)
    assert not torch.equal(a.es.mu, mu0)


def test_mlprnn_resumes_bit_for_bit_and_refuses_the_other_policy(tmp_path):
    whole = trainer("mlprnn")
    whole.train(max_generations=4)
    first = trainer("mlprnn")
    first.train(max_generations=2)
    path = str(tmp_path / "es_mlprnn.pt")
    saved = first.save_checkpoint(path)
    assert saved["policy"] == "mlprnn" and "es_net_state_dict" in saved and "model_state_dict" not in saved
    second = trainer("mlprnn")
    second.flat_params.zero_()
    second.es.sigma.zero_()
    second.load_checkpoint(path)
    assert second.generation == 2 and torch.equal(second.es.mu, first.es.mu) and torch.equal(second.es.sigma, first.es.sigma)
    second.train(max_generations=2)
    assert second.generation == whole.generation == 4
    assert torch.equal(second.es.mu, whole.es.mu) and torch.equal(second.es.sigma, whole.es.sigma)
    assert torch.equal(second.last_returns, whole.last_returns)
    with pytest.raises(ValueError, match="mlprnn"):
        trainer("mlp").load_checkpoint(path)
    other = trainer("mlp")
    other.step_generation()
    path = str(tmp_path / "es_mlp.pt")
    assert other.save_checkpoint(path)["policy"] == "mlp"
    with pytest.raises(ValueError, match="'mlp'"):
        trainer("mlprnn").load_checkpoint(path)
    with pytest.raises(ValueError, match="policy"):
        trainer("gru")


def test_mlprnn_evaluate_is_evals_returns():
    t = trainer("mlprnn")
    t.step_generation()
    returns, lengths, terminated = t.evaluate(4)
    assert returns.dtype == np.float64 and returns.shape == (1, 4) and lengths.dtype == np.int32 and terminated.dtype == np.uint8
    assert t.eval(num_episodes=4) == returns[0].astype(np.float32).tolist()
    # a stack of the centre's copies through evaluate(params=...)
    both = t.evaluate(4, params=torch.stack([t.flat_params, t.flat_params]))
    assert np.array_equal(both[0][0], returns[0]) and np.array_equal(both[0][1], returns[0])
