"""The evolution-strategies trainers under both learners on the GPU: es_cartpole.ESTrainer with method = "snes" (replay, resume,
a seeded learning run) and with the default method (the bits of an OpenAIES driven by hand), and es_lunarlander.ESTrainer (one
generation against the learner and the evaluator driven by hand, and an ES checkpoint played by a PPOTrainer)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LEARN_GENERATIONS = 30       # the generation budget of the learning test (DESIGN §4v has the measured means)


def cartpole(method, seed=0, **kw):
    from gymrl_amd.es_cartpole import Config, ESTrainer
    cfg = Config()
    cfg.method, cfg.seed, cfg.hidden_dim, cfg.population, cfg.episodes_per_policy, cfg.log_freq = method, seed, 64, 64, 4, 0
    for k, v in kw.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    return ESTrainer(cfg)


def lunar(method, seed=3):
    from gymrl_amd.es_lunarlander import Config, ESTrainer
    cfg = Config()
    cfg.method, cfg.seed, cfg.hidden_dim, cfg.population, cfg.episodes_per_policy, cfg.log_freq = method, seed, 64, 8, 2, 0
    return ESTrainer(cfg)


def test_cartpole_snes_replays_bit_for_bit():
    from gymrl_amd.es import SeparableNES
    a, b = cartpole("snes"), cartpole("snes")
    assert isinstance(a.es, SeparableNES) and a.es.mu is a.flat_params
    mu0, sigma0 = a.es.mu.clone(), a.es.sigma.clone()
    assert torch.equal(sigma0, torch.full_like(sigma0, a.cfg.sigma))
    for _ in range(3):
        a.step_generation()
        b.step_generation()
    assert a.generation == b.generation == 3 and a.last_returns.dtype == torch.float32
    assert torch.equal(a.es.mu, b.es.mu) and torch.equal(a.es.sigma, b.es.sigma) and torch.equal(a.last_returns, b.last_returns)
    assert not torch.equal(a.es.mu, mu0) and not torch.equal(a.es.sigma, sigma0)
    assert bool((a.es.sigma >= a.es.sigma_min).all()) and bool((a.es.sigma <= a.es.sigma_max).all())


def test_cartpole_snes_resumes_bit_for_bit(tmp_path):
    whole = cartpole("snes")
    whole.train(max_generations=4)
    first = cartpole("snes")
    first.train(max_generations=2)
    path = str(tmp_path / "snes.pt")
    first.save_checkpoint(path)
    second = cartpole("snes", eta_mu=0.5)                             # the learning rates and bounds come from the file too
    second.flat_params.zero_()
    second.es.sigma.zero_()
    second.load_checkpoint(path)
    assert second.generation == 2 and second.es.seed == 0 and second.es.eta_mu == 1.0
    assert torch.equal(second.es.mu, first.es.mu) and torch.equal(second.es.sigma, first.es.sigma)
    second.train(max_generations=2)
    assert second.generation == whole.generation == 4
    assert torch.equal(second.es.mu, whole.es.mu) and torch.equal(second.es.sigma, whole.es.sigma)
    assert torch.equal(second.last_returns, whole.last_returns)


def test_cartpole_default_method_is_openai_es_driven_by_hand():
    """Config's defaults but for the seed: the trainer's centre after 2 generations is an OpenAIES's on a copy of the initial
    centre, asked, evaluated on the training streams through evaluate() and told by hand — the path the trainer had before there
    was a choice of method."""
    from gymrl_amd.es import OpenAIES
    from gymrl_amd.es_cartpole import Config, ESTrainer
    cfg = Config()
    cfg.seed, cfg.log_freq = 0, 0
    assert cfg.method == "openai"
    t = ESTrainer(cfg)
    assert isinstance(t.es, OpenAIES)
    theta = t.flat_params.clone()
    hand = OpenAIES(theta, t.base_seed, cfg.population, cfg.sigma, cfg.lr)
    E = cfg.episodes_per_policy
    for g in range(2):
        stack = hand.ask()
        returns, _, _ = t.evaluate(E, params=stack, stream_offset=(t.TRAIN_ENV_ID0 - t.EVAL_ENV_ID0) + g * E)
        hand.tell(torch.from_numpy(np.ascontiguousarray(returns, np.float32)).to(t.device))
        t.step_generation()
        assert torch.equal(t.last_returns.cpu(), torch.from_numpy(np.asarray(returns, np.float32)))
    assert t.generation == hand.generation == 2
    assert torch.equal(t.flat_params, theta) and torch.equal(t.es.optimizer.m, hand.optimizer.m)


def test_cartpole_snes_improves():
    """Seeded, hence reproducible: the centre after LEARN_GENERATIONS generations against the initial centre, on the same 64
    held-out episodes (eval()'s streams: no training start is among them).  Measured: DESIGN §4v."""
    t = cartpole("snes")
    before = float(t.evaluate(64)[0].mean())
    t.train(max_generations=LEARN_GENERATIONS)
    after = float(t.evaluate(64)[0].mean())
    print(f"CartPole-v1 SNES centre, 64 held-out episodes: {before:.2f} -> {after:.2f} after {LEARN_GENERATIONS} generations")
    assert after > before


def test_cartpole_checkpoints_carry_the_method(tmp_path):
    a = cartpole("openai", population=8, episodes_per_policy=2)
    a.step_generation()
    path = str(tmp_path / "openai.pt")
    a.save_checkpoint(path)
    with pytest.raises(ValueError, match="openai"):
        cartpole("snes", population=8, episodes_per_policy=2).load_checkpoint(path)
    b = cartpole("snes", population=8, episodes_per_policy=2)
    b.step_generation()
    path = str(tmp_path / "snes.pt")
    b.save_checkpoint(path)
    with pytest.raises(ValueError, match="snes"):
        cartpole("openai", population=8, episodes_per_policy=2).load_checkpoint(path)
    with pytest.raises(ValueError):
        cartpole("cma")


@pytest.mark.parametrize("method", ["snes", "openai"])
def test_lunar_generation_is_ask_evaluate_tell_by_hand(method):
    from gymrl_amd import ops
    from gymrl_amd.es_cartpole import make_learner
    t = lunar(method)
    cfg = t.cfg
    centre = t.flat_params.clone()
    hand = make_learner(cfg, centre, t.base_seed)
    stack = ops.LunarPolicyStack(t.model._act_net(), t.flat_params, hand.ask())
    returns = ops.lunar_policy_eval(stack, 2, t.base_seed + 1_000_003, (1 << 41) + 0 * 2, want_terminal_obs=False)[0]
    hand.tell(returns if method == "snes" else returns.to(torch.float32))
    t.step_generation()
    assert t.generation == 1 and t.train_stream_id0() == (1 << 41) + 2
    assert t.last_returns.dtype == torch.float64 and tuple(t.last_returns.shape) == (8, 2)
    assert torch.equal(t.last_returns, returns) and len(torch.unique(returns)) > 1
    assert torch.equal(t.flat_params, centre) and torch.equal(t.es.weights, hand.weights)
    if method == "snes":
        assert torch.equal(t.es.sigma, hand.sigma) and not torch.equal(hand.sigma, torch.full_like(hand.sigma, cfg.sigma))
    else:
        assert torch.equal(t.es.optimizer.m, hand.optimizer.m) and torch.equal(t.es.optimizer.v, hand.optimizer.v)


@pytest.mark.parametrize("method", ["snes", "openai"])
def test_lunar_checkpoint_is_a_policy_a_ppo_trainer_plays(method, tmp_path):
    from gymrl_amd import ppo_lunarlander
    t = lunar(method)
    t.step_generation()
    path = str(tmp_path / "es_lunar.pt")
    t.save_checkpoint(path)
    mine = t.evaluate(2)
    assert mine[0].dtype == np.float64 and mine[0].shape == (1, 2)
    assert t.eval(num_episodes=2) == mine[0][0].astype(np.float32).tolist()
    cfg = ppo_lunarlander.Config()
    cfg.seed, cfg.hidden_dim, cfg.num_envs, cfg.update_freq = t.base_seed, 64, 16, 8
    ppo = ppo_lunarlander.PPOTrainer(cfg)
    ppo.load_checkpoint(path)
    theirs = ppo.evaluate(2)
    for a, b in zip(mine, theirs):
        assert np.array_equal(a, b)
    # and back into an ES trainer: the learner's state with it
    again = lunar(method)
    again.load_checkpoint(path)
    assert again.generation == 1 and torch.equal(again.flat_params, t.flat_params)
    with pytest.raises(ValueError):
        lunar("openai" if method == "snes" else "snes").load_checkpoint(path)
