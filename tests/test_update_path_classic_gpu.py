"""The fused PPO update (gymrl_amd/ppo_net.FusedActorCriticUpdate.step) on the three-action classic envs — MountainCar-v0
(obs 2) and Acrobot-v1 (obs 6): step() against torch autograd in f32 and f64 with tests/test_update_path_gpu.py's own
bounds, the one finalize launch against the five, the first layer at obs 6, and PPOTrainer.update() on both envs (fused
against autograd on one replayed minibatch, two trainers alike, the hipGraph replay against the eager loop)."""
import copy

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOSS_CFG = (0.2, 3.0, 0.5, 0.01)       # clip_eps, dual_clip, value_coef, entropy_coef (ppo_lunarlander.py:36-42)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from gymrl_amd import ops
    assert ops.device_ok()
    return torch.device("cuda:0")


def ppo_loss_torch(logits, values, act, lpo, adv, ret, cfg):
    """ppo_lunarlander.py:110-117, :278-300 restated with torch ops (any dtype): tests/test_update_path_gpu.py's."""
    clip_eps, dual_clip, value_coef, entropy_coef = cfg
    logp_all = torch.log_softmax(logits, dim=-1)
    lp = logp_all.gather(1, act.long().unsqueeze(1)).squeeze(1)
    ent = -(logp_all.exp() * logp_all).sum(-1)
    ratio = torch.exp(lp - lpo)
    s1, s2 = ratio * adv, torch.clamp(ratio, 1 - clip_eps, 1 + clip_eps) * adv
    ms = torch.min(s1, s2)
    pol = -torch.mean(torch.where(adv < 0, torch.max(ms, dual_clip * adv), ms))
    return pol + value_coef * torch.mean((values - ret).pow(2)) - entropy_coef * ent.mean()


def _minibatch(B, dev, seed, D, A):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(B, D, device=dev, generator=g)
    act = torch.randint(0, A, (B,), device=dev, generator=g, dtype=torch.int32)
    lpo = -1.099 + 0.2 * torch.randn(B, device=dev, generator=g)
    adv, ret = torch.randn(B, device=dev, generator=g), torch.randn(B, device=dev, generator=g)
    return x, act, lpo, adv, ret


def _net(dev, seed, hidden, D, A):
    from gymrl_amd import ppo_net
    from gymrl_amd.flat import flatten_module
    from gymrl_amd.ppo_lunarlander import ActorCritic
    torch.manual_seed(seed)
    net = ActorCritic(D, A, hidden)
    with torch.no_grad():
        for p in net.parameters():           # non-zero biases, a policy with opinions: every term is exercised
            if p.dim() == 1:
                p.normal_(0, 0.1)
        net.actor[2].weight.mul_(30.0)
    flatten_module(net, dev, order=ppo_net.LAYOUT)
    return net


def _check_against_f64(named_hip, g32, g64):
    """test_step_matches_autograd_f32_and_f64's bounds: within f32 round-off of the f64 gradient, and in the same class as
    torch's own f32 backward."""
    worst = 0.0
    for k, g in named_hip.items():
        scale = float(g64[k].abs().max()) + 1e-30
        e_hip = float((g.double() - g64[k]).abs().max()) / scale
        e_t32 = float((g32[k].double() - g64[k]).abs().max()) / scale
        assert e_hip <= 2e-6 and e_hip <= 4 * e_t32 + 1e-6, (k, e_hip, e_t32)
        worst = max(worst, e_hip)
    return worst


@pytest.mark.parametrize("B,hidden,D,A", [(40, 64, 2, 3), (33, 64, 6, 3), (1000, 64, 6, 3), (4097, 128, 6, 3),
                                          (300, 256, 6, 3), (16385, 256, 2, 3)])
def test_step_matches_autograd_f32_and_f64(dev, B, hidden, D, A):
    from gymrl_amd import ppo_net
    net = _net(dev, B, hidden, D, A)
    x, act, lpo, adv, ret = _minibatch(B, dev, B + 1, D, A)
    net._flat_grads.zero_()
    lg, vl = net(x)
    ppo_loss_torch(lg, vl.view(-1), act, lpo, adv, ret, LOSS_CFG).backward()
    g32 = {k: p.grad.clone() for k, p in net.named_parameters()}
    net64 = copy.deepcopy(net).double()
    for p in net64.parameters():
        p.grad = None
    lg, vl = net64(x.double())
    loss64 = ppo_loss_torch(lg, vl.view(-1), act, lpo.double(), adv.double(), ret.double(), LOSS_CFG)
    loss64.backward()
    g64 = {k: p.grad.clone() for k, p in net64.named_parameters()}
    del net64, lg, vl
    net._flat_grads.fill_(float("nan"))           # every element is written
    fu = ppo_net.FusedActorCriticUpdate(net, B)
    assert fu.one_pass_heads and fu.defer_finalize == (hidden == 256)
    assert (hidden == 256) or (not hasattr(fu, "logits") and not hasattr(fu, "dlogits"))     # no logits round trip
    parts = torch.zeros(fu.metric_blocks(B), 5, dtype=torch.float64, device=dev)
    fu.step(x, act, lpo, adv, ret, LOSS_CFG, None, parts)
    worst = _check_against_f64({k: p.grad for k, p in net.named_parameters()}, g32, g64)
    m = parts.sum(0).cpu().numpy() / B
    assert abs((m[0] + m[1] - LOSS_CFG[3] * m[2]) - float(loss64.detach())) <= 1e-5 * max(1.0, abs(float(loss64.detach())))
    print(f"B={B} hidden={hidden} D={D} A={A}: worst relative gradient error vs f64 = {worst:.2e}")


@pytest.mark.parametrize("B,D,A", [(1, 6, 3), (300, 2, 3), (16385, 6, 3)])
def test_one_finalize_launch_equals_five(dev, B, D, A):
    """step() with the five batch reductions' second halves as ONE launch (gymrl_update_finalize) against the five launches
    behind their producers — every gradient of the flat buffer and the metric partials bit for bit."""
    from gymrl_amd import ppo_net
    outs = []
    for defer in (False, True):
        net = _net(dev, 3, 256, D, A)
        x, act, lpo, adv, ret = _minibatch(B, dev, B + 5, D, A)
        fu = ppo_net.FusedActorCriticUpdate(net, B)
        assert fu.defer_finalize
        fu.defer_finalize = defer
        net._flat_grads.fill_(float("nan"))           # every element is written
        parts = torch.zeros(fu.metric_blocks(B), 5, dtype=torch.float64, device=dev)
        for _ in range(2):                            # the second pass finds the workspaces dirty
            fu.step(x, act, lpo, adv, ret, LOSS_CFG, None, parts)
        assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
        outs.append((torch.cat([p.grad.reshape(-1) for p in net.parameters()]), parts.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("B", [1, 17, 1025])
def test_first_layer_at_six_inputs(dev, B, C):
    from gymrl_amd import ops
    g = torch.Generator(device=dev).manual_seed(100 * B + C)
    x = torch.randn(B, 6, device=dev, generator=g)
    W, b = torch.randn(C, 6, device=dev, generator=g) / 6 ** 0.5, 0.1 * torch.randn(C, device=dev, generator=g)
    out = torch.full((B, C), float("nan"), device=dev)
    ops.linear_tanh_smallk(x, W, b, out)
    want = torch.tanh(x.double() @ W.double().T + b.double())
    err = float((out.double() - want).abs().max())
    print(f"B={B} C={C}: |tanh(x W^T + b) - f64| = {err:.2e}")
    assert err <= 2e-6
    lin = torch.full((B, C), float("nan"), device=dev)
    ops.linear_smallk(x, W, b, lin)                   # the same launch without the tanh
    assert float((lin.double() - (x.double() @ W.double().T + b.double())).abs().max()) <= 2e-6


# ---------------------------------------------------------------------------------------------- trainer level ---
ENVS = [("Acrobot-v1", 6), ("MountainCar-v0", 2)]


def _trainer(env_name, fused=True, graphs=False, epochs=1, minibatches=1):
    from gymrl_amd.ppo_lunarlander import Config, PPOTrainer
    cfg = Config()
    cfg.env_name, cfg.hidden_dim, cfg.num_envs, cfg.update_freq, cfg.seed = env_name, 64, 16, 64, 11
    cfg.num_epochs, cfg.num_minibatches, cfg.fused_update, cfg.use_graphs = epochs, minibatches, fused, graphs
    return PPOTrainer(cfg)


def _first_minibatch_gradient(tr, indices):
    """update() on one explicit shuffle order; the flat gradient as the first minibatch left it (Adam zeroes it as it
    consumes it, so it is read on the way into the first optimizer step), as name -> tensor."""
    grabbed = []
    step = tr.optimizer.step

    def spy(*a, **k):
        if not grabbed:
            grabbed.append(tr.flat_grads.clone())
        return step(*a, **k)
    tr.optimizer.step = spy
    tr.update(tr.collect_rollout(), indices=indices)
    flat = grabbed[0]
    out = {}
    for k, p in tr.model.named_parameters():
        off = (p.data_ptr() - tr.flat_params.data_ptr()) // 4
        out[k] = flat[off:off + p.numel()].view(p.shape)
    return out


@pytest.mark.parametrize("env_name,D", ENVS)
def test_trainer_takes_the_fused_update(dev, env_name, D):
    from gymrl_amd import ppo_net
    total = 16 * 64
    idx = torch.randperm(total, generator=torch.Generator().manual_seed(3)).to(torch.int32).view(1, total)
    fused, plain = _trainer(env_name, True), _trainer(env_name, False)
    assert ppo_net.supported(fused.model) and fused.model.shared[0].in_features == D and fused.action_dim == 3
    assert torch.equal(fused.flat_params, plain.flat_params)
    from gymrl_amd.ppo_lunarlander import ActorCritic
    net64 = ActorCritic(D, 3, 64)                     # parameters of its own, off the flat buffer, as they are before the update
    net64.load_state_dict(fused.model.state_dict())
    net64 = net64.to(dev).double()
    g_hip = _first_minibatch_gradient(fused, idx)
    g_t32 = _first_minibatch_gradient(plain, idx)
    assert fused._fused_update is not None and fused._fused_update.one_pass_heads and not fused._fused_update.defer_finalize
    assert plain._fused_update is None
    for tr in (fused, plain):
        assert bool(torch.isfinite(tr.flat_params).all())
    # the same rows in float64: both trainers collected the same rollout (same seed, same parameters)
    b = fused.buffer
    assert torch.equal(b.states, plain.buffer.states) and torch.equal(b.advantages, plain.buffer.advantages)
    rows = idx[0].long().to(dev)
    x = b.states[:b.T].reshape(total, D)[rows].double()
    act, lpo = b.actions.view(-1)[rows], b.log_probs.view(-1)[rows].double()
    adv, ret = b.advantages.view(-1)[rows].double(), b.returns.view(-1)[rows].double()
    cnt, s1, s2 = (float(v) for v in fused._moments.cpu())
    mean = s1 / cnt
    adv = (adv - mean) / (max(s2 / cnt - mean * mean, 0.0) ** 0.5 + 1e-8)
    for p in net64.parameters():
        p.grad = None
    lg, vl = net64(x)
    ppo_loss_torch(lg, vl.view(-1), act, lpo, adv, ret, fused._loss_cfg).backward()
    g64 = {k: p.grad for k, p in net64.named_parameters()}
    worst = _check_against_f64(g_hip, g_t32, g64)
    print(f"{env_name}: fused first-minibatch gradient vs f64, worst relative error = {worst:.2e}")


@pytest.mark.parametrize("env_name,D", ENVS)
def test_trainer_update_is_reproducible_and_graphable(dev, env_name, D):
    """Two fused trainers built alike end an update() on the same bits; so does the one whose minibatch body is replayed as
    a hipGraph (8 minibatches: two eager warm-ups, the capture, five replays)."""
    outs = []
    for graphs in (False, False, True):
        tr = _trainer(env_name, True, graphs, epochs=2, minibatches=4)
        m = tr.update(tr.collect_rollout())
        assert tr._fused_update is not None and tr.optimizer.step_count == 8
        assert (tr._graph is not None and tr._graph["step"].graph is not None) if graphs else tr._graph is None
        outs.append((tr.flat_params.clone(), tr.optimizer.m.clone(), tr.optimizer.v.clone(), m))
    a, b, g = outs
    assert bool(torch.isfinite(a[0]).all())
    assert torch.equal(a[0], b[0]) and a[3] == b[3]
    assert torch.equal(a[0], g[0]) and torch.equal(a[1], g[1]) and torch.equal(a[2], g[2]) and a[3] == g[3]
