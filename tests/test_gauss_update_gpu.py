"""The Gaussian head's fused PPO update on an MI355X (gymrl_amd/ppo_net.FusedGaussianUpdate, gymrl_gauss_heads_loss_fwd_bwd):
step() against torch autograd in float32 and float64 with tests/test_update_path_classic_gpu.py's bounds, the kernel's outputs
under three grids bit for bit, dZac per row against gymrl_ppo_gauss_loss_fwd_bwd on known means and values, and
ppo_pendulum.PPOTrainer.update() through it (counted, reproducible, against autograd, replayed as a hipGraph).

Every buffer a kernel reads or writes here ends in a NaN guard row behind its last row, and the guard is checked afterwards."""
import copy
import math

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOSS_CFG = (0.2, 3.0, 0.5, 0.01)       # clip_eps, dual_clip, value_coef, entropy_coef
# (ratio, advantage) pairs written over the first rows: below / inside / above the clip band under both signs, both sides of the
# dual clip under a negative advantage, and a zero advantage (tests/gauss_policy_ref.PLANTED)
PLANTED = ((0.75, 1.0), (0.85, 1.0), (1.15, 1.0), (1.25, 1.0), (0.75, -1.0), (0.85, -1.0), (1.15, -1.0), (1.25, -1.0),
           (2.85, -1.0), (3.15, -1.0), (5.0, -2.0), (3.15, 1.0), (1.0, 0.0))
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from gymrl_amd import ops
    assert ops.device_ok()
    return torch.device("cuda:0")


def guarded(t):
    """t [n, ...] -> (the same values as the first n rows of a buffer of n + 1, the guard row filled with NaN / a sentinel)."""
    buf = torch.empty((t.shape[0] + 1,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    buf[:-1].copy_(t)
    buf[-1] = NAN if t.dtype.is_floating_point else -0x5A5A5A5A
    return buf[:-1], buf


def guard_intact(buf):
    g = buf[-1]
    return bool(torch.isnan(g).all()) if buf.dtype.is_floating_point else bool((g == -0x5A5A5A5A).all())


def ppo_gauss_loss_torch(mu, log_std, values, act, lpo, adv, ret, cfg):
    """tests/test_update_path_classic_gpu.ppo_loss_torch's surrogate with the Gaussian head's log-probability and entropy."""
    clip_eps, dual_clip, value_coef, entropy_coef = cfg
    dist = torch.distributions.Normal(mu, log_std.exp().expand_as(mu))
    lp = dist.log_prob(act).sum(-1)
    ent = dist.entropy().sum(-1)
    ratio = torch.exp(lp - lpo)
    s1, s2 = ratio * adv, torch.clamp(ratio, 1 - clip_eps, 1 + clip_eps) * adv
    ms = torch.min(s1, s2)
    pol = -torch.mean(torch.where(adv < 0, torch.max(ms, dual_clip * adv), ms))
    return pol + value_coef * torch.mean((values - ret).pow(2)) - entropy_coef * ent.mean()


def _net(dev, seed, hidden, D, log_std):
    from gymrl_amd import ppo_net
    from gymrl_amd.flat import flatten_module
    from gymrl_amd.ppo_pendulum import GaussianActorCritic
    torch.manual_seed(seed)
    net = GaussianActorCritic(D, 1, hidden, log_std_init=log_std)
    with torch.no_grad():
        for p in net.parameters():           # non-zero biases, a mean that moves with the observation: every term is exercised
            if p.dim() == 1 and p is not net.log_std:
                p.normal_(0, 0.1)
        net.actor[2].weight.mul_(3.0)
    flatten_module(net, dev, order=ppo_net.LAYOUT)
    return net


def _minibatch(net, B, dev, seed, D):
    """x, the action as the packed int32 column, logp_old, adv, ret: the action is a draw around the float64 mean, logp_old the
    float64 log-probability moved by N(0, 0.05), and the first rows carry PLANTED's (ratio, advantage) pairs.
    The bounds are relative to max |g64| of a parameter, and for the one-element parameters (actor.2.bias, critic.2.bias, log_std)
    that is a sum over the rows: rows whose terms cancel would measure that sum's condition number, not the kernel (random signs
    at B = 17, log_std = -1 left torch's own float32 backward 1.6e-6 from float64 on log_std, and step() 2.0e-6).  So the draw lies
    on the side of the mean its advantage has the sign of (every d(loss) / d(mean) has one sign), further than one standard
    deviation out under a positive advantage and nearer under a negative one (so has every row's -adv * (z^2 - 1), the term of
    d(loss) / d(log_std)), and the returns lie around 2 (so has every d(loss) / d(value)): the sums are conditioned like their
    terms."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(B, D, device=dev, generator=g)
    net64 = copy.deepcopy(net).double()
    with torch.no_grad():
        mu, _ = net64(x.double())
        std = net64.log_std.exp()
        adv, ret = torch.randn(B, device=dev, generator=g), 2.0 + torch.randn(B, device=dev, generator=g)
        n = min(B, len(PLANTED))
        adv[:n] = torch.tensor([a for _, a in PLANTED[:n]], device=dev)
        u = torch.rand(B, device=dev, generator=g)
        eps = torch.where(adv < 0, -0.9 * u, 1.0 + u).view(-1, 1)
        act = (mu + std * eps.double()).float()
        lp = torch.distributions.Normal(mu, std.expand_as(mu)).log_prob(act.double()).sum(-1)
        lpo = lp + 0.05 * torch.randn(B, device=dev, generator=g).double()
        lpo[:n] = lp[:n] - torch.log(torch.tensor([r for r, _ in PLANTED[:n]], dtype=torch.float64, device=dev))
    return x, act.view(torch.int32).view(-1), lpo.float(), adv, ret


def _check_against_f64(named_hip, g32, g64):
    """tests/test_update_path_classic_gpu._check_against_f64, restated: relative to max |g64|, e_hip <= 2e-6 and
    e_hip <= 4 * e_t32 + 1e-6 — within f32 round-off of the f64 gradient, and in the same class as torch's own f32 backward."""
    worst = 0.0
    for k, g in named_hip.items():
        scale = float(g64[k].abs().max()) + 1e-30
        e_hip = float((g.double() - g64[k]).abs().max()) / scale
        e_t32 = float((g32[k].double() - g64[k]).abs().max()) / scale
        print(f"  {k}: e_hip = {e_hip:.3e}  e_t32 = {e_t32:.3e}")
        assert e_hip <= 2e-6 and e_hip <= 4 * e_t32 + 1e-6, (k, e_hip, e_t32)
        worst = max(worst, e_hip)
    return worst


def _padding_mask(net):
    """True at the elements of the flat gradient that belong to no parameter (flatten_module's 64-float alignment)."""
    mask = torch.ones_like(net._flat_grads, dtype=torch.bool)
    for p in net.parameters():
        off = (p.data_ptr() - net._flat_params.data_ptr()) // 4
        mask[off:off + p.numel()] = False
    return mask


SHAPES = [(1, 64, 3), (31, 64, 3), (32, 64, 3), (33, 64, 3), (129, 64, 3), (17, 128, 3), (9, 256, 3), (33, 256, 3), (1000, 64, 3),
          (300, 256, 4)]


@pytest.mark.parametrize("log_std", [-1.0, 0.0, 0.5])
@pytest.mark.parametrize("B,hidden,D", SHAPES)
def test_step_matches_autograd_f32_and_f64(dev, B, hidden, D, log_std):
    from gymrl_amd import ops, ppo_net
    net = _net(dev, B + hidden, hidden, D, log_std)
    x, act, lpo, adv, ret = _minibatch(net, B, dev, B + 1, D)
    actf = act.view(torch.float32).view(-1, 1)
    if B >= len(PLANTED):                               # the planted rows sit where they were meant to, in float64
        with torch.no_grad():
            n64 = copy.deepcopy(net).double()
            mu = n64(x.double())[0]
            lp = torch.distributions.Normal(mu, n64.log_std.exp().expand_as(mu)).log_prob(actf.double()).sum(-1)
            ratio = torch.exp(lp - lpo.double())[:len(PLANTED)].cpu()
        assert torch.allclose(ratio, torch.tensor([r for r, _ in PLANTED], dtype=torch.float64), rtol=1e-4)
    net._flat_grads.zero_()
    mu, vl = net(x)
    ppo_gauss_loss_torch(mu, net.log_std, vl.view(-1), actf, lpo, adv, ret, LOSS_CFG).backward()
    g32 = {k: p.grad.clone() for k, p in net.named_parameters()}
    net64 = copy.deepcopy(net).double()
    for p in net64.parameters():
        p.grad = None
    mu, vl = net64(x.double())
    loss64 = ppo_gauss_loss_torch(mu, net64.log_std, vl.view(-1), actf.double(), lpo.double(), adv.double(), ret.double(), LOSS_CFG)
    loss64.backward()
    g64 = {k: p.grad.clone() for k, p in net64.named_parameters()}
    assert set(g64) == set(g32) and "log_std" in g64
    del net64, mu, vl
    net._flat_grads.fill_(NAN)                          # every element of every parameter's gradient is written
    pad = _padding_mask(net)
    fu = ppo_net.FusedGaussianUpdate(net, B + 1)        # one row more than the minibatch: the guard row of every activation
    assert fu.one_pass_heads and not fu.defer_finalize and fu.ws2 is None and not hasattr(fu, "logits")
    acts = [fu.H1, fu.H2, fu.Hac, fu.dH2, fu.dH1]
    for t in acts:
        t.fill_(NAN)
    nbatch = ops.lib().gymrl_gauss_heads_loss_workspace_bytes(B, hidden, 1) // 8
    fu.dls_ws = torch.full((nbatch + 1,), NAN, dtype=torch.float64, device=dev)
    parts = torch.full((fu.metric_blocks(B) + 1, 5), NAN, dtype=torch.float64, device=dev)
    ins = [guarded(t) for t in (x, act, lpo, adv, ret)]
    fu.step(*[v for v, _ in ins], LOSS_CFG, None, parts[:-1])
    torch.cuda.synchronize()
    assert all(guard_intact(buf) for _, buf in ins) and all(guard_intact(t[:B + 1]) for t in acts)
    assert guard_intact(parts) and guard_intact(fu.dls_ws) and bool(torch.isfinite(fu.dls_ws[:-1]).all())
    assert bool(torch.isnan(net._flat_grads[pad]).all())                      # nothing written between the parameters
    assert net.log_std.grad.data_ptr() == fu.dlog_std.data_ptr()
    print(f"B={B} hidden={hidden} D={D} log_std={log_std}:")
    worst = _check_against_f64({k: p.grad for k, p in net.named_parameters()}, g32, g64)
    m = parts[:-1].sum(0).cpu().numpy() / B
    total, want = m[0] + m[1] - LOSS_CFG[3] * m[2], float(loss64.detach())
    print(f"  loss {total:.9f} vs f64 {want:.9f}; worst relative gradient error vs f64 = {worst:.2e}")
    assert abs(total - want) <= 1e-5 * max(1.0, abs(want))


def _kernel_case(dev, B, C, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    Zac = r(B, 2 * C)
    heads = dict(bac=0.1 * r(2 * C), Wa2=r(1, C) / C ** 0.5, ba2=0.1 * r(1), Wc2=r(1, C) / C ** 0.5, bc2=0.1 * r(1))
    log_std = torch.tensor([-0.3], device=dev)
    act, lpo = r(B, 1), -1.2 + 0.3 * r(B)
    adv, ret = r(B), r(B)
    mom = torch.tensor([float(B), float(adv.double().sum()), float((adv.double() ** 2).sum())], dtype=torch.float64, device=dev)
    return Zac, heads, log_std, act, lpo, adv, ret, mom


def _run_kernel(dev, case, grid):
    from gymrl_amd import ops
    Zac, heads, log_std, act, lpo, adv, ret, mom = case
    B, C = Zac.shape[0], Zac.shape[1] // 2
    z, zbuf = guarded(Zac)
    ins = [guarded(t) for t in (act, lpo, adv, ret)]
    outs = {k: torch.full((n + 1,), NAN, device=dev) for k, n in (("dbac", 2 * C), ("dWa2", C), ("dba2", 1), ("dWc2", C), ("dbc2", 1),
                                                                  ("dls", 1))}
    nblk = ops.heads_loss_blocks(B, C)
    parts = torch.full((nblk + 1, 5), NAN, dtype=torch.float64, device=dev)
    dws = torch.full((ops.lib().gymrl_gauss_heads_loss_workspace_bytes(B, C, 1) // 8 + 1,), NAN, dtype=torch.float64, device=dev)
    ws = ops.mlp_train_workspace(C, 3, 1, dev)
    ops.gauss_heads_loss_fwd_bwd(z, heads["bac"], heads["Wa2"], heads["ba2"], heads["Wc2"], heads["bc2"], log_std, ins[0][0], ins[1][0],
                                 ins[2][0], ins[3][0], LOSS_CFG, mom, outs["dbac"][:-1], outs["dWa2"][:-1].view(1, C), outs["dba2"][:-1],
                                 outs["dWc2"][:-1].view(1, C), outs["dbc2"][:-1], outs["dls"][:-1], parts[:-1], ws, dws, grid_blocks=grid)
    torch.cuda.synchronize()
    assert guard_intact(zbuf) and all(guard_intact(b) for _, b in ins) and all(guard_intact(t) for t in outs.values())
    assert guard_intact(parts) and guard_intact(dws)
    assert all(bool(torch.isfinite(t[:-1]).all()) for t in outs.values()) and bool(torch.isfinite(z).all())
    assert bool(torch.isfinite(parts[:-1]).all()) and bool(torch.isfinite(dws[:-1]).all())
    met = ops.reduce_rows(parts[:-1].contiguous().view(1, nblk, 5), 1, nblk, 5)
    return dict(dZac=z.clone(), met=met.clone().view(-1), parts=parts[:-1].clone(), **{k: v[:-1].clone() for k, v in outs.items()})


@pytest.mark.parametrize("C", [64, 256])
def test_outputs_do_not_depend_on_the_grid(dev, C):
    """B = 9 batches + 3 rows is ten batches on three workgroups by default; one workgroup walks all ten (its waves take 3, 3, 2
    and 2 of them), and every output keeps its bits: dlog_std, dZac, the five head gradients — and the metric rows, so that their
    reduction agrees far inside float64 reassociation."""
    from gymrl_amd import ops
    kBatch = 8 * (256 // C)
    B = 9 * kBatch + 3
    assert ops.heads_loss_blocks(B, C) == 3
    case = _kernel_case(dev, B, C, 7 + C)
    runs = [_run_kernel(dev, case, grid) for grid in (1, 3, 0, 0, 1)]
    for r in runs[1:]:
        for k in ("dls", "dZac", "dbac", "dWa2", "dba2", "dWc2", "dbc2"):
            assert torch.equal(r[k], runs[0][k]), k
        assert torch.allclose(r["met"], runs[0]["met"], rtol=1e-12, atol=0.0)
    assert float(runs[0]["dls"].abs()) > 0.0 and float(runs[0]["dZac"].abs().max()) > 0.0
    assert bool((runs[0]["dZac"][B - 1, C:] != 0).all())                      # the last batch's three rows were written


@pytest.mark.parametrize("B,C", [(37, 64), (19, 128), (11, 256)])
def test_dzac_per_row_is_the_loss_kernels_gradient_times_tanh_prime(dev, B, C):
    """Head weights that are zero except one column each (a one there), no head bias: mu = tanh(Zac + bac)[c0] and v = the same
    at critic column c1 are known float32 values (gymrl_tanh_inplace runs the same train_tanhf), and dZac's only non-zero columns
    are gymrl_ppo_gauss_loss_fwd_bwd's dmu / dvalue on those, times 1 - h * h."""
    from gymrl_amd import ops
    Zac, heads, log_std, act, lpo, adv, ret, mom = _kernel_case(dev, B, C, 100 + C)
    c0, c1 = 5, C - 3
    heads["Wa2"] = torch.zeros(1, C, device=dev)
    heads["Wc2"] = torch.zeros(1, C, device=dev)
    heads["Wa2"][0, c0] = 1.0
    heads["Wc2"][0, c1] = 1.0
    heads["ba2"], heads["bc2"] = None, None
    H = ops.tanh_inplace(Zac.clone(), heads["bac"])
    mu, v = H[:, c0:c0 + 1].contiguous(), H[:, C + c1].contiguous()
    dmu, dv, dls = ops.ppo_gauss_loss_fwd_bwd(mu, log_std, v, act, lpo, adv, ret, LOSS_CFG, adv_moments=mom)
    got = _run_kernel(dev, (Zac, heads, log_std, act, lpo, adv, ret, mom), 0)
    want = torch.zeros(B, 2 * C, device=dev)
    want[:, c0] = dmu.view(-1) * (1.0 - mu.view(-1) * mu.view(-1))
    want[:, C + c1] = dv * (1.0 - v * v)
    assert bool((want[:, c0] != 0).any()) and bool((want[:, C + c1] != 0).all())
    assert torch.equal(got["dZac"], want)               # (-0.0 == 0.0: the other columns are a product with a zero weight)
    # the head's own bias gradients are the column sums of dmu / dvalue, and dlog_std the loss kernel's up to the order of the sum
    assert abs(float(got["dba2"]) - float(dmu.double().sum())) <= 1e-6 * float(dmu.double().abs().sum())
    assert abs(float(got["dbc2"]) - float(dv.double().sum())) <= 1e-6 * float(dv.double().abs().sum())
    assert abs(float(got["dls"]) - float(dls)) <= 1e-6 * max(abs(float(dls)), 1e-3)


# ---------------------------------------------------------------------------------------------- trainer level ---
def _trainer(fused=True, graphs=False, hidden=64):
    from gymrl_amd.ppo_pendulum import Config, PPOTrainer
    cfg = Config()
    cfg.num_envs, cfg.update_freq, cfg.num_epochs, cfg.num_minibatches, cfg.hidden_dim, cfg.seed = 8, 16, 2, 2, hidden, 5
    cfg.fused_update, cfg.use_graphs, cfg.entropy_coef = fused, graphs, 0.01
    return PPOTrainer(cfg)


def test_trainer_update_goes_through_the_fused_step(dev, monkeypatch):
    from gymrl_amd import ppo_net
    steps = []
    orig = ppo_net.FusedGaussianUpdate.step

    def counting_step(self, x, *a, **k):
        steps.append((type(self).__name__, int(x.shape[0])))
        return orig(self, x, *a, **k)
    monkeypatch.setattr(ppo_net.FusedGaussianUpdate, "step", counting_step)
    outs = []
    for _ in range(2):                                  # two trainers from one seed
        tr = _trainer()
        assert ppo_net.gauss_supported(tr.model) and not ppo_net.supported(tr.model)
        for _ in range(2):
            m = tr.update(tr.collect_rollout())
        assert isinstance(tr._fused_update, ppo_net.FusedGaussianUpdate) and tr.optimizer.step_count == 8
        assert all(math.isfinite(float(v)) for v in m.values()) and bool(torch.isfinite(tr.flat_params).all())
        outs.append(tr.flat_params.clone())
    assert steps == [("FusedGaussianUpdate", 64)] * 16                        # every optimiser step of all four updates
    assert torch.equal(outs[0], outs[1])
    plain = _trainer(fused=False)
    plain.update(plain.collect_rollout())
    assert plain._fused_update is None and len(steps) == 16                   # fused_update = False stays on autograd


def _first_minibatch_gradient(tr, indices):
    """update() on one explicit shuffle order; the flat gradient as the first minibatch left it (read on the way into the first
    optimizer step: Adam zeroes it as it consumes it), as name -> tensor."""
    grabbed = []
    step = tr.optimizer.step

    def spy(*a, **k):
        if not grabbed:
            grabbed.append(tr.flat_grads.clone())
        return step(*a, **k)
    tr.optimizer.step = spy
    tr.update(tr.collect_rollout(), indices=indices)
    out = {}
    for k, p in tr.model.named_parameters():
        off = (p.data_ptr() - tr.flat_params.data_ptr()) // 4
        out[k] = grabbed[0][off:off + p.numel()].view(p.shape)
    return out


def test_trainer_fused_and_autograd_agree_on_one_minibatch(dev):
    from gymrl_amd.ppo_pendulum import GaussianActorCritic
    total = 8 * 16
    idx = torch.stack([torch.randperm(total, generator=torch.Generator().manual_seed(3 + e)) for e in range(2)]).to(torch.int32)
    fused, plain = _trainer(True), _trainer(False)
    assert torch.equal(fused.flat_params, plain.flat_params)
    net64 = GaussianActorCritic(3, 1, 64)               # parameters of its own, as they are before the update
    net64.load_state_dict(fused.model.state_dict())
    net64 = net64.to(dev).double()
    g_hip, g_t32 = _first_minibatch_gradient(fused, idx), _first_minibatch_gradient(plain, idx)
    assert fused._fused_update is not None and plain._fused_update is None
    b = fused.buffer
    assert torch.equal(b.states, plain.buffer.states) and torch.equal(b.actions, plain.buffer.actions)
    assert torch.equal(b.advantages, plain.buffer.advantages)
    rows = idx[0, :64].long().to(dev)                   # the first minibatch
    x = b.states[:b.T].reshape(total, 3)[rows].double()
    act, lpo = b.actions.view(-1, 1)[rows].double(), b.log_probs.view(-1)[rows].double()
    adv, ret = b.advantages.view(-1)[rows].double(), b.returns.view(-1)[rows].double()
    cnt, s1, s2 = (float(v) for v in fused._moments.cpu())
    mean = s1 / cnt
    adv = (adv - mean) / (max(s2 / cnt - mean * mean, 0.0) ** 0.5 + 1e-8)
    for p in net64.parameters():
        p.grad = None
    mu, vl = net64(x)
    ppo_gauss_loss_torch(mu, net64.log_std, vl.view(-1), act, lpo, adv, ret, fused._loss_cfg).backward()
    worst = _check_against_f64(g_hip, g_t32, {k: p.grad for k, p in net64.named_parameters()})
    print(f"Pendulum-v1: fused first-minibatch gradient vs f64, worst relative error = {worst:.2e}")


def test_trainer_graph_replay_equals_the_eager_loop(dev):
    outs = []
    for graphs in (False, True):
        tr = _trainer(True, graphs)
        m = tr.update(tr.collect_rollout())             # 4 minibatches: two eager warm-ups, the capture, one replay
        assert tr.optimizer.step_count == 4
        assert (tr._graph is not None and tr._graph["step"].graph is not None) if graphs else tr._graph is None
        outs.append((tr.flat_params.clone(), tr.optimizer.m.clone(), tr.optimizer.v.clone(), m))
    e, g = outs
    assert bool(torch.isfinite(e[0]).all())
    assert torch.equal(e[0], g[0]) and torch.equal(e[1], g[1]) and torch.equal(e[2], g[2]) and e[3] == g[3]
