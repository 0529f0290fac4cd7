"""The fused discrete-SAC vector step (csrc/dsac_step.hip: acting + env + replay row in one launch, update() in four) against
the layer-by-layer path it replaces (gymrl_lin_* launches, the stand-alone draw / loss / optimiser / replay / env kernels —
which tests/test_trainers_gpu.py pins against the reference's own update() — and the softmax of csrc/softmax_device.hpp,
Config.kernel_softmax): same noise, same index draws -> every parameter, Adam moment, both targets, the temperature, the
loss sums and the replay ring equal BIT FOR BIT."""
import ctypes

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FLATS = ("actor_flat", "c1_flat", "c2_flat", "c1_target_flat", "c2_target_flat")
OPTS = ("actor_optim", "critic1_optim", "critic2_optim")


def _trainer(N, B, hidden, fused, graphs=None, images=True, seed=5, softmax=True):
    from gymrl_amd import sac_cartpole
    cfg = sac_cartpole.Config()
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed = N, B, hidden, seed
    cfg.max_episodes, cfg.memory_capacity = 10 ** 9, (1 << 20 if N >= 4096 else max(4096, 4 * B))
    cfg.fused_step, cfg.fused_images, cfg.kernel_softmax = fused, images, softmax
    if graphs is not None:
        cfg.use_graphs = graphs
    return sac_cartpole.SACTrainer(cfg)


def _exp_draws(N, A, steps, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.empty(N, A, device="cuda").exponential_(generator=g) for _ in range(steps)]


def _run(fused, steps, N, B, hidden, explicit=True, images=True):
    """Trainer A (layer path, kernel softmax, eager update) or B (fused_step alone).  explicit: Exp(1) draws through
    _parity_noise; otherwise the kernels' own Philox.  Each path draws its own indices from the same (seed, counter, size)."""
    tr = _trainer(N, B, hidden, fused, graphs=None if fused else False, images=images)
    assert tr._fused_ok() == fused
    if explicit:
        tr._parity_noise = iter(_exp_draws(N, tr.action_dim, steps))
    tr.train(max_vector_steps=steps)
    torch.cuda.synchronize()
    return tr


def _assert_same(a, b, what=""):
    for opt in OPTS:
        assert getattr(a, opt).step_count == getattr(b, opt).step_count, (what, opt)
    assert (a.memory.cursor, a.memory.size, a.memory.draws) == (b.memory.cursor, b.memory.size, b.memory.draws), what
    assert (a._act_counter, a._alpha_steps) == (b._act_counter, b._alpha_steps), what
    for k, (x, y) in enumerate(zip(a.memory.ring, b.memory.ring)):
        assert torch.equal(x, y), (what, "ring", k)          # acting: same actions, same physics, same rows
    for name in FLATS:
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    for opt in OPTS:
        assert torch.equal(getattr(a, opt).m, getattr(b, opt).m) and torch.equal(getattr(a, opt).v, getattr(b, opt).v), (what, opt)
    for name in ("log_alpha", "_alpha_m", "_alpha_v", "_sums_c", "_sums_a", "_alpha_loss"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name, getattr(a, name), getattr(b, name))
    assert list(a.episode_rewards) == list(b.episode_rewards), what


# (hidden 256: the instances built for that width, weight images; 36: no images, no 16-column alignment; B = 24 / 100 / 250: a
#  partial last slab; N = 1: the scalar surface's; 4096 / 128 / 256: 256 acting workgroups, ring of 2^20 rows)
SHAPES = [(64, 128, 256, 16), (20, 24, 32, 14), (33, 100, 36, 16), (17, 250, 256, 28), (1, 16, 32, 40), (4096, 128, 256, 12)]


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_fused_step_equals_layer_by_layer(case):
    N, B, hidden, steps = SHAPES[case]
    explicit = case % 2 == 0                 # explicit draws in half the cases, the kernels' own Philox in the other half
    a, b = _run(False, steps, N, B, hidden, explicit), _run(True, steps, N, B, hidden, explicit)
    assert a._fused is None and b._fused is not None
    assert b.critic1_optim.step_count >= 10 and b.actor_optim.step_count >= 10
    assert len(b.episode_rewards) >= 1       # auto-reset and the terminal observation took part
    _assert_same(a, b)


def test_images_change_where_a_value_is_read_not_the_value():
    from gymrl_amd import ops
    N, B, hidden, steps = 64, 128, 256, 16
    b, c = _run(True, steps, N, B, hidden), _run(True, steps, N, B, hidden, images=False)
    assert b._fused[4] is not None and c._fused[4] is None
    _assert_same(b, c)
    before = b._fused[4].clone()                       # and they do hold the parameters: rebuilding them changes nothing
    ops.dsac_pack_images(b._fused[1])
    torch.cuda.synchronize()
    assert torch.equal(before, b._fused[4])
    assert before.abs().sum().item() > 0


@pytest.mark.parametrize("N,hidden,steps", [(4096, 256, 24), (50, 64, 60)])
def test_act_launch_equals_the_kernels_composed_by_hand(N, hidden, steps):
    """gymrl_dsac_act_step against actor.logits (gymrl_lin_fwd) -> ops.categorical_sample -> env.step -> memory.push, kernels
    that are pinned to the oracle one by one.  Episodes end under the fresh policy within the 60 steps (auto-reset, TERMINAL
    observation in the ring).  CartPole's 500-step truncation is NOT reached here (an untrained policy falls long before): it is
    cartpole_step_one's own branch, shared with the stand-alone stepper and pinned by the env tests."""
    from gymrl_amd import ops
    a, b = _trainer(N, 128, hidden, False), _trainer(N, 128, hidden, True)
    assert torch.equal(a.actor_flat, b.actor_flat)
    dev, D, A = a.device, a.env.obs_dim, a.action_dim
    draws = _exp_draws(N, A, steps, seed=3)
    obs_a, obs_b = a.env.reset(), torch.empty(N, D, device=dev)
    b.env.reset(obs_b)
    assert torch.equal(obs_a, obs_b)
    nxt_a, tobs, nxt_b = (torch.empty(N, D, device=dev) for _ in range(3))
    rew_a, rew_b = torch.empty(N, device=dev), torch.empty(N, device=dev)
    done_a, done_b = (torch.zeros(N, dtype=torch.uint8, device=dev) for _ in range(2))
    act_b = torch.empty(N, dtype=torch.int32, device=dev)
    args = b._fused_args()[0]
    dones = 0
    for t in range(steps):
        noise = draws[t] if t % 2 == 0 else None          # explicit / Philox
        with torch.no_grad():
            logits = a.actor.logits(obs_a)
        act_a, _, _, _ = ops.categorical_sample(logits, noise_exp=noise, seed=a.base_seed, counter=t + 1, env_id0=a.env.env_id0)
        a.env.step(act_a, nxt_a, rew_a, done_out=done_a, term_obs_out=tobs)
        a.memory.push(obs_a, act_a, rew_a, tobs, done_a)
        ops.dsac_act_step(args, b.env, obs_b, nxt_b, cursor=b.memory.cursor, noise_exp=noise, seed=b.base_seed, counter=t + 1,
                          action_out=act_b, rew_out=rew_b, done_out=done_b)
        b.memory.advance(N)
        assert torch.equal(act_a, act_b) and torch.equal(nxt_a, nxt_b) and torch.equal(rew_a, rew_b) and torch.equal(done_a, done_b), t
        dones += int(done_a.sum().item())
        obs_a, nxt_a = nxt_a, obs_a
        obs_b, nxt_b = nxt_b, obs_b
    print("episode ends:", dones)
    assert steps < 60 or dones >= N
    assert (a.memory.cursor, a.memory.size) == (b.memory.cursor, b.memory.size)
    for x, y in zip(a.memory.ring, b.memory.ring):
        assert torch.equal(x, y)


def test_fused_update_matches_reference(monkeypatch):
    """tests/test_trainers_gpu.py::test_dsac_update_matches_reference itself (tests/golden/dsac.npz: two consecutive reference
    update() calls; four losses <= 1e-5, log_alpha <= 1e-6, all five networks <= 5e-6) with Config.fused_step switched on."""
    from gymrl_amd import ops, sac_cartpole
    import test_trainers_gpu
    calls = []

    class FusedConfig(sac_cartpole.Config):
        def __init__(self):
            super().__init__()
            self.fused_step = True

    real = ops.dsac_update
    monkeypatch.setattr(sac_cartpole, "Config", FusedConfig)
    monkeypatch.setattr(ops, "dsac_update", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    test_trainers_gpu.test_dsac_update_matches_reference()
    assert len(calls) == 2                             # the fused update did run, both times


def _chunk_run(graphs, inject, N=64, B=128, hidden=256):
    tr = _trainer(N, B, hidden, True, graphs=graphs)
    assert tr._fused_ok()
    if inject:                  # fill the ring, then ONE update outside train(): every counter starts elsewhere in the chunks
        tr.train(max_vector_steps=8)
        tr.update()
    tr.train(max_vector_steps=64)
    torch.cuda.synchronize()
    return tr


@pytest.mark.parametrize("inject", [False, True])
def test_chunked_graph_equals_eager(inject):
    """16 vector steps replay as ONE captured graph, every per-step scalar read from the device record of its step."""
    a, b = _chunk_run(False, inject), _chunk_run(True, inject)
    assert getattr(a, "_chunk", None) is None
    assert b._chunk is not None and b._chunk.graph is not None
    assert b.critic1_optim.step_count >= 48
    _assert_same(a, b)


def _switch_schedule(fused, tmp_path=None):
    tr = _trainer(48, 64, 64, fused, graphs=None if fused else False)
    tr.train(max_vector_steps=9)
    tr.cfg.fused_step = False
    assert not tr._fused_update_ok()
    tr.update()
    tr.soft_update(tr.c1_target_flat, tr.c1_flat)
    tr.cfg.fused_step = fused
    if tmp_path is not None:        # leave the schedule for one more layer-path update, then come back by the checkpoint
        path = str(tmp_path / "dsac.pt")
        tr.save_checkpoint(path)
        tr.cfg.fused_step = False
        tr.update()
        tr.cfg.fused_step = fused
        tr.load_checkpoint(path)
    tr.train(max_vector_steps=9)
    torch.cuda.synchronize()
    return tr


def test_switching_between_the_paths(tmp_path):
    """9 fused steps, one layer-by-layer update() and a soft_update() (both leave the weight images stale), 9 more fused steps ==
    the same schedule on the layer path throughout; and a load_checkpoint() of the state saved in the middle, after a further
    update had moved everything, continues exactly like the uninterrupted run."""
    layer, fused, resumed = _switch_schedule(False), _switch_schedule(True), _switch_schedule(True, tmp_path)
    assert fused._fused is not None and fused._fused[4] is not None
    _assert_same(layer, fused, "switch")
    _assert_same(fused, resumed, "checkpoint")


def test_unsupported_batch_is_refused_and_trains_layer_by_layer():
    from gymrl_amd import _lib, ops
    out = []
    for fused in (True, False):
        tr = _trainer(64, 300, 64, fused, graphs=False)
        assert tr._fused_update_ok() is False and not tr._fused_ok()
        tr.train(max_vector_steps=8)
        torch.cuda.synchronize()
        assert tr._fused is None and tr.critic1_optim.step_count == 4
        out.append(tr)
    _assert_same(out[0], out[1])
    tr = out[0]
    m = tr.memory
    ws = ops.dsac_update_workspace(300, 4, 2, 64, tr.device)
    for B, want in ((300, -22), (257, -22)):
        a = ops.dsac_update_args(B, 4, 2, tr.actor, tr.critic1, tr.critic2, tr.critic1_target, tr.critic2_target, tr.actor_optim,
                                 tr.critic1_optim, tr.critic2_optim, m.ring, (0.9, 0.005, -1.0, 1e-3), tr.log_alpha, tr._alpha_m,
                                 tr._alpha_v, tr._sums, tr._alpha_loss, ws)
        a.idx_size, a.alpha_t = m.size, 1
        before = tr.c1_flat.clone()
        rc = _lib.lib().gymrl_dsac_update(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == want and torch.equal(before, tr.c1_flat)


def _softmax_logits(B, A, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randn(B, A, generator=g, device="cuda") * 3.0
    z[1] = 0.75                                                          # equal logits
    z[2] = -11.5
    z[3] = torch.linspace(-40.0, 40.0, A, device="cuda")                 # a +-40 spread (e^-80 is still a normal float32)
    z[4] = torch.linspace(40.0, -40.0, A, device="cuda")
    return z, torch.randn(B, A, generator=g, device="cuda")


@pytest.mark.parametrize("B,A", [(257, 2), (100, 8)])
def test_kernel_softmax_against_float64(B, A):
    """ops.softmax_rows (csrc/softmax_device.hpp) forward and backward against a float64 softmax of the same logits.  The bound
    is F.softmax's own error on the same inputs, measured here: the kernel may err twice as much (det_expf and torch's exp may
    differ by an ulp), with a floor of 2^-22 for inputs where torch happens to be exact.  Forward: the largest relative error
    of a probability.  Backward: the largest absolute error of dz over max|g| — an element-wise relative error has no bound
    where g_k and sum_j g_j p_j cancel, for torch as for the kernel."""
    import torch.nn.functional as F
    from gymrl_amd import ops
    z, g = _softmax_logits(B, A, 11 + A)
    z64 = z.double().requires_grad_(True)
    p64 = F.softmax(z64, dim=-1)
    p64.backward(g.double())
    outs = {}
    for name, fn in (("torch", lambda x: F.softmax(x, dim=-1)), ("kernel", ops.softmax_rows)):
        x = z.clone().requires_grad_(True)
        p = fn(x)
        p.backward(g)
        fwd = ((p.detach().double() - p64.detach()).abs() / p64.detach()).max().item()
        bwd = ((x.grad.double() - z64.grad).abs().max() / g.abs().max()).item()
        outs[name] = (fwd, bwd, p.detach(), x.grad)
        print(f"softmax [{B}, {A}] {name}: forward max rel err {fwd:.3e}, backward max abs err / max|g| {bwd:.3e}")
    floor = 2.0 ** -22
    assert outs["kernel"][0] <= max(2.0 * outs["torch"][0], floor)
    assert outs["kernel"][1] <= max(2.0 * outs["torch"][1], floor)
    p, dz = outs["kernel"][2], outs["kernel"][3]
    assert (p.double().sum(-1) - 1.0).abs().max().item() <= floor
    assert dz.double().sum(-1).abs().max().item() <= floor * g.abs().max().item()
    assert torch.equal(p[1], torch.full((A,), 1.0 / A, device="cuda"))   # equal logits: e_k = 1 exactly


def test_defaults_keep_torch_softmax():
    """kernel_softmax = False and fused_step = False (the defaults): Actor.forward is F.softmax of the logits, as before."""
    import torch.nn.functional as F
    from gymrl_amd import sac_cartpole
    cfg = sac_cartpole.Config()
    cfg.num_envs, cfg.hidden_dim = 8, 32
    tr = sac_cartpole.SACTrainer(cfg)
    assert tr.actor.kernel_softmax is False
    x = torch.randn(37, 4, device=tr.device)
    with torch.no_grad():
        assert torch.equal(tr.actor(x), F.softmax(tr.actor.logits(x), dim=-1))
    cfg.kernel_softmax = True
    tr2 = sac_cartpole.SACTrainer(cfg)
    assert tr2.actor.kernel_softmax is True
