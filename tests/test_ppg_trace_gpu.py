"""Replay of the reference's PPGTrainer.train() / PPORNNTrainer.train() traces (tests/golden/make_golden_ppg_trace.py:
scripted env, batch_size 4, 8 episodes = two updates, epochs 2 + aux_epochs 2, seed None) through this repo's trainers at
num_envs = 1, episodes_per_minibatch = 1: the fixture's initial weights, its Exp(1) draws and its permutations.

Integers are exact: episode lengths, actions, dones, dw, learn_step, the per-parameter Adam step counts (torch.optim.Adam
skips grad-None parameters; the critic / aux head ranges here) and the raw returns (the script's rewards are multiples of
1/4).  Floats, and why these bounds:
  * normalised states and scaled rewards: gymrl_running_norm / gymrl_reward_scaling restate the reference's f32 mean /
    f64 S, std arithmetic; the reference keeps the scaled reward in f64, this trainer in f32 -> 1e-6 relative.
  * log-probs, values, next values, adv, v_target, grad norms, metrics: the network runs in f32 with other summation
    orders (MFMA tiles when acting, library GEMMs and the GRU kernels in the update, f32 vs the reference's CPU f32), and
    from the second batch on the weights themselves differ by a few f32 ulps after 16 Adam steps -> TOL below.  Observed
    worst cases on one MI355X: log-prob 4.1e-5 absolute (|logp| ~ 1, 5x inside TOL), values 3.8e-6, adv 3.3e-6, grad
    norms 9.9e-6 relative; states exact, scaled rewards 9e-8.  Metrics such as the clip loss sit near zero, where only the
    absolute part of TOL is meaningful.
  * the weights after the second update (full small tensors, the first 4 rows and the norm of the large ones): Adam's
    first steps move each weight by ~lr = 1e-3 whatever the gradient's size, so last-bit gradient differences show up
    as ~1e-7 absolute (observed 6.0e-7); 2e-5 absolute leaves a 30x margin."""
import os

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = dict(rtol=2e-4, atol=2e-5)
TOL_SD = dict(rtol=0, atol=2e-5)


class _RoundScriptedEnv:
    """The scripted env behind VecEnv's device interface with GymView's reset rule: the stepper auto-resets after a done,
    and the reset() that starts the next round hands out that already-started episode instead of skipping it.  An env
    whose episode has ended is not stepped again until then (the trainer masks it; this keeps the script's episode
    numbering equal to the reference's sequential one)."""

    def __init__(self, n, device):
        import sys
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from scripted_env import ScriptedEnv
        self.envs = [ScriptedEnv(8, 4) for _ in range(n)]
        self.n, self.device = n, device
        self.obs_dim, self.act_dim, self.max_steps = 8, 4, 500
        self.seed, self.env_id0 = 0, 0
        self.ended = [False] * n

    def _put(self, dst, arr):
        dst.copy_(torch.from_numpy(np.asarray(arr)).to(self.device))

    def reset(self, obs_out=None, seed=None):
        for i, e in enumerate(self.envs):
            if not self.ended[i]:
                e.reset(seed=seed)
            self.ended[i] = False
        obs = np.stack([e._obs() for e in self.envs])
        if obs_out is None:
            return torch.from_numpy(obs).to(self.device)
        self._put(obs_out, obs)
        return obs_out

    def step(self, action, obs_out, rew_out, term_obs_out=None, terminated_out=None, truncated_out=None, **_):
        acts = action.tolist()
        obs, tobs = np.zeros((self.n, 8), np.float32), np.zeros((self.n, 8), np.float32)
        rew, te, tr = np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8), np.zeros(self.n, np.uint8)
        for i, e in enumerate(self.envs):
            if self.ended[i]:
                obs[i] = tobs[i] = e._obs()
                continue
            o, r, a, b, _ = e.step(acts[i])
            tobs[i], rew[i], te[i], tr[i] = o, r, a, b
            if a or b:
                self.ended[i] = True
                o, _ = e.reset()
            obs[i] = o
        self._put(obs_out, obs)
        self._put(rew_out, rew)
        for dst, src in ((term_obs_out, tobs), (terminated_out, te), (truncated_out, tr)):
            if dst is not None:
                self._put(dst, src)

    def close(self):
        pass


def _replay(tmp_path, modname, fixture):
    import importlib
    mod = importlib.import_module(f"gymrl_amd.{modname}")
    d = np.load(os.path.join(ROOT, "tests", "golden", fixture))
    cfg = mod.Config()
    cfg.batch_size, cfg.max_episodes, cfg.epochs, cfg.seed = 4, 8, 2, None
    if hasattr(cfg, "aux_epochs"):
        cfg.aux_epochs = 2
    cfg.num_envs, cfg.episodes_per_minibatch = 1, 1
    cfg.save_path = str(tmp_path / "ck.pth")
    tr = (mod.PPGTrainer if hasattr(mod, "PPGTrainer") else mod.PPORNNTrainer)(cfg)
    with torch.no_grad():
        tr.net.load_state_dict({k[5:]: torch.from_numpy(d[k]) for k in d if k.startswith("init_")})
    tr.env = _RoundScriptedEnv(1, tr.device)
    lengths = [int(n) for k in ("u0_lengths", "u1_lengths") for n in d[k]]
    starts = np.concatenate([[0], np.cumsum(np.array(lengths) + 1)])
    noise = torch.from_numpy(d["noise_exp"]).to(tr.device)
    ones = torch.ones(1, 4, device=tr.device)

    def draws(rnd, t):        # episode rnd's draw t: the reset state's (t = 0), then one per step; past the end: unused
        return noise[starts[rnd] + t].view(1, 4) if t <= lengths[rnd] else ones
    tr._parity_noise = draws
    tr._parity_perms = iter(d["perms"])
    tr.grad_norms = []
    recs = []
    orig = tr.update

    def update():
        g0 = len(tr.grad_norms)
        m = orig()
        recs.append((tr.last_sample, list(tr.grad_norms[g0:]), m, tr.learn_step, tr.param_steps()))
        return m
    tr.update = update
    tr.train()
    return tr, d, recs


def _check(tr, d, recs):
    assert len(recs) == 2
    for k, (b, gn, m, ls, steps) in enumerate(recs):
        u = lambda f: d[f"u{k}_{f}"]     # noqa: E731
        assert b["lengths"] == u("lengths").tolist()
        assert np.array_equal(b["act"].cpu().numpy(), u("actions"))
        assert np.array_equal(b["done"].cpu().numpy(), u("dones")) and np.array_equal(b["dw"].cpu().numpy(), u("dw"))
        assert ls == int(u("learn_step")) and steps == u("adam_steps").tolist()
        np.testing.assert_allclose(b["states"].cpu().numpy(), u("states"), rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(b["rew"].cpu().numpy(), u("rewards"), rtol=1e-6, atol=1e-7)
        for ours, ref in (("logp", "log_probs"), ("value", "values"), ("next_value", "next_values"), ("adv", "adv"),
                          ("v_target", "v_target")):
            np.testing.assert_allclose(b[ours].cpu().numpy(), u(ref), err_msg=f"u{k} {ours}", **TOL)
        np.testing.assert_allclose(gn, u("grad_norms"), err_msg=f"u{k} grad norms", **TOL)
        for name in m:
            np.testing.assert_allclose(m[name], float(u("metric_" + name)), err_msg=f"u{k} {name}", **TOL)
        assert set(m) == {f[len(f"u{k}_metric_"):] for f in d if f.startswith(f"u{k}_metric_")}
    assert list(tr.episode_rewards) == d["episode_rewards"].tolist()
    sd = {k: v.detach().cpu().numpy() for k, v in tr.net.state_dict().items()}
    for k, v in sd.items():
        if "final_" + k in d:
            np.testing.assert_allclose(v, d["final_" + k], err_msg=k, **TOL_SD)
        else:
            np.testing.assert_allclose(v[:4], d[f"final_{k}__rows4"], err_msg=k, **TOL_SD)
            np.testing.assert_allclose(np.linalg.norm(v.astype(np.float64)), float(d[f"final_{k}__norm"]), rtol=1e-5)


def test_ppg_rnn_replays_reference_trace(tmp_path):
    tr, d, recs = _replay(tmp_path, "ppg_rnn_lunarlander", "ppg_rnn_trace.npz")
    _check(tr, d, recs)
    # per update: trunk + actor 16 steps, critic 8 (policy phase only), aux head 8 (aux phase only)
    assert tr.optimizer.steps == {"critic": 16, "trunk": 32, "aux": 16}


def test_ppo_rnn_replays_reference_trace(tmp_path):
    tr, d, recs = _replay(tmp_path, "ppo_rnn_lunarlander", "ppo_rnn_trace.npz")
    _check(tr, d, recs)
    assert tr.optimizer.steps == {"critic": 16, "trunk": 16}


def test_choose_action_carries_the_hidden_state_like_the_reference(tmp_path):
    """choose_action(state) on one observation returns python scalars and carries net.rnn_h across calls, as the
    reference's does (:311-320); net.reset_hidden() starts over."""
    from gymrl_amd import ppg_rnn_lunarlander as ppg
    cfg = ppg.Config()
    cfg.save_path = str(tmp_path / "ck.pth")
    tr = ppg.PPGTrainer(cfg)
    s = np.linspace(-1, 1, 8).astype(np.float32)
    tr.net.reset_hidden()
    a, lp, v1 = tr.choose_action(s)
    assert isinstance(a, int) and isinstance(lp, float) and isinstance(v1, float)
    h1 = tr.net.rnn_h.clone()
    assert h1.abs().sum() > 0
    v2 = tr.choose_action(s)[2]
    assert v2 != v1                                  # same input, carried state
    tr.net.reset_hidden()
    assert tr.choose_action(s)[2] == v1 and torch.equal(tr.net.rnn_h, h1)
    with torch.no_grad():                            # the torch composition from the same state agrees
        tr.net.reset_hidden()
        _, v_ref, _ = tr.net(torch.from_numpy(s).cuda().unsqueeze(0))
    assert abs(float(v_ref) - v1) < 1e-4
