#!/usr/bin/env python3
"""Golden vectors for the whole-episode recurrent kernels, from the REFERENCE's own Python (ppg_rnn_lunarlander.py).

Runs only in the build container (needs the reference checkout; make_golden.py's stub gym and loader).  It drives the
reference's EpisodeBuffer.compute_advantage on ragged episodes and its PPGTrainer.update(), unmodified, on one scripted
episode per case (the network replaced by leaf tensors whose gradients are recorded at optimizer.step, clip_grad_norm_
made a no-op so the recorded gradients are the loss's own).  Writes ppg_rnn_parts.npz (f32 / f64, compressed).

    python tests/golden/make_golden_ppg.py
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import load_ref, save, seed_all  # noqa: E402

GAE_LENS = [1, 9, 21, 2, 57, 300]
GAMMA, LAM = 0.995, 0.95


def gen_gae(mod, out):
    rng = np.random.default_rng(0)
    rec = []

    class _TorchRec:                      # records the raw adv the reference builds before normalising it (:210-212)
        def __getattr__(self, k):
            return getattr(torch, k)

        def tensor(self, *a, **kw):
            t = torch.tensor(*a, **kw)
            rec.append(t.clone())
            return t

    real = mod.torch
    mod.torch = _TorchRec()
    try:
        buf = mod.EpisodeBuffer(GAMMA, LAM, "cpu")
        cols = {k: [] for k in ("rew", "val", "next_val", "done", "dw", "adv_raw", "v_target", "adv_norm")}
        for n in GAE_LENS:
            rew = (rng.normal(size=n) * 3).astype(np.float32)
            val, nv = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
            done, dw = np.zeros(n, np.float32), np.zeros(n, np.float32)
            done[-1] = 1.0
            dw[-1] = float(n % 2)
            if n > 100:
                done[n // 2] = 1.0        # a done inside the segment resets the recursion there
            t = lambda a: torch.from_numpy(a).view(-1, 1)  # noqa: E731
            rec.clear()
            adv, vt = buf.compute_advantage(t(rew), t(done), t(dw), t(val), t(nv))
            for k, v in (("rew", rew), ("val", val), ("next_val", nv), ("done", done), ("dw", dw),
                         ("adv_raw", rec[0].numpy().reshape(-1)), ("v_target", vt.numpy().reshape(-1)),
                         ("adv_norm", adv.numpy().reshape(-1))):
                cols[k].append(np.asarray(v, np.float32))
    finally:
        mod.torch = real
    out["gae_offsets"] = np.concatenate([[0], np.cumsum(GAE_LENS)]).astype(np.int64)
    out["gae_gamma_lam"] = np.array([GAMMA, LAM])
    for k, v in cols.items():
        out["gae_" + k] = np.concatenate(v)


class _Net(torch.nn.Module):
    """Stands in for ActorCriticPPG: its forward returns softmax(logits) and the two value heads as leaf tensors."""

    def __init__(self, logits, value, aux):
        super().__init__()
        self.logits = torch.nn.Parameter(torch.from_numpy(logits))
        self.value = torch.nn.Parameter(torch.from_numpy(value).view(-1, 1))
        self.aux = torch.nn.Parameter(torch.from_numpy(aux).view(-1, 1))

    def reset_hidden(self, device=None):
        pass

    def forward(self, s):
        return torch.softmax(self.logits, -1), self.value, self.aux


class _Opt:
    def __init__(self, net):
        self.net, self.grads = net, []
        self.param_groups = [{"lr": 1e-3}]

    def zero_grad(self):
        for p in self.net.parameters():
            p.grad = None

    def step(self):
        self.grads.append([(torch.zeros_like(p) if p.grad is None else p.grad).detach().clone().numpy()
                           for p in (self.net.logits, self.net.value, self.net.aux)])


class _Mem:
    def __init__(self, samples):
        self.samples = samples

    def sample(self):
        return self.samples

    def clear(self):
        pass


def _tie_old_logp(lp):
    """An f32 old log-prob that makes exp(lp - old) == 3 in f32 with the true value as close to 3 as possible (the
    torch.max(min_surr, dual_clip * adv) tie at ratio == dual_clip)."""
    base = np.float32(lp - math.log(3.0))
    best, err = None, None
    cand = base
    for _ in range(64):
        cand = np.nextafter(cand, np.float32(-np.inf))
    for _ in range(128):
        d = np.float32(np.float32(lp) - cand)
        if float(torch.exp(torch.tensor(d))) == 3.0:
            e = abs(math.exp(float(d)) - 3.0)
            if err is None or e < err:
                best, err = cand, e
        cand = np.nextafter(cand, np.float32(np.inf))
    assert best is not None
    return best


def _loss_case(mod, rng, n, k):
    M = n
    logits = (rng.normal(size=(M, 4)) * 1.5).astype(np.float32)
    act = rng.integers(0, 4, size=M).astype(np.int64)
    adv = rng.normal(size=M).astype(np.float32)
    if M >= 16:
        logits[0] = (40.0, 0.0, -1.0, 0.5)            # saturated: p0 >= 1 - eps, the rest <= eps
        logits[1] = (-30.0, 25.0, -2.0, 0.0)
        act[1] = 0                                    # the taken action clamped at eps: no gradient through its log
        logits[12:16] = 0.0                           # p = 1/4 exactly: the dual-clip tie rows below
    p = torch.softmax(torch.from_numpy(logits), -1)
    lp = torch.distributions.Categorical(p).log_prob(torch.from_numpy(act)).numpy()
    old = (lp + rng.normal(size=M) * 0.3).astype(np.float32)
    if M >= 16:
        adv[6:12] = -np.abs(adv[6:12]) - 0.5          # adv < 0, ratio e^2: the dual clip binds
        old[6:12] = lp[6:12] - 2.0
        adv[12:16] = -np.abs(adv[12:16]) - 0.5        # adv < 0, ratio exactly 3 == dual_clip: torch.max ties
        for i in range(12, 16):
            old[i] = _tie_old_logp(lp[i])
    value, aux, vt = (rng.normal(size=M).astype(np.float32) for _ in range(3))

    cfg = mod.Config()
    cfg.epochs, cfg.aux_epochs, cfg.batch_size, cfg.device = 1, 1, 1, "cpu"
    tr = object.__new__(mod.PPGTrainer)
    tr.cfg, tr.learn_step = cfg, 0
    tr.net = _Net(logits, value, aux)
    tr.optimizer = _Opt(tr.net)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).view(-1, 1)  # noqa: E731
    tr.memory = [_Mem((torch.zeros(M, 8), torch.from_numpy(act).view(-1, 1), t(old), t(adv), t(vt)))]
    m = tr.update()
    (g_pol, g_val, _), (g_aux_logits, _, g_aux) = tr.optimizer.grads
    pre = f"l{k}_"
    return {pre + "logits": logits, pre + "value": value, pre + "aux": aux, pre + "act": act.astype(np.int32),
            pre + "old_logp": old, pre + "adv": adv, pre + "v_target": vt,
            pre + "dlogits_policy": g_pol, pre + "dvalue": g_val.reshape(-1), pre + "dlogits_aux": g_aux_logits,
            pre + "daux": g_aux.reshape(-1),
            pre + "metrics": np.array([m["total_loss"], m["clip_loss"], m["value_loss"], m["entropy_loss"], m["advantage"],
                                       m["aux_value_loss"]], np.float64)}


def main():
    seed_all(0)
    mod = load_ref("algorithms/ppg_rnn_lunarlander.py", "ref_ppg_rnn")
    out = {}
    gen_gae(mod, out)
    clip = torch.nn.utils.clip_grad_norm_
    torch.nn.utils.clip_grad_norm_ = lambda *a, **kw: torch.tensor(0.0)   # the recorded gradients are the loss's own
    try:
        rng = np.random.default_rng(1)
        for k, n in enumerate((37, 1, 64)):
            out.update(_loss_case(mod, rng, n, k))
    finally:
        torch.nn.utils.clip_grad_norm_ = clip
    cfg = mod.Config()
    out["loss_cfg"] = np.array([cfg.clip, cfg.dual_clip, cfg.val_coef, cfg.ent_coef, cfg.beta_clone], np.float64)
    out["loss_cases"] = np.array([3], np.int32)
    save("ppg_rnn_parts", **out)


if __name__ == "__main__":
    main()
