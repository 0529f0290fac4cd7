#!/usr/bin/env python3
"""Training traces of the REFERENCE's PPGTrainer.train() (ppg_rnn_lunarlander.py:431-499) and PPORNNTrainer.train()
(ppo_rnn_lunarlander.py), run unmodified on the scripted env (ScriptedEnv(8, 4) behind make_golden.py's stub gym) with
batch_size 4, max_episodes 8 (two updates), epochs 2, aux_epochs 2, seed None, in a temporary directory (they save
./checkpoints/...).  Runs only in the build container (needs the reference checkout).

Recorded (ppg_rnn_trace.npz / ppo_rnn_trace.npz, compressed):
  init_<key>        the initial state_dict
  noise_exp         every Exp(1) draw Categorical.sample consumed, f32[draws, 4], in call order (the replay of each draw
                    is asserted to reproduce the reference's action)
  perms             every np.random.permutation, i32[n, batch_size], in call order
  u<k>_<field>      per update k: the buffers in episode order (states = normalised, actions, rewards = scaled, dones,
                    dw, log_probs, values, next_values), lengths, adv, v_target, grad_norms (pre-clip, every optimiser
                    step), the metrics dict (metric_<name>), learn_step, and the Adam state's per-parameter step
  final_<key>       the state_dict after the last update: every tensor of <= 4096 elements in full, the first 4 rows of
                    the larger ones (<key>__rows4) and their float64 L2 norm (<key>__norm) — the full intermediate and final
                    state_dicts would take the file past 1 MiB
  episode_rewards   raw returns in episode order

    python tests/golden/make_golden_ppg_trace.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, load_ref, save, seed_all  # noqa: E402

BIG = 4096


def _trace(relpath, modname, trainer_cls, has_aux, name):
    sys.path.insert(0, os.path.dirname(OUT))
    from scripted_env import ScriptedEnv
    mod = load_ref(relpath, modname)
    sys.modules[modname] = mod                     # save_model pickles the reference's Normalization object
    sys.modules["gymnasium"].make = lambda n, **kw: ScriptedEnv(8, 4)
    cfg = mod.Config()
    cfg.batch_size, cfg.max_episodes, cfg.epochs, cfg.seed, cfg.device = 4, 8, 2, None, "cpu"
    if has_aux:
        cfg.aux_epochs = 2
    seed_all(0)
    cwd = os.getcwd()
    tmp = tempfile.mkdtemp()
    os.chdir(tmp)
    try:
        tr = getattr(mod, trainer_cls)(cfg)
        out = {"init_" + k: v.numpy().copy() for k, v in tr.net.state_dict().items()}
        noise, perms, gnorms, upd = [], [], [], []
        orig_choose = tr.choose_action

        def choose_action(state):
            h_before = tr.net.rnn_h.clone()
            st = torch.get_rng_state()
            a, lp, v = orig_choose(state)
            after = torch.get_rng_state()
            h_after = tr.net.rnn_h
            torch.set_rng_state(st)
            q = torch.empty(1, 4).exponential_(1.0)
            torch.set_rng_state(after)
            with torch.no_grad():                  # the probs the draw saw, from the same hidden state
                tr.net.rnn_h = h_before
                prob = tr.net(torch.tensor(state, dtype=torch.float).unsqueeze(0))[0]
                tr.net.rnn_h = h_after
            p2 = prob / prob.sum(-1, keepdim=True)
            assert int(torch.argmax(p2 / q)) == a, "the Exp(1) replay must reproduce the reference's action"
            noise.append(q.numpy()[0].copy())
            return a, lp, v
        tr.choose_action = choose_action
        orig_perm, orig_clip = np.random.permutation, mod.nn.utils.clip_grad_norm_

        def permutation(n):
            r = orig_perm(n)
            perms.append(np.asarray(r, np.int32))
            return r

        def clip(params, max_norm, *a, **k):
            tn = orig_clip(params, max_norm, *a, **k)
            gnorms.append(float(tn))
            return tn
        orig_update = tr.update

        def update():
            rec = {}
            fields = ("states", "actions", "rewards", "dones", "dw", "log_probs", "values", "next_values")
            cols = {f: [] for f in fields}
            lengths, advs, vts = [], [], []
            for m in tr.memory:
                lengths.append(len(m.buffer))
                for f, col in zip(fields, zip(*m.buffer)):
                    cols[f].extend(col)
                _, _, _, adv, vt = m.sample()
                advs.append(adv.numpy().reshape(-1))
                vts.append(vt.numpy().reshape(-1))
            rec["states"] = np.array(cols["states"], np.float32)
            rec["actions"] = np.array(cols["actions"], np.int32)
            for f in ("rewards", "log_probs", "values", "next_values"):     # the scaled reward is a shape-(1,) array
                rec[f] = np.array(cols[f], np.float64).reshape(-1)
            rec["dones"] = np.array(cols["dones"], np.uint8)
            rec["dw"] = np.array(cols["dw"], np.uint8)
            rec["lengths"] = np.array(lengths, np.int64)
            rec["adv"], rec["v_target"] = np.concatenate(advs), np.concatenate(vts)
            g0 = len(gnorms)
            metrics = orig_update()
            rec["grad_norms"] = np.array(gnorms[g0:], np.float64)
            for k, v in metrics.items():
                rec["metric_" + k] = np.float64(v)
            rec["learn_step"] = np.int64(tr.learn_step)
            st = tr.optimizer.state_dict()["state"]
            rec["adam_steps"] = np.array([int(st[i]["step"]) if i in st else 0
                                          for i in range(len(list(tr.net.parameters())))], np.int64)
            upd.append(rec)
            return metrics
        tr.update = update
        np.random.permutation, mod.nn.utils.clip_grad_norm_ = permutation, clip
        try:
            tr.train()
        finally:
            np.random.permutation, mod.nn.utils.clip_grad_norm_ = orig_perm, orig_clip
    finally:
        os.chdir(cwd)
    assert len(upd) == 2
    out["noise_exp"] = np.stack(noise).astype(np.float32)
    out["perms"] = np.stack(perms)
    for k, rec in enumerate(upd):
        for f, v in rec.items():
            out[f"u{k}_{f}"] = v
    for k, v in tr.net.state_dict().items():
        a = v.numpy()
        if a.size <= BIG:
            out["final_" + k] = a.copy()
        else:
            out[f"final_{k}__rows4"] = a[:4].copy()
            out[f"final_{k}__norm"] = np.float64(np.linalg.norm(a.astype(np.float64)))
    out["episode_rewards"] = np.array(tr.episode_rewards, np.float64)
    save(name, **out)


def main():
    _trace("algorithms/ppg_rnn_lunarlander.py", "ref_ppg_rnn_trace", "PPGTrainer", True, "ppg_rnn_trace")
    _trace("algorithms/ppo_rnn_lunarlander.py", "ref_ppo_rnn_trace", "PPORNNTrainer", False, "ppo_rnn_trace")


if __name__ == "__main__":
    main()
