#!/usr/bin/env python3
"""Golden vectors for the two PER trainers, from the REFERENCE's own Python (ddqn_per_cartpole.py, ddqn_per_duel_cartpole.py).

Runs only in the build container (needs the reference checkout; make_golden.py's stub gym and loader).  For each script: hidden
32, batch 32, capacity 32, the memory filled with exactly the batch, the target de-correlated from the policy as gen_dqn_update
does, then two consecutive update() calls under random.seed.  Recorded: the stratified uniforms (random.uniform(a, b) is
a + (b - a) * random.random(): the same stream re-drawn after the same seed), the sampled tree indices, the importance weights,
both losses, |td| as update_priorities received it, the tree after each update, beta, and the state dicts before and after.
Writes ddqn_per_update.npz; keys carry the prefix "ddqn_" or "duel_".

    python tests/golden/make_golden_ddqn.py
"""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import load_ref, save, seed_all  # noqa: E402

B = CAP = HIDDEN = 32
SEED_NET, SEED_DRAW = 71, 6


def gen(relpath, modname, trainer_name, prefix, out):
    mod = load_ref(relpath, modname)
    cfg = mod.Config()
    cfg.device, cfg.batch_size, cfg.hidden_dim, cfg.memory_capacity = "cpu", B, HIDDEN, CAP
    seed_all(SEED_NET)
    tr = getattr(mod, trainer_name)(cfg)
    rng = np.random.default_rng(SEED_NET)
    trans = []
    for _ in range(B):
        trans.append((rng.normal(size=4).astype(np.float32), int(rng.integers(0, 2)), float(rng.normal()),
                      rng.normal(size=4).astype(np.float32), bool(rng.random() < 0.2)))
        tr.memory.push(trans[-1])
    with torch.no_grad():   # de-correlate target from policy
        for p in tr.target_net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    sd = lambda net: {k: v.numpy().copy() for k, v in net.state_dict().items()}  # noqa: E731
    states = {"p0_": sd(tr.policy_net), "t0_": sd(tr.target_net)}
    rec = {k: [] for k in ("indices", "abs_td", "is_weight", "tree", "beta", "loss")}
    real_update, real_sample = tr.memory.update_priorities, tr.memory.sample

    def sample(batch_size):
        batch, indices, w = real_sample(batch_size)
        rec["is_weight"].append(np.asarray(w, np.float64).copy())
        return batch, indices, w

    def update_priorities(indices, errors):
        rec["indices"].append(np.asarray(indices, np.int32).copy())
        rec["abs_td"].append(np.asarray(errors, np.float32).copy())
        real_update(indices, errors)

    tr.memory.sample, tr.memory.update_priorities = sample, update_priorities
    tree0 = tr.memory.tree.tree.copy()
    random.seed(SEED_DRAW)
    for k in (1, 2):
        rec["loss"].append(tr.update())
        rec["tree"].append(tr.memory.tree.tree.copy())
        rec["beta"].append(cfg.beta)
        states[f"p{k}_"] = sd(tr.policy_net)
    random.seed(SEED_DRAW)
    u = np.array([[random.random() for _ in range(B)] for _ in range(2)])
    o = dict(u=u, indices=np.stack(rec["indices"]), abs_td=np.stack(rec["abs_td"]), is_weight=np.stack(rec["is_weight"]),
             tree0=tree0, tree=np.stack(rec["tree"]), beta=np.array(rec["beta"]), loss=np.array(rec["loss"], np.float64),
             states=np.stack([t[0] for t in trans]), actions=np.array([t[1] for t in trans], np.int32),
             rewards=np.array([t[2] for t in trans], np.float32), next_states=np.stack([t[3] for t in trans]),
             dones=np.array([t[4] for t in trans], np.uint8), gamma=np.float64(cfg.gamma), lr=np.float64(cfg.lr),
             alpha=np.float64(cfg.alpha), eps=np.float64(cfg.eps), error_max=np.float64(cfg.error_max),
             beta0=np.float64(0.4), beta_increment=np.float64(cfg.beta_increment))
    for pre, d in states.items():
        for k, v in d.items():
            o[pre + k] = v
    for k, v in o.items():
        out[prefix + k] = v


if __name__ == "__main__":
    out = {}
    gen("algorithms/ddqn_per_cartpole.py", "ref_ddqn_per", "DDQNPERTrainer", "ddqn_", out)
    gen("algorithms/ddqn_per_duel_cartpole.py", "ref_ddqn_per_duel", "DDQNPERDuelTrainer", "duel_", out)
    save("ddqn_per_update", **out)
