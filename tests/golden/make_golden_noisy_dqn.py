#!/usr/bin/env python3
"""Golden vectors for the NoisyNet dueling DQN trainer, from the REFERENCE's own Python (algorithms/noisy_dqn_cartpole.py).

Runs only in the build container (needs the reference checkout; make_golden.py's stub gym and loader).  Hidden 32, batch 32,
capacity 32, the memory filled with exactly the batch, the target de-correlated from the policy as make_golden_ddqn.py does,
then two consecutive update() calls under random.seed.

Two things are replaced on the reference's NoisyLinear:
  * `_scale_noise` records the raw torch.randn vector it draws (the value it returns is unchanged);
  * `reset_noise` REBINDS weight_epsilon / bias_epsilon to new tensors instead of copy_() into them.  This is the one change
    that lets the script's own update() run: as written, the no_grad forward on next_states overwrites — in place — the noise
    tensors the first forward saved for the gradient of sigma, and loss.backward() raises "modified by an inplace operation".
    With the rebinding the gradient flows through the noise of policy_net(states), the first draw: the intended semantics.

Recorded per update: the 16 raw vectors (two training-mode forwards x four layers x (in, out), in the forward's order fc1, fc2,
value_stream, advantage_stream) concatenated into one row, the sampled order (ring rows, found by matching the sampled states),
loss and q_mean, and the state dicts before and after.  Also one select_action in each mode on one state, with the 8 raw
vectors of the noisy forward and the Q values of both; the state is chosen so that both Q gaps exceed 1e-4 (asserted).
Writes noisy_dqn_update.npz.

    python tests/golden/make_golden_noisy_dqn.py
"""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import load_ref, save, seed_all  # noqa: E402

B = CAP = HIDDEN = 32
SEED_NET, SEED_DRAW = 83, 9
Q_GAP = 1e-4


def main():
    mod = load_ref("algorithms/noisy_dqn_cartpole.py", "ref_noisy_dqn")
    raws = []

    def _scale_noise(self, size):
        x = torch.randn(size, device=self.weight_mu.device)
        raws.append(x.numpy().copy())
        return x.sign() * x.abs().sqrt()

    def reset_noise(self):
        epsilon_i = self._scale_noise(self.in_features)
        epsilon_j = self._scale_noise(self.out_features)
        self.weight_epsilon = torch.outer(epsilon_j, epsilon_i)      # rebound, not copy_(): see the docstring
        self.bias_epsilon = epsilon_j.clone()

    mod.NoisyLinear._scale_noise, mod.NoisyLinear.reset_noise = _scale_noise, reset_noise
    cfg = mod.Config()
    cfg.device, cfg.batch_size, cfg.hidden_dim, cfg.memory_capacity = "cpu", B, HIDDEN, CAP
    seed_all(SEED_NET)
    tr = mod.NoisyDQNTrainer(cfg)
    rng = np.random.default_rng(SEED_NET)
    trans = []
    for _ in range(B):
        trans.append((rng.normal(size=4).astype(np.float32), int(rng.integers(0, 2)), float(rng.normal()),
                      rng.normal(size=4).astype(np.float32), bool(rng.random() < 0.2)))
        tr.memory.push(*trans[-1])
    with torch.no_grad():   # de-correlate target from policy
        for p in tr.target_net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    sd = lambda net: {k: v.numpy().copy() for k, v in net.state_dict().items()}  # noqa: E731
    states = {"p0_": sd(tr.policy_net), "t0_": sd(tr.target_net)}
    order, real_sample = [], tr.memory.sample
    all_states = np.stack([t[0] for t in trans])

    def sample(batch_size):
        out = real_sample(batch_size)
        rows = [int(np.flatnonzero((all_states == s).all(axis=1))[0]) for s in out[0]]
        order.append(np.array(rows, np.int32))
        return out

    tr.memory.sample = sample
    raw_rows, losses, q_means = [], [], []
    random.seed(SEED_DRAW)
    for k in (1, 2):
        del raws[:]
        m = tr.update()
        assert len(raws) == 16
        raw_rows.append(np.concatenate(raws))
        losses.append(m["loss"])
        q_means.append(m["q_mean"])
        states[f"p{k}_"] = sd(tr.policy_net)
    # select_action in both modes, on the first probe state whose two Q gaps are wide enough for the argmax to be no tie
    probe = np.random.default_rng(SEED_NET + 1).normal(size=(64, 4)).astype(np.float32)
    chosen = None
    for s in probe:
        del raws[:]
        with torch.no_grad():
            x = torch.tensor(s).unsqueeze(0)
            a_noisy = tr.select_action(s)
            act_raw = np.concatenate(raws)
            assert len(raws) == 8
            # the Q values of that very forward: the same noise again (rebinding left the tensors in place)
            net = tr.policy_net
            q_noisy = _forward_with_current_noise(net, x)
            net.eval()
            q_det = net(x).numpy()[0].copy()
            net.train()
        n0 = len(raws)
        a_det = tr.select_action(s, deterministic=True)
        assert len(raws) == n0                                     # mu only: no draw
        if abs(q_noisy[0] - q_noisy[1]) > Q_GAP and abs(q_det[0] - q_det[1]) > Q_GAP:
            assert a_noisy == int(np.argmax(q_noisy)) and a_det == int(np.argmax(q_det))
            chosen = (s, act_raw, q_noisy, q_det, a_noisy, a_det)
            break
    assert chosen is not None, "no probe state with both Q gaps > 1e-4"
    o = dict(raw=np.stack(raw_rows), order=np.stack(order), loss=np.array(losses, np.float64), q_mean=np.array(q_means, np.float64),
             states=all_states, actions=np.array([t[1] for t in trans], np.int32),
             rewards=np.array([t[2] for t in trans], np.float32), next_states=np.stack([t[3] for t in trans]),
             dones=np.array([t[4] for t in trans], np.uint8), gamma=np.float64(cfg.gamma), lr=np.float64(cfg.lr),
             sigma_init=np.float64(cfg.sigma_init), act_state=chosen[0], act_raw=chosen[1], act_q_noisy=chosen[2],
             act_q_det=chosen[3], act_noisy=np.int32(chosen[4]), act_det=np.int32(chosen[5]))
    for pre, d in states.items():
        for k, v in d.items():
            o[pre + k] = v
    save("noisy_dqn_update", **o)


def _forward_with_current_noise(net, x):
    """The training-mode forward with the epsilon tensors as they stand (no new draw)."""
    import torch.nn.functional as F

    def lin(m, h):
        return F.linear(h, m.weight_mu + m.weight_sigma * m.weight_epsilon, m.bias_mu + m.bias_sigma * m.bias_epsilon)

    h = F.relu(lin(net.fc2, F.relu(lin(net.fc1, x))))
    v, a = lin(net.value_stream, h), lin(net.advantage_stream, h)
    return (v + (a - a.mean(dim=-1, keepdim=True))).numpy()[0].copy()


if __name__ == "__main__":
    main()
