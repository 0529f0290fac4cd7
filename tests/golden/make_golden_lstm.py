#!/usr/bin/env python3
"""Golden vectors for the recurrent PPO trainer's LSTM layer, from the REFERENCE's own Python (ppo_lstm_lunarlander.py
with URNN(layer=nn.LSTM)).

Runs only in the build container (needs the reference checkout; make_golden.py's stub gym and loader).  Writes
  ppo_lstm_lstm_parts.npz   the reference URNN(12, 16, layer=nn.LSTM) on a [5, 6, 12] window from a nonzero [5, 32] state
                            cat(h, c): outputs, new state, dx, dh0 (both halves), state dict and every parameter gradient
                            (the fields gen_ppo_lstm_parts records for the GRU)
  ppo_lstm_lstm_trace.npz   the reference PPOTrainer.train() for two iterations on the scripted env with the small-width
                            ActorCritic whose URNN is built with nn.LSTM (hidden 32): make_golden.gen_ppo_lstm_trace itself,
                            run with the network class and the output name swapped, so the two traces are recorded alike

    python tests/golden/make_golden_lstm.py
"""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
from make_golden import load_ref, save, seed_all  # noqa: E402


def gen_parts():
    mod = load_ref("algorithms/ppo_lstm_lunarlander.py", "ref_ppo_lstm_lstm")
    seed_all(43)
    rnn = mod.URNN(input_size=12, hidden_size=16, layer=nn.LSTM)
    x = torch.randn(5, 6, 12, requires_grad=True)
    h0 = (0.5 * torch.randn(5, 32)).requires_grad_(True)
    w_out, w_h = torch.randn(5, 6, 16), torch.randn(5, 32)
    ro, hn = rnn(x, h0)
    ((ro * w_out).sum() + (hn * w_h).sum()).backward()
    out = {"lstm_x": x.detach().numpy(), "lstm_h0": h0.detach().numpy(), "lstm_w_out": w_out.numpy(), "lstm_w_h": w_h.numpy(),
           "lstm_out": ro.detach().numpy(), "lstm_hn": hn.detach().numpy(), "lstm_dx": x.grad.numpy(),
           "lstm_dh0": h0.grad.numpy()}
    for k, v in rnn.state_dict().items():
        out["lstm_sd_" + k] = v.numpy().copy()
    for k, p in rnn.named_parameters():
        out["lstm_grad_" + k] = p.grad.numpy().copy()
    save("ppo_lstm_lstm_parts", **out)


def _small_lstm_net(mod, hidden=32, head=32, embed=64):
    """make_golden._small_lstm_ref with the URNN built on nn.LSTM."""

    class SmallActorCritic(mod.ActorCritic):
        def __init__(self, state_dim, action_dim, config=None):
            nn.Module.__init__(self)
            self.shared = mod.MHCBackbone(input_dim=state_dim, output_dim=config.mhc_dim, rate=config.mhc_rate,
                                          num_layers=config.mhc_layers, max_sk_it=config.mhc_sk_it)
            self.rnn = mod.URNN(input_size=config.mhc_dim, hidden_size=hidden, layer=nn.LSTM)
            self.actor = mod.MLP([hidden, head, action_dim], last_std=0.001)
            self.critic = mod.MLP([hidden, head, 1], last_std=1.0)
            self.rnd = mod.RND(input_dim=state_dim, embed_dim=embed)
    return SmallActorCritic


def gen_trace():
    net, write = mg._small_lstm_ref, mg.save
    mg._small_lstm_ref = _small_lstm_net
    mg.save = lambda name, **arrays: write("ppo_lstm_lstm_trace", **arrays)
    try:
        mg.gen_ppo_lstm_trace()
    finally:
        mg._small_lstm_ref, mg.save = net, write


if __name__ == "__main__":
    gen_parts()
    gen_trace()
