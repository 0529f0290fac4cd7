"""Micro-benchmark: the GRU recurrence over whole episodes, fused (gymrl_gru_seq_fwd + _bwd: one launch per direction)
against the per-step composition (one F.linear + one gymrl_gru_cell_fwd / _bwd launch per step and direction), at
T = 1000 steps, H = 64, G in {4, 16, 64} full-length episodes.  Prints one JSON line per G (milliseconds per
forward + backward, median of the timed repetitions)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gymrl_amd import ops  # noqa: E402


def per_step(gi, W, b, h0):
    T = gi.shape[0]
    h, hs = h0, []
    for t in range(T):
        h = ops.gru_cell_fwd(gi[t], torch.nn.functional.linear(h, W, b).contiguous(), h)
        hs.append(h)
    dh = torch.ones_like(h0)
    for t in range(T - 1, -1, -1):
        hp = h0 if t == 0 else hs[t - 1]
        _, dgh, ddir = ops.gru_cell_bwd(gi[t], torch.nn.functional.linear(hp, W, b).contiguous(), hp, dh)
        dh = ddir + dgh @ W


def fused(gi, W, b, h0, lens, d_hlast):
    h_seq, _ = ops.gru_seq_fwd(gi, W, b, lens, h0=h0)
    ops.gru_seq_bwd(gi, W, b, h_seq, lens, d_hlast=d_hlast, h0=h0)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        z.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(z))
    out.sort()
    return out[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--H", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    for G in (4, 16, 64):
        T, H = args.T, args.H
        gi = torch.randn(T, G, 3 * H, generator=g).to(dev)
        W = (torch.randn(3 * H, H, generator=g) * 0.2).to(dev)
        b = torch.randn(3 * H, generator=g).to(dev)
        h0 = torch.zeros(G, H, device=dev)
        lens = [T] * G
        d_hlast = torch.ones(G, H, device=dev)
        fused(gi, W, b, h0, lens, d_hlast)
        per_step(gi, W, b, h0)
        torch.cuda.synchronize()
        tf = timed(lambda: fused(gi, W, b, h0, lens, d_hlast), args.reps)
        ts = timed(lambda: per_step(gi, W, b, h0), max(2, args.reps // 2))
        print(json.dumps({"G": G, "T": T, "H": H, "fused_ms": round(tf, 3), "per_step_ms": round(ts, 3),
                          "fused_us_per_step": round(1000 * tf / T, 3), "speedup": round(ts / tf, 2)}), flush=True)


if __name__ == "__main__":
    main()
