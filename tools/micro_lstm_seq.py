"""Micro-benchmark: the LSTM recurrence, fused (gymrl_lstm_seq_fwd + _bwd: one launch per direction) against the per-step
composition (one F.linear + one gymrl_lstm_cell_fwd / _bwd launch per step and direction, plus the dgates . W_hh GEMM of
the reverse pass) in the same process, at the trainer's window shape (T = 8, B = 128, H = 64) and at whole-episode shapes
(T = 1000, B in {4, 16, 64}, H = 64).  Prints one JSON line per shape (milliseconds per forward + backward by device
events, median of the timed repetitions after a warm-up of both)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gymrl_amd import ops  # noqa: E402


def per_step(gi, W, b, h0, c0):
    T = gi.shape[0]
    h, c, hs, cs = h0, c0, [], []
    for t in range(T):
        h, c = ops.lstm_cell_fwd(gi[t], torch.nn.functional.linear(h, W, b).contiguous(), c)
        hs.append(h)
        cs.append(c)
    dh, dc = torch.ones_like(h0), torch.zeros_like(c0)
    for t in range(T - 1, -1, -1):
        hp, cp = (h0, c0) if t == 0 else (hs[t - 1], cs[t - 1])
        dgates, dc = ops.lstm_cell_bwd(gi[t], torch.nn.functional.linear(hp, W, b).contiguous(), cp, dh, dc)
        dh = dgates @ W


def fused(gi, W, b, h0, c0, lens, d_hlast):
    h_seq, c_seq, _, _ = ops.lstm_seq_fwd(gi, W, b, lens, h0=h0, c0=c0)
    ops.lstm_seq_bwd(gi, W, b, h_seq, c_seq, lens, d_hlast=d_hlast, h0=h0, c0=c0)


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
    ap.add_argument("--H", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    H = args.H
    for what, T, B in (("window", 8, 128), ("episode", 1000, 4), ("episode", 1000, 16), ("episode", 1000, 64)):
        gi = torch.randn(T, B, 4 * H, generator=g).to(dev)
        W = (torch.randn(4 * H, H, generator=g) * 0.2).to(dev)
        b = torch.randn(4 * H, generator=g).to(dev)
        h0, c0 = torch.zeros(B, H, device=dev), torch.zeros(B, H, device=dev)
        lens = [T] * B
        d_hlast = torch.ones(B, H, device=dev)
        fused(gi, W, b, h0, c0, lens, d_hlast)
        per_step(gi, W, b, h0, c0)
        torch.cuda.synchronize()
        tf = timed(lambda: fused(gi, W, b, h0, c0, lens, d_hlast), args.reps)
        ts = timed(lambda: per_step(gi, W, b, h0, c0), args.reps)
        print(json.dumps({"shape": what, "T": T, "B": B, "H": H, "fused_ms": round(tf, 3), "per_step_ms": round(ts, 3),
                          "fused_us_per_step": round(1000 * tf / T, 3), "speedup": round(ts / tf, 2)}), flush=True)


if __name__ == "__main__":
    main()
