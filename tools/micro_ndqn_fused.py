"""Time per vector step of train() for noisy_dqn_cartpole.NoisyDQNTrainer: the fused step (Config.fused_step,
csrc/noisy_dqn_step.hip, sixteen steps per hipGraph replay) against the layer-by-layer path with its update replayed as a
hipGraph (use_graphs = True), on one library.

    python tools/micro_ndqn_fused.py --out profiles/ndqn_fused_micro.jsonl

Method: tools/micro_dqn_fused.py's.  One trainer per variant; a warm-up train() call fills the ring, loads the code objects and
captures the graphs; then `--runs` timed train(max_vector_steps=steps) calls, each a host clock around work that ends in a
device synchronise; the figure is the MEDIAN run.  The variants of a shape alternate inside each of `--pairs` rounds, so that a
drift of the machine falls on both.  Each trainer gets an episode_rewards deque of 99 entries, which the stop rule (it asks for
100) never accepts; every line carries its count of optimiser steps, which must equal the steps asked for.  A run with no GPU
fails: there is no CPU figure.  Lines are appended to --out as JSON."""
import argparse
import collections
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(8192, 64, 64, 1024), (64, 64, 64, 2048)]      # (N, B, hidden, timed steps)


def _make(N, B, H, fused):
    from gymrl_amd import noisy_dqn_cartpole as mod
    cfg = mod.Config()
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed = N, B, H, 0
    cfg.max_episodes, cfg.use_graphs, cfg.fused_step = 10 ** 9, True, fused
    cfg.memory_capacity = max(cfg.memory_capacity, 4 * N)
    tr = mod.NoisyDQNTrainer(cfg)
    assert tr._fused_ok() == fused
    return tr


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=48)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_ndqn_fused: needs an MI355X; there is no CPU figure")
    box = f"1x {torch.cuda.get_device_name(0)}, torch {torch.__version__}"
    lines = []
    for N, B, H, steps in SHAPES:
        trainers = {}
        for name, fused in (("layer_graphed", False), ("fused", True)):
            tr = _make(N, B, H, fused)
            tr.train(max_vector_steps=max(args.warmup, (B + N - 1) // N + 32))     # fills the ring, captures the graphs
            torch.cuda.synchronize()
            tr.episode_rewards = collections.deque(maxlen=99)
            trainers[name] = tr
        for pair in range(args.pairs):
            for name, tr in trainers.items():
                runs, before = [], tr.optimizer.step_count
                for _ in range(args.runs):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tr.train(max_vector_steps=steps)
                    torch.cuda.synchronize()
                    runs.append((time.perf_counter() - t0) * 1e3 / steps)
                done = tr.optimizer.step_count - before
                assert done == args.runs * steps, (name, done)      # no call returned early
                lines.append(dict(what="vector_step", variant=name, tree=args.tag, N=N, B=B, H=H, steps=steps,
                                  ms_per_step=round(statistics.median(runs), 4), ms_per_step_runs=[round(r, 4) for r in runs],
                                  chunk_graphs=len(getattr(tr, "_chunks", {})), updates=done, box=box, pair=pair))
                print(json.dumps(lines[-1]), flush=True)
        ms = {n: [ln["ms_per_step"] for ln in lines if ln.get("variant") == n and ln["N"] == N] for n in trainers}
        sp = [round(a / b, 3) for a, b in zip(ms["layer_graphed"], ms["fused"])]
        lines.append(dict(what="comparison", tree=args.tag, N=N, B=B, H=H, layer_ms=ms["layer_graphed"], fused_ms=ms["fused"],
                          speedup_per_pair=sp, fused_wins_every_pair=all(s > 1.0 for s in sp)))
        print(json.dumps(lines[-1]), flush=True)
        del trainers
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
