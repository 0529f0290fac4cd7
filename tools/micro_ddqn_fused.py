"""Time per vector step of train() for ddqn_per_cartpole.DDQNPERTrainer and ddqn_per_duel_cartpole.DDQNPERDuelTrainer: the fused
step (Config.fused_step, csrc/ddqn_step.hip, sixteen steps per hipGraph replay where the loop can chunk) against the
layer-by-layer path with its update replayed as a hipGraph (use_graphs = True), on one library, with DQN's fused step
(csrc/dqn_step.hip) at the same shape as the yardstick.

    python tools/micro_ddqn_fused.py --out profiles/ddqn_fused_micro.jsonl

Method: tools/micro_dqn_fused.py's.  One trainer per variant; a warm-up train() call fills the ring, loads the code objects and
captures the graphs; then `--runs` timed train(max_vector_steps=steps) calls, each a host clock around work that ends in a
device synchronise; the figure is the MEDIAN run.  The variants of a shape alternate inside each of `--pairs` rounds, so that a
drift of the machine falls on all of them.  Each trainer gets an episode_rewards deque of 99 entries, which the stop rule (it
asks for 100) never accepts; every line carries its count of optimiser steps, which must equal the steps asked for.  A run
with no GPU fails: there is no CPU figure.  Lines are appended to --out as JSON.
--env_name MountainCar-v0 | Acrobot-v1 times the same loops on those envs (the fused act launch is gymrl_dqn_act_step_classic /
gymrl_dsac_act_step_classic there); every line then carries "env".  The default, CartPole-v1, prints the lines it always printed.
The dueling variants are two-action kernels: they are left out on those envs."""
import argparse
import collections
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(8192, 64, 256, 1024), (64, 64, 256, 2048), (1, 64, 256, 2048)]      # (N, B, hidden, timed steps)
DEFAULT_ENV = "CartPole-v1"
ENV = DEFAULT_ENV              # --env_name


def _make(module, trainer, N, B, H, fused):
    import importlib
    mod = importlib.import_module("gymrl_amd." + module)
    cfg = mod.Config()
    cfg.env_name = ENV
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed = N, B, H, 0
    cfg.max_episodes, cfg.use_graphs, cfg.fused_step = 10 ** 9, True, fused
    cfg.memory_capacity = max(cfg.memory_capacity, 4 * N)
    tr = getattr(mod, trainer)(cfg)
    assert tr._fused_ok() == fused
    return tr


VARIANTS = {"ddqn_layer_graphed": ("ddqn_per_cartpole", "DDQNPERTrainer", False),
            "ddqn_fused": ("ddqn_per_cartpole", "DDQNPERTrainer", True),
            "duel_layer_graphed": ("ddqn_per_duel_cartpole", "DDQNPERDuelTrainer", False),
            "duel_fused": ("ddqn_per_duel_cartpole", "DDQNPERDuelTrainer", True),
            "dqn_fused": ("dqn_cartpole", "DQNTrainer", True)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=48)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--out", default=None)
    ap.add_argument("--env_name", default=DEFAULT_ENV)
    args = ap.parse_args()
    global ENV
    ENV = args.env_name
    env_key = {} if ENV == DEFAULT_ENV else {"env": ENV}
    if args.variants is None:
        args.variants = ",".join(v for v in VARIANTS if ENV == DEFAULT_ENV or not v.startswith("duel_"))
    if not torch.cuda.is_available():
        raise SystemExit("micro_ddqn_fused: needs an MI355X; there is no CPU figure")
    box = f"1x {torch.cuda.get_device_name(0)}, torch {torch.__version__}"
    lines = []
    for N, B, H, steps in SHAPES:
        trainers = {}
        for name in args.variants.split(","):
            tr = _make(*VARIANTS[name][:2], N, B, H, VARIANTS[name][2])
            tr.train(max_vector_steps=max(args.warmup, (B + N - 1) // N + 32))     # fills the ring, captures the graphs
            torch.cuda.synchronize()
            tr.episode_rewards = collections.deque(maxlen=99)      # the stop rule asks for 100 entries: every timed call runs all its steps
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
                chunk = getattr(tr, "_chunk", None)
                lines.append(dict(what="vector_step", variant=name, tree=args.tag, N=N, B=B, H=H, steps=steps,
                                  ms_per_step=round(statistics.median(runs), 4), ms_per_step_runs=[round(r, 4) for r in runs],
                                  chunk_graph=bool(chunk is not None and chunk.graph is not None), updates=done, box=box, pair=pair, **env_key))
                print(json.dumps(lines[-1]), flush=True)
        ms = {n: [ln["ms_per_step"] for ln in lines if ln.get("variant") == n and ln["N"] == N] for n in trainers}
        for net in ("ddqn", "duel"):
            if f"{net}_layer_graphed" in ms and f"{net}_fused" in ms:
                sp = [round(a / b, 3) for a, b in zip(ms[f"{net}_layer_graphed"], ms[f"{net}_fused"])]
                over = [round(a / b, 3) for a, b in zip(ms[f"{net}_fused"], ms.get("dqn_fused", []))]
                lines.append(dict(what="comparison", net=net, tree=args.tag, N=N, B=B, H=H, layer_ms=ms[f"{net}_layer_graphed"],
                                  fused_ms=ms[f"{net}_fused"], dqn_fused_ms=ms.get("dqn_fused"), speedup_per_pair=sp,
                                  fused_over_dqn_fused=over, fused_wins_every_pair=all(s > 1.0 for s in sp), **env_key))
                print(json.dumps(lines[-1]), flush=True)
        del trainers
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
