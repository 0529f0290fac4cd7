"""Time per vector step of dqn_cartpole.DQNTrainer.train(): the fused step (Config.fused_step, csrc/dqn_step.hip, sixteen steps per
hipGraph replay where the loop can chunk) against the layer-by-layer path with its update replayed as a hipGraph
(use_graphs = True), on one library; optionally discrete SAC's fused step at the same shape as the yardstick.

    python tools/micro_dqn_fused.py --out profiles/dqn_fused_micro.jsonl            # every shape, both paths, dSAC's fused step
    python tools/micro_dqn_fused.py --variants layer --tag parent --out ...         # the layer path alone (a tree without the fused step)

Method: one trainer per variant; a warm-up train() call fills the ring, loads the code objects and captures the graphs; then
`--runs` timed train(max_vector_steps=steps) calls, each a host clock around work that ends in a device synchronise; the figure
is the MEDIAN run.  The variants of a shape alternate inside each of `--pairs` rounds, so that a drift of the machine falls on
all of them.  DQN solves CartPole within the timed window, and train() would return where mean(last 100) >= 495: the
tool gives each DQN trainer an episode_rewards deque of 99 entries, which the stop rule (it asks for 100) never accepts; every line
carries its count of optimiser steps, which must equal the steps asked for.  A run with no GPU fails: there is no CPU figure.  Lines are appended to --out as JSON.
--env_name MountainCar-v0 | Acrobot-v1 times the same loops on those envs (the fused act launch is gymrl_dqn_act_step_classic /
gymrl_dsac_act_step_classic there); every line then carries "env".  The default, CartPole-v1, prints the lines it always printed."""
import argparse
import collections
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(8192, 64, 256, 2048), (1, 64, 256, 4096), (64, 64, 256, 4096)]      # (N, B, hidden, timed steps): the flagship width, the reference's N, a small vector
DEFAULT_ENV = "CartPole-v1"
ENV = DEFAULT_ENV              # --env_name


def _dqn(N, B, H, fused):
    from gymrl_amd import dqn_cartpole
    cfg = dqn_cartpole.Config()
    cfg.env_name = ENV
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed = N, B, H, 0
    cfg.max_episodes, cfg.use_graphs, cfg.fused_step = 10 ** 9, True, fused
    cfg.memory_capacity = max(cfg.memory_capacity, 4 * N)
    tr = dqn_cartpole.DQNTrainer(cfg)
    assert bool(getattr(tr, "_fused_ok", lambda: False)()) == fused
    return tr, (lambda: tr.optimizer.step_count)


def _dsac(N, B, H, fused):
    from gymrl_amd import sac_cartpole
    cfg = sac_cartpole.Config()
    cfg.env_name = ENV
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed = N, B, H, 0
    cfg.max_episodes, cfg.use_graphs, cfg.fused_step = 10 ** 9, True, fused
    cfg.memory_capacity = max(cfg.memory_capacity, 4 * N)
    tr = sac_cartpole.SACTrainer(cfg)
    assert tr._fused_ok() == fused
    return tr, (lambda: tr.critic1_optim.step_count)


VARIANTS = {"layer": ("dqn_layer_graphed", lambda N, B, H: _dqn(N, B, H, False)),
            "fused": ("dqn_fused", lambda N, B, H: _dqn(N, B, H, True)),
            "dsac": ("dsac_fused", lambda N, B, H: _dsac(N, B, H, True))}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="layer,fused,dsac")
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
    if not torch.cuda.is_available():
        raise SystemExit("micro_dqn_fused: needs an MI355X; there is no CPU figure")
    box = f"1x {torch.cuda.get_device_name(0)}, torch {torch.__version__}"
    lines = []
    for N, B, H, steps in SHAPES:
        trainers = {}
        for v in args.variants.split(","):
            name, make = VARIANTS[v]
            tr, count = make(N, B, H)
            tr.train(max_vector_steps=max(args.warmup, (B + N - 1) // N + 32))     # fills the ring, captures the graphs
            torch.cuda.synchronize()
            if v != "dsac":            # (discrete SAC's train() has no stop rule)
                tr.episode_rewards = collections.deque(maxlen=99)      # DQN's asks for 100 entries: every timed call runs all its steps
            trainers[name] = (tr, count)
        for pair in range(args.pairs):
            for name, (tr, count) in trainers.items():
                runs, before = [], count()
                for _ in range(args.runs):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tr.train(max_vector_steps=steps)
                    torch.cuda.synchronize()
                    runs.append((time.perf_counter() - t0) * 1e3 / steps)
                assert count() - before == args.runs * steps, (name, count() - before)      # no call returned early
                chunk = getattr(tr, "_chunk", None)
                lines.append(dict(what="vector_step", variant=name, tree=args.tag, N=N, B=B, H=H, steps=steps,
                                  ms_per_step=round(statistics.median(runs), 4), ms_per_step_runs=[round(r, 4) for r in runs],
                                  chunk_graph=bool(chunk is not None and chunk.graph is not None),
                                  updates=count() - before, box=box, pair=pair, **env_key))
                print(json.dumps(lines[-1]), flush=True)
        if "dqn_layer_graphed" in trainers and "dqn_fused" in trainers:
            ms = {n: [ln["ms_per_step"] for ln in lines if ln.get("variant") == n and ln["N"] == N] for n in trainers}
            sp = [round(a / b, 3) for a, b in zip(ms["dqn_layer_graphed"], ms["dqn_fused"])]
            lines.append(dict(what="comparison", tree=args.tag, N=N, B=B, H=H, layer_ms=ms["dqn_layer_graphed"], fused_ms=ms["dqn_fused"],
                              dsac_fused_ms=ms.get("dsac_fused"), speedup_per_pair=sp, fused_wins_every_pair=all(s > 1.0 for s in sp), **env_key))
            print(json.dumps(lines[-1]), flush=True)
        del trainers
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
