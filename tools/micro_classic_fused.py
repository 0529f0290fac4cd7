"""Time per vector step of train() with Config.fused_step = True on MountainCar-v0 and Acrobot-v1 — DQN, DDQN + PER (non-dueling)
and discrete SAC — on this tree against ANOTHER tree with its own library (the parent commit's, where the same setting runs the
fused update behind a layer-by-layer act and never reaches a StepChunk replay), and against this tree's layer-by-layer path with
its graphed update.

    python tools/micro_classic_fused.py --parent_tree ../parent --out profiles/dqn_classic_fused_micro.jsonl

Method: the driver never opens the GPU.  A round is one child process per tree, the other tree's first, each under its own time
limit; a child builds one trainer per (algorithm, env, shape, variant), warms it up (fills the ring, loads the code objects,
captures the graphs), then takes the MEDIAN of --runs timed train(max_vector_steps = --steps) calls, each a host clock around work
that ends in a device synchronise, and checks that every call ran all its optimiser steps.  After --rounds rounds the driver
writes every line, and per (algorithm, env, shape) the median over the rounds of each variant, the other tree's own
(max - min) / median, and the ratios.  It stops at the first child that fails.  A run with no GPU fails: there is no CPU figure."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8192, 64, 256), (64, 64, 256), (64, 64, 64), (1, 64, 256)]          # (N, B, hidden)
ENVS = ("MountainCar-v0", "Acrobot-v1")
ALGOS = {"dqn": ("dqn_cartpole", "DQNTrainer"), "ddqn_per": ("ddqn_per_cartpole", "DDQNPERTrainer"), "dsac": ("sac_cartpole", "SACTrainer")}
VARIANTS = {"fused_step": True, "layer_graphed": False}                         # Config.fused_step


def child(tree, tag, variants, steps, warmup, runs):
    sys.path.insert(0, os.path.abspath(tree))
    import importlib
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("micro_classic_fused: needs an MI355X; there is no CPU figure")
    box = f"1x {torch.cuda.get_device_name(0)}, torch {torch.__version__}"
    for algo, (module, trainer) in ALGOS.items():
        mod = importlib.import_module("gymrl_amd." + module)
        assert os.path.abspath(mod.__file__).startswith(os.path.abspath(tree) + os.sep), mod.__file__
        for env_name in ENVS:
            for N, B, H in SHAPES:
                for variant in variants:
                    cfg = mod.Config()
                    cfg.env_name = env_name
                    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed = N, B, H, 0
                    cfg.max_episodes, cfg.use_graphs, cfg.fused_step = 10 ** 9, True, VARIANTS[variant]
                    cfg.memory_capacity = max(cfg.memory_capacity, 4 * N)
                    if algo == "dsac":
                        cfg.kernel_softmax = True
                    tr = getattr(mod, trainer)(cfg)
                    count = (lambda tr=tr: tr.critic1_optim.step_count) if algo == "dsac" else (lambda tr=tr: tr.optimizer.step_count)
                    tr.train(max_vector_steps=max(warmup, (B + N - 1) // N + 32))
                    torch.cuda.synchronize()
                    per, before = [], count()
                    for _ in range(runs):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        tr.train(max_vector_steps=steps)
                        torch.cuda.synchronize()
                        per.append((time.perf_counter() - t0) * 1e3 / steps)
                    assert count() - before == runs * steps, (algo, env_name, N, variant, count() - before)
                    chunk = getattr(tr, "_chunk", None)
                    print(json.dumps(dict(what="vector_step", tree=tag, algo=algo, env=env_name, N=N, B=B, H=H, variant=variant, steps=steps,
                                          ms_per_step=round(statistics.median(per), 4), ms_per_step_runs=[round(p, 4) for p in per],
                                          fused_update=bool(tr._fused_update_ok()), fused_act=bool(tr._fused_ok()),
                                          chunk_graph=bool(chunk is not None and chunk.graph is not None), box=box)), flush=True)
                    del tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent_tree", help="another checkout with its own built library")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=48)
    ap.add_argument("--limit", type=int, default=400, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_classic_fused_micro.jsonl"))
    ap.add_argument("--child", nargs=3, metavar=("TREE", "TAG", "VARIANTS"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.child[2].split(","), args.steps, args.warmup, args.runs)
    trees = ([(os.path.abspath(args.parent_tree), "parent", "fused_step")] if args.parent_tree else []) + [(ROOT, "this", "fused_step,layer_graphed")]
    lines = []
    for rnd in range(args.rounds):
        for tree, tag, variants in trees:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", tree, tag, variants,
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--runs", str(args.runs)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=tree)
            got = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
            for rec in got:
                rec["round"] = rnd
                print(json.dumps(rec), flush=True)
            lines += got
            if r.returncode != 0:                 # nothing more is started on the GPU after a failure
                print(f"{tag} (round {rnd}) ended with status {r.returncode}: stopping", file=sys.stderr)
                _write(args.out, lines)
                return r.returncode
    key = lambda ln: (ln["algo"], ln["env"], ln["N"], ln["B"], ln["H"])     # noqa: E731
    for k in sorted({key(ln) for ln in lines}, key=lambda k: (k[0], k[1], -k[2], -k[4])):
        ms = {}
        for ln in lines:
            if key(ln) == k:
                ms.setdefault((ln["tree"], ln["variant"]), []).append(ln["ms_per_step"])
        med = {tv: statistics.median(v) for tv, v in ms.items()}
        rec = dict(what="comparison", algo=k[0], env=k[1], N=k[2], B=k[3], H=k[4], this_fused_ms=ms[("this", "fused_step")],
                   this_layer_graphed_ms=ms[("this", "layer_graphed")], this_fused_median=med[("this", "fused_step")],
                   layer_over_fused=round(med[("this", "layer_graphed")] / med[("this", "fused_step")], 3))
        if ("parent", "fused_step") in ms:
            p = ms[("parent", "fused_step")]
            rec.update(parent_fused_step_ms=p, parent_median=med[("parent", "fused_step")],
                       parent_spread=round((max(p) - min(p)) / med[("parent", "fused_step")], 4),
                       parent_over_this=round(med[("parent", "fused_step")] / med[("this", "fused_step")], 3))
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    _write(args.out, lines)
    return 0


def _write(path, lines):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    sys.exit(main())
