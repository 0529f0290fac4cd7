"""Micro-benchmark of the discrete-SAC CartPole vector step (one MI355X): milliseconds per vector step at N = 4096, B = 128,
H = 256, a ring of 2^20 rows, on
  layer         the layer-by-layer path with its graphed update (fused_step off, kernel softmax on: the path the fused step
                reproduces bit for bit)
  fused_eager   gymrl_dsac_act_step + gymrl_dsac_update, launched eagerly (use_graphs off)
  fused_chunk   ... sixteen vector steps replayed as one hipGraph (graphs.StepChunk)
The three run ALTERNATELY, --pairs times, every measurement in a child process of its own under its own time limit; the parent
never opens the GPU and stops at the first child that fails.  A child reports the minimum of three timed runs of --steps
vector steps.  One JSON line per measurement plus one summary line per comparison -> profiles/dsac_fused_micro.jsonl.
--env_name MountainCar-v0 | Acrobot-v1 times the same loops on those envs (the fused act launch is gymrl_dqn_act_step_classic /
gymrl_dsac_act_step_classic there); every line then carries "env".  The default, CartPole-v1, prints the lines it always printed."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"layer": (False, True), "fused_eager": (True, False), "fused_chunk": (True, True)}      # (fused_step, use_graphs)


DEFAULT_ENV = "CartPole-v1"


def child(variant, steps, warmup, env_name=DEFAULT_ENV):
    import torch
    sys.path.insert(0, ROOT)
    from gymrl_amd import sac_cartpole
    fused, graphs = VARIANTS[variant]
    cfg = sac_cartpole.Config()
    cfg.env_name = env_name
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed = 4096, 128, 256, 0
    cfg.max_episodes, cfg.memory_capacity, cfg.use_graphs = 10 ** 9, 1 << 20, graphs
    cfg.fused_step, cfg.kernel_softmax = fused, True
    tr = sac_cartpole.SACTrainer(cfg)
    assert tr._fused_ok() == fused
    tr.train(max_vector_steps=warmup)
    torch.cuda.synchronize()
    per = []
    for _ in range(3):
        t0 = time.perf_counter()
        tr.train(max_vector_steps=steps)
        torch.cuda.synchronize()
        per.append(1000 * (time.perf_counter() - t0) / steps)
    assert all(torch.isfinite(getattr(tr, n)).all() for n in ("actor_flat", "c1_flat", "c2_flat", "log_alpha"))
    chunk = getattr(tr, "_chunk", None)
    print(json.dumps({"what": "vector_step", "variant": variant, "N": 4096, "B": 128, "H": 256, "steps": steps, "ms_per_step": round(min(per), 4),
                      "ms_per_step_runs": [round(p, 4) for p in per], "chunk_graph": bool(chunk is not None and chunk.graph is not None),
                      "updates": tr.critic1_optim.step_count, "box": f"1x MI355X (gfx950), torch {torch.__version__}",
                      **({} if env_name == DEFAULT_ENV else {"env": env_name})}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dsac_fused_micro.jsonl"))
    ap.add_argument("--env_name", default=DEFAULT_ENV)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps, args.warmup, args.env_name)
    lines, got = [], {v: [] for v in VARIANTS}
    for pair in range(args.pairs):
        for v in ("layer", "fused_chunk", "fused_eager"):
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", v, "--steps", str(args.steps),
                   "--warmup", str(args.warmup)] + ([] if args.env_name == DEFAULT_ENV else ["--env_name", args.env_name])
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:                 # nothing more is started on the GPU after a failure
                print(f"{v} (pair {pair}) ended with status {r.returncode}: stopping", file=sys.stderr)
                return r.returncode
            rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            rec["pair"] = pair
            got[v].append(rec["ms_per_step"])
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    for new in ("fused_chunk", "fused_eager"):
        ratios = [b / n for b, n in zip(got["layer"], got[new])]
        rec = {"what": "comparison", "layer": "layer", "fused": new, "layer_ms": got["layer"], "fused_ms": got[new],
               "speedup_per_pair": [round(x, 3) for x in ratios], "speedup_min": round(min(ratios), 3), "speedup_max": round(max(ratios), 3),
               "fused_wins_every_pair": all(x > 1.0 for x in ratios)}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(x) + "\n" for x in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
