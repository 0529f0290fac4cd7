"""Micro-benchmark of the TD3 / DDPG Pendulum vector step (one MI355X): milliseconds per vector step at N = 4096, B = 128,
H = 256 (BASELINE config 4's sizes) on
  td3_layer         TD3 on the layer-by-layer path (fused_step off: one gymrl_lin_* launch per layer and direction, eager update)
  ddpg_layer        DDPG on the layer-by-layer path with its graphed update (GraphedUpdate)
  td3_fused_eager   TD3 on gymrl_td3_act_step + gymrl_td3_update, launched eagerly (use_graphs off)
  td3_fused_chunk   ... sixteen vector steps replayed as one hipGraph (graphs.StepChunk)
  ddpg_fused_chunk  DDPG likewise
The layer path and the fused path run ALTERNATELY, --pairs times, every measurement in a child process of its own under its
own time limit; the parent never opens the GPU and stops at the first child that fails.  One JSON line per measurement plus one
summary line per comparison (fused / layer per pair, and the spread between pairs) -> profiles/td3_fused_micro.jsonl."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"td3_layer": ("td3", False, True), "ddpg_layer": ("ddpg", False, True), "td3_fused_eager": ("td3", True, False),
            "td3_fused_chunk": ("td3", True, True), "ddpg_fused_chunk": ("ddpg", True, True)}


def child(variant, steps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    from gymrl_amd import ddpg_pendulum, td3_pendulum
    algo, fused, graphs = VARIANTS[variant]
    mod, cls = (td3_pendulum, "TD3Trainer") if algo == "td3" else (ddpg_pendulum, "DDPGTrainer")
    cfg = mod.Config()
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed = 4096, 128, 256, 0
    cfg.max_episodes, cfg.memory_capacity, cfg.use_graphs, cfg.fused_step = 10 ** 9, 1 << 20, graphs, fused
    tr = getattr(mod, cls)(cfg)
    assert tr._fused_ok() == fused
    tr.train(max_vector_steps=warmup)
    torch.cuda.synchronize()
    per = []
    for _ in range(3):
        t0 = time.perf_counter()
        tr.train(max_vector_steps=steps)
        torch.cuda.synchronize()
        per.append(1000 * (time.perf_counter() - t0) / steps)
    assert all(torch.isfinite(getattr(tr, n)).all() for n in ("actor_flat", "critic_flat"))
    chunk = getattr(tr, "_chunk", None)
    print(json.dumps({"what": "vector_step", "variant": variant, "N": 4096, "B": 128, "H": 256, "steps": steps, "ms_per_step": round(min(per), 4),
                      "ms_per_step_runs": [round(p, 4) for p in per], "chunk_graph": bool(chunk is not None and chunk.graph is not None),
                      "updates": tr.critic_optimizer.step_count, "box": f"1x MI355X (gfx950), torch {torch.__version__}"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "td3_fused_micro.jsonl"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps, args.warmup)
    lines, got = [], {v: [] for v in VARIANTS}
    order = ["td3_layer", "td3_fused_chunk", "ddpg_layer", "ddpg_fused_chunk", "td3_fused_eager"]
    for pair in range(args.pairs):
        for v in order:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", v, "--steps", str(args.steps),
                   "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:                 # nothing more is started on the GPU after a failure
                print(f"{v} (pair {pair}) ended with status {r.returncode}: stopping", file=sys.stderr)
                return r.returncode
            rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            rec["pair"] = pair
            got[v].append(rec["ms_per_step"])
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    for base, new in (("td3_layer", "td3_fused_chunk"), ("ddpg_layer", "ddpg_fused_chunk"), ("td3_layer", "td3_fused_eager")):
        ratios = [b / n for b, n in zip(got[base], got[new])]
        rec = {"what": "comparison", "layer": base, "fused": new, "layer_ms": got[base], "fused_ms": got[new],
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
