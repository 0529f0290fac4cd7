"""Time of the learner's stages of one generation under separable NES and under OpenAI-ES (gymrl_amd/es.py, csrc/es.hip), in
one process on the same machine.

For (population, hidden) in (64, 64), (256, 64), (4096, 64), (256, 256), (4096, 256) — DESIGN §4u's shapes — on CartPole-v1's
policy, E = 1 episode per policy (the returns of one evaluation launch, taken once):

  * snes_ask / snes_tell      SeparableNES.ask(): gymrl_snes_perturb; .tell(): gymrl_snes_tell (one launch up to 256 policies,
                              two above) — no optimiser launch;
  * openai_ask / openai_tell  OpenAIES.ask(): gymrl_es_perturb; .tell(): gymrl_es_shape_grad (one launch / two) + gymrl_adam_step;
  * snes_both / openai_both   ask() then tell() back to back, as a generation issues them around the evaluation.

tools/micro_es.py's method: device events around a batch of back-to-back calls after a warm-up batch, per-call median and
minimum over `--repeats` batches, the two learners alternating inside a repeat so both see the same machine state.  A batch is
200 calls at the small shapes and 20 at the large ones.  The expectation to record for or against: SNES draws the same number of
normals and issues one launch fewer, so its ask + tell should not exceed OpenAI-ES's.  Needs an MI355X; appends one JSON line
per shape to profiles/snes_micro.jsonl and names the shapes where SNES lost; it exits 0 either way.

    python tools/micro_snes.py [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SHAPES = ((64, 64), (256, 64), (4096, 64), (256, 256), (4096, 256))


def timed(torch, fn, batch):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(batch):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / batch            # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snes_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops
    from gymrl_amd.es_cartpole import Config, ESTrainer
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_snes.py measures on an MI355X: none found")
    sha = _lib.lib_sha256()[:16]
    lines = []
    for P, hidden in SHAPES:
        learners = {}
        for method in ("snes", "openai"):
            cfg = Config()
            cfg.seed, cfg.population, cfg.hidden_dim, cfg.episodes_per_policy, cfg.log_freq, cfg.method = 3, P, hidden, 1, 0, method
            learners[method] = ESTrainer(cfg)
        tr = learners["openai"]
        n = tr.flat_params.numel()
        tr.es.ask()
        returns = tr._eval_launch(tr._call, n_episodes=1, seed=tr.base_seed + tr.EVAL_SEED_OFFSET, stream_id0=tr.TRAIN_ENV_ID0,
                                  params=tr.es.stack)[0]
        fns = {}
        for method, t in learners.items():
            es = t.es

            def both(es=es):
                es.ask()
                es.tell(returns)
            fns[method + "_ask"], fns[method + "_tell"], fns[method + "_both"] = es.ask, (lambda es=es: es.tell(returns)), both
        order = ["snes_ask", "openai_ask", "snes_tell", "openai_tell", "snes_both", "openai_both"]
        batch = 200 if P * n < (1 << 22) else 20
        us = {k: [] for k in order}
        for rep in range(args.repeats + 1):                      # repeat 0 warms every call of the shape up
            for name in order:
                t = timed(torch, fns[name], batch)
                if rep:
                    us[name].append(t)
        med = {k: statistics.median(v) for k, v in us.items()}
        line = {"what": "snes_vs_openai_es_stages", "population": P, "hidden": hidden, "n_params": n, "episodes_per_policy": 1,
                "pair_chunk": ops.ES_PAIR_CHUNK, "snes_tell_launches": 1 if P <= 256 else 2,
                "openai_tell_launches": 2 if P <= 256 else 3, "normals_per_stage": P // 2 * n}
        for k in order:
            line[k + "_us_median"], line[k + "_us_min"] = round(med[k], 2), round(min(us[k]), 2)
        line.update({"snes_over_openai_both": round(med["snes_both"] / med["openai_both"], 3),
                     "snes_over_openai_tell": round(med["snes_tell"] / med["openai_tell"], 3),
                     "repeats": args.repeats, "calls_per_repeat": batch,
                     "timer": "device events around a batch of back-to-back calls, the two learners alternating per repeat",
                     "lib_sha256": sha})
        lines.append(line)
        print(json.dumps(line), flush=True)
        del learners, fns, tr
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    lost = [(ln["population"], ln["hidden"]) for ln in lines if ln["snes_over_openai_both"] > 1.0]
    print(f"SNES ask + tell exceeds OpenAI-ES's at {lost}" if lost else "SNES ask + tell does not exceed OpenAI-ES's at any shape")


if __name__ == "__main__":
    main()
