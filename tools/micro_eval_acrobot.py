"""Time of a policy evaluation on Acrobot-v1, both ways the trainers can run it (tools/micro_eval_mountaincar.py for env kind 5).

  * one gymrl_acrobot_net_eval launch (csrc/eval_net.hip): device events around `--batch` back-to-back launches of the
    same shape after a warm-up batch, per-launch median and minimum over `--repeats` such batches (tools/micro_eval_classic.py's
    method).  Shapes: 1 policy x 10 episodes at hidden 64 and 256; 1 policy x 4096 and 8 policies x 4096 episodes at hidden 256;
    with and without the forward image of fc2 where P = 1;
  * the same episodes through the same trainer's step loop — eval() with fused_eval = False: per step the network's layer
    launches, the pick, gymrl_env_step, a torch.where and a blocking read-back — for P = 1: host clock around eval(), which ends
    in a device synchronise.  The loop has no population form: P policies are P loops.
Nets: a freshly initialised DQN network (three layers, net 0) and a freshly initialised Rainbow network (dueling, net 2).  A
fresh network rarely swings the tip over the line, so the longest episode of a launch runs to the TimeLimit: 500 dependent steps,
each an RK4 step of the env on 16 lanes of one wave behind the network's forward.  us_per_dependent_step beside the same figure
of profiles/eval_acrobot_micro.jsonl prices that RK4 body.  The returns of the two ways are compared before a line is written.
Needs an MI355X; appends one JSON line per measurement to profiles/eval_acrobot_micro.jsonl.  The device clock is not read:
the lines carry none.

    python tools/micro_eval_acrobot.py [--repeats 3] [--batch 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SHAPES = ((64, 1, 10), (256, 1, 10), (256, 1, 4096), (256, 8, 4096))          # (hidden, policies, episodes)
ALGOS = (("dqn_cartpole", "DQNTrainer"), ("rainbow_dqn_cartpole", "RainbowDQNTrainer"))


def make_trainer(algo, cls, hidden):
    import importlib
    mod = importlib.import_module("gymrl_amd." + algo)
    cfg = mod.Config()
    cfg.env_name, cfg.hidden_dim, cfg.seed, cfg.memory_capacity = "Acrobot-v1", hidden, 5, 4096
    return getattr(mod, cls)(cfg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_acrobot_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_eval_acrobot.py measures on an MI355X: none found")
    sha = _lib.lib_sha256()[:16]
    lines = []

    def emit(line):
        line["lib_sha256"] = sha
        lines.append(line)
        print(json.dumps(line), flush=True)

    for algo, cls in ALGOS:
        trainers = {}
        for hidden, P, E in SHAPES:
            if hidden not in trainers:
                trainers[hidden] = make_trainer(algo, cls, hidden)
            tr = trainers[hidden]
            call = tr._eval_call()
            seed, id0 = tr.base_seed + tr.EVAL_SEED_OFFSET, tr.EVAL_ENV_ID0
            params = None if P == 1 else call["flat"].repeat(P, 1)
            images = [None] + ([ops.lin_fwd_image(call["trunk"][1][0])] if P == 1 and hidden % 16 == 0 else [])
            launch_returns = None
            for img in images:
                ms = []
                for rep in range(args.repeats + 1):                               # batch 0 warms the shape up
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    for _ in range(args.batch):
                        ret, length, term = ops.acrobot_net_eval(n_episodes=E, seed=seed, stream_id0=id0, params=params,
                                                                 images=img, **call)
                    stop.record()
                    torch.cuda.synchronize()
                    if rep:
                        ms.append(start.elapsed_time(stop) / args.batch)
                launch_returns = ret[0].tolist()
                med, longest, steps = statistics.median(ms), int(length.max().item()), int(length.sum().item())
                emit({"what": "acrobot_net_eval_one_launch", "algo": algo, "net": call["net"], "hidden": hidden, "policies": P,
                      "episodes": E, "fc2_image": img is not None, "workgroups": P * ((E + 15) // 16), "longest_episode": longest,
                      "env_steps": steps, "launch_ms_median": round(med, 4), "launch_ms_min": round(min(ms), 4),
                      "us_per_dependent_step": round(med * 1e3 / longest, 3), "repeats": args.repeats,
                      "launches_per_repeat": args.batch,
                      "timer": "device events around a batch of launches, outputs allocated inside", "device_clock": "not recorded"})
            if P != 1:
                continue
            s = []
            for rep in range(args.repeats + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loop_returns = tr.eval(E)                                         # fused_eval is False: the step loop
                torch.cuda.synchronize()
                if rep:
                    s.append(time.perf_counter() - t0)
            assert loop_returns == launch_returns, "the step loop is not the launch's episodes"
            med = statistics.median(s)
            emit({"what": "trainer_eval_step_loop", "algo": algo, "hidden": hidden, "policies": 1, "episodes": E,
                  "vector_steps": longest, "loop_ms_median": round(med * 1e3, 3), "loop_ms_min": round(min(s) * 1e3, 3),
                  "us_per_vector_step_median": round(med * 1e6 / longest, 2), "repeats": args.repeats,
                  "timer": "host clock around eval(), ending in a device synchronise", "device_clock": "not recorded"})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
