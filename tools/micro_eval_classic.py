"""Time of a policy evaluation on CartPole-v1 / Pendulum-v1, both ways the trainers can run it.

  * one gymrl_classic_policy_eval launch (csrc/eval_classic.hip) for P = 1 and 8 policies x E = 10 and 4096 episodes: device events
    around `--batch` back-to-back launches of the same shape after a warm-up batch, per-launch median and minimum over
    `--repeats` such batches (tools/micro_mountaincar.py's method);
  * the same episodes through the trainer's step loop — eval() with fused_eval = False, which is what the trainers ran before the
    launch existed: per step three gymrl_lin_fwd launches, the pick, gymrl_env_step, a torch.where and a blocking read-back — for
    P = 1: host clock around eval(), which ends in a device synchronise.  The loop has no population form: P policies are P loops.
Nets: a DQN network that holds the pole to the TimeLimit (a linear controller through a ReLU pair, the rest of the H x H layer at
its initial values so that the layer is streamed whole) and a freshly initialised TD3 actor, hidden 64 and 256; with and without
the forward image of fc2 where P = 1.
Needs an MI355X; appends one JSON line per measurement to profiles/eval_classic_micro.jsonl.

    python tools/micro_eval_classic.py [--episodes 10 4096] [--policies 1 8] [--hidden 64 256] [--repeats 3] [--batch 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

CONTROLLER = (0.1, 0.3, 1.0, 0.5)          # push right iff k . obs > 0: holds every reset draw for 500 steps


def make_trainer(algo, hidden):
    import importlib
    import torch
    mod = importlib.import_module("gymrl_amd." + algo)
    cfg = mod.Config()
    cfg.hidden_dim, cfg.seed, cfg.memory_capacity = hidden, 5, 4096
    tr = getattr(mod, "DQNTrainer" if algo == "dqn_cartpole" else "TD3Trainer")(cfg)
    if algo == "dqn_cartpole":
        fc1, fc2, fc3 = tr._eval_policy()[0]
        with torch.no_grad():
            k = torch.tensor(CONTROLLER, device=tr.device)
            fc1.weight[0], fc1.weight[1] = k, -k
            fc1.bias[:2] = 0.0
            fc2.weight[:2] = 0.0
            fc2.weight[0, 0] = fc2.weight[1, 1] = 1.0
            fc2.bias[:2] = 0.0
            fc3.weight.zero_()
            fc3.bias.zero_()
            fc3.weight[0, 1] = fc3.weight[1, 0] = 1.0
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, nargs="+", default=[10, 4096])
    ap.add_argument("--policies", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--hidden", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_classic_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_eval_classic.py measures on an MI355X: none found")
    sha = _lib.lib_sha256()[:16]
    lines = []

    def emit(line):
        line["lib_sha256"] = sha
        lines.append(line)
        print(json.dumps(line), flush=True)

    for algo in ("dqn_cartpole", "td3_pendulum"):
        for hidden in args.hidden:
            tr = make_trainer(algo, hidden)
            call = tr._eval_call()
            seed, id0 = tr.base_seed + tr.EVAL_SEED_OFFSET, tr.EVAL_ENV_ID0
            flat = call["flat"]
            for E in args.episodes:
                launch_returns = None
                for P in args.policies:
                    params = None if P == 1 else flat.repeat(P, 1)
                    images = [None] + ([ops.lin_fwd_image(call["layers"][1].weight)] if P == 1 and hidden % 16 == 0 else [])
                    for img in images:
                        ms = []
                        for rep in range(args.repeats + 1):                       # batch 0 warms the shape up
                            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            start.record()
                            for _ in range(args.batch):
                                ret, length, term = ops.classic_policy_eval(n_episodes=E, seed=seed, stream_id0=id0, params=params,
                                                                            images=img, **call)
                            stop.record()
                            torch.cuda.synchronize()
                            if rep:
                                ms.append(start.elapsed_time(stop) / args.batch)
                        if P == 1:
                            launch_returns = ret[0].tolist()
                        med, longest, steps = statistics.median(ms), int(length.max().item()), int(length.sum().item())
                        emit({"what": "classic_policy_eval_one_launch", "algo": algo, "hidden": hidden, "policies": P, "episodes": E,
                              "fc2_image": img is not None, "workgroups": P * ((E + 15) // 16), "longest_episode": longest,
                              "env_steps": steps, "launch_ms_median": round(med, 4), "launch_ms_min": round(min(ms), 4),
                              "us_per_dependent_step": round(med * 1e3 / longest, 3), "repeats": args.repeats,
                              "launches_per_repeat": args.batch,
                              "timer": "device events around a batch of launches, outputs allocated inside"})
                s = []
                for rep in range(args.repeats + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    loop_returns = tr.eval(E)                                     # fused_eval is False: the step loop
                    torch.cuda.synchronize()
                    if rep:
                        s.append(time.perf_counter() - t0)
                assert loop_returns == launch_returns, "the step loop is not the launch's episodes"
                med = statistics.median(s)
                emit({"what": "trainer_eval_step_loop", "algo": algo, "hidden": hidden, "policies": 1, "episodes": E,
                      "vector_steps": longest, "loop_ms_median": round(med * 1e3, 3), "loop_ms_min": round(min(s) * 1e3, 3),
                      "us_per_vector_step_median": round(med * 1e6 / longest, 2), "repeats": args.repeats,
                      "timer": "host clock around eval(), ending in a device synchronise"})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
