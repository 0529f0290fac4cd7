"""Run-steps per second of the tabular Q-learning population kernel (csrc/tabular.hip) at the reference's default configs.

For FrozenLake-v1 and CliffWalking-v0 at R = 64, 4096 and 65536 runs: the whole run (500 episodes) as ONE launch, timed with
device events after a warm-up launch of the same shape, median and minimum of `--repeats` launches; run-steps = the training
actions the launch took, summed over the runs (the kernel's own k).  Next to each figure: the CPU time of the Python test
reference (tests/tabular_ref.py) for ONE run of the same config — a reading of what the float64 loop costs on a host, not a
tuned baseline.  Needs an MI355X; appends one JSON line per (env, R) to profiles/qlearn_micro.jsonl.
The file's `default_config_greedy_eval` lines come from tests/test_qlearn_gpu.py::test_default_config_end_to_end, which appends
them only when the environment variable GYMRL_QLEARN_RECORD=1 is set (a plain suite run records nothing).

    python tools/micro_qlearn.py [--runs 64 4096 65536] [--repeats 5] [--out profiles/qlearn_micro.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, nargs="+", default=[64, 4096, 65536])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qlearn_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops, qlearning_cliffwalking, qlearning_frozenlake
    import tabular_ref as ref
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_qlearn.py measures on an MI355X: none found")
    dev = torch.device("cuda:0")
    lines = []
    for name, mod, kind in (("FrozenLake-v1", qlearning_frozenlake, ops.FROZENLAKE), ("CliffWalking-v0", qlearning_cliffwalking, ops.CLIFFWALKING)):
        cfg = mod.Config()
        flags = dict(is_slippery=getattr(cfg, "is_slippery", False), shaped=getattr(cfg, "use_reward_shaping", False))
        rcfg = {k: getattr(cfg, k) for k in ("seed", "max_episodes", "max_steps", "lr", "gamma", "epsilon_start", "epsilon_end", "epsilon_decay")}
        env = ref.FrozenLake(flags["is_slippery"], flags["shaped"]) if kind == ops.FROZENLAKE else ref.CliffWalking()
        t0 = time.perf_counter()
        one = ref.train_run(env, rcfg, 0)
        cpu_s = time.perf_counter() - t0
        total = cfg.max_episodes * cfg.max_steps
        tr = mod.QLearningTrainer(cfg)
        eps = torch.tensor([tr._epsilon_at(k) for k in range(1, total + 1)], dtype=torch.float64).to(dev)
        for R in args.runs:
            Q = torch.zeros(R, tr.n_states, 4, dtype=torch.float64, device=dev)
            state = torch.zeros(ops.qlearn_state_bytes(R), dtype=torch.uint8, device=dev)
            rew = torch.zeros(R, cfg.max_episodes, dtype=torch.float64, device=dev)
            length = torch.zeros(R, cfg.max_episodes, dtype=torch.int32, device=dev)
            k_dev = torch.zeros(R, dtype=torch.int32, device=dev)
            done = torch.zeros(R, dtype=torch.int32, device=dev)
            ms = []
            for rep in range(args.repeats + 1):                   # launch 0 warms the shape up
                Q.zero_()
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                ops.qlearn_train(kind, Q, state, eps, cfg.seed, 0, cfg.max_episodes, cfg.max_steps, total, cfg.lr, cfg.gamma, rew, length,
                                 k_dev, done, restart=True, **flags)
                stop.record()
                torch.cuda.synchronize()
                if rep:
                    ms.append(start.elapsed_time(stop))
            assert int(done.min().item()) == cfg.max_episodes
            steps = int(k_dev.sum(dtype=torch.int64).item())
            assert int(k_dev[0].item()) == one["k"], "run 0 is not the reference's run"
            med, best = statistics.median(ms), min(ms)
            lines.append({"what": "qlearn_train_whole_run_one_launch", "env": name, "runs": R, "run_steps": steps,
                          "longest_run_steps": int(k_dev.max().item()), "launch_ms_median": round(med, 4), "launch_ms_min": round(best, 4),
                          "run_steps_per_s_median": round(steps / (med * 1e-3), 1), "repeats": args.repeats,
                          "cpu_reference_one_run_s": round(cpu_s, 4), "cpu_reference_run_steps_per_s": round(one["k"] / cpu_s, 1),
                          "timer": "device events around one launch", "lib_sha256": _lib.lib_sha256()[:16]})
            print(json.dumps(lines[-1]), flush=True)
            del Q, rew, length
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
