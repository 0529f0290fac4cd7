"""Launch time of the tabular TD population kernels (csrc/tabular.hip: gymrl_tabular_train) at the scripts' default configs.

For FrozenLake-v1 and CliffWalking-v0, each rule (Q-learning through the new entry point, SARSA, Expected SARSA, Double
Q-learning) and R = 64, 4096, 65536 runs: the whole run (500 episodes) as ONE launch, timed with device events after a warm-up
launch of the same shape; median, minimum and maximum of `--repeats` launches.  run-steps = the env steps the launch took,
summed over the runs (the episode lengths; SARSA's k also counts the dropped draws).  Beside every shape, in the same process
and alternating with the rules launch by launch: gymrl_qlearn_train, the kernel the rules are set against (tools/micro_qlearn.py
times that entry point alone, at the same shapes).  Needs an MI355X; appends one JSON line per (env, rule, R) to
profiles/tabular_td_micro.jsonl.

    python tools/micro_tabular_td.py [--runs 64 4096 65536] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, nargs="+", default=[64, 4096, 65536])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tabular_td_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops, qlearning_cliffwalking, qlearning_frozenlake
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_tabular_td.py measures on an MI355X: none found")
    dev = torch.device("cuda:0")
    rules = dict(ops.TABULAR_RULES)
    lines = []
    for name, mod, kind in (("FrozenLake-v1", qlearning_frozenlake, ops.FROZENLAKE), ("CliffWalking-v0", qlearning_cliffwalking, ops.CLIFFWALKING)):
        cfg = mod.Config()
        flags = dict(is_slippery=getattr(cfg, "is_slippery", False), shaped=getattr(cfg, "use_reward_shaping", False))
        tr = mod.QLearningTrainer(cfg)
        E, T = cfg.max_episodes, cfg.max_steps
        eps = torch.tensor([tr._epsilon_at(k) for k in range(1, E * (T + 1) + 1)], dtype=torch.float64).to(dev)
        for R in args.runs:
            Q, Q2 = (torch.zeros(R, tr.n_states, 4, dtype=torch.float64, device=dev) for _ in range(2))
            state = torch.zeros(ops.tabular_state_bytes(0, R), dtype=torch.uint8, device=dev)
            rew = torch.zeros(R, E, dtype=torch.float64, device=dev)
            length = torch.zeros(R, E, dtype=torch.int32, device=dev)
            k_dev = torch.zeros(R, dtype=torch.int32, device=dev)
            done = torch.zeros(R, dtype=torch.int32, device=dev)

            def launch(rule):
                Q.zero_()
                Q2.zero_()
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                if rule is None:
                    ops.qlearn_train(kind, Q, state, eps[:E * T], cfg.seed, 0, E, T, E * T, cfg.lr, cfg.gamma, rew, length, k_dev, done,
                                     restart=True, **flags)
                else:
                    n = ops.tabular_draws(rule, E, T)
                    ops.tabular_train(rule, kind, Q, state, eps[:n], cfg.seed, 0, E, T, n, cfg.lr, cfg.gamma, rew, length, k_dev, done,
                                      Q2=Q2 if rule == ops.TABULAR_RULES["double_q"] else None, restart=True, **flags)
                stop.record()
                torch.cuda.synchronize()
                assert int(done.min().item()) == E
                return start.elapsed_time(stop), int(length.sum(dtype=torch.int64).item()), int(k_dev.max().item())

            what = [("gymrl_qlearn_train", None)] + [(f"gymrl_tabular_train:{n}", r) for n, r in rules.items()]
            ms, steps, longest = {w: [] for w, _ in what}, {}, {}
            for rep in range(args.repeats + 1):                   # round 0 warms every shape up; the entries alternate within a round
                for w, rule in what:
                    t, steps[w], longest[w] = launch(rule)
                    if rep:
                        ms[w].append(t)
            for w, _ in what:
                med = statistics.median(ms[w])
                lines.append({"what": w, "env": name, "runs": R, "run_steps": steps[w], "longest_run_draws": longest[w],
                              "launch_ms_median": round(med, 4), "launch_ms_min": round(min(ms[w]), 4), "launch_ms_max": round(max(ms[w]), 4),
                              "ns_per_run_step_median": round(med * 1e6 / steps[w], 4), "repeats": args.repeats,
                              "timer": "device events around one launch, entries alternating", "lib_sha256": _lib.lib_sha256()[:16]})
                print(json.dumps(lines[-1]), flush=True)
            del Q, Q2, rew, length
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
