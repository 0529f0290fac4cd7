"""Time of PPO's rollout and evaluation on Pendulum-v1 under the Gaussian policy, both ways gymrl_amd.ppo_pendulum.PPOTrainer can run
them: tools/micro_rollout_classic.py's measurement (same clock, repeats and rounds) for the continuous env.

  * rollout — collect_rollout() with Config.persistent_rollout on (gymrl_rollout_pendulum: the whole rollout in one launch) and off
    (the step loop: gymrl_mlp_forward + gymrl_gaussian_sample + gymrl_env_step + the reward scale per vector step) at the
    (envs, hidden) pairs of `--shapes`, T = `--steps`.  A figure is the median of `--repeats` timed calls after one warm-up call;
    the two variants alternate inside each of `--rounds` rounds, and the step loop's own spread between rounds is reported beside
    the ratio.  Both variants are new code: the ratio is reported, not gated.
  * evaluation — evaluate(E) (gymrl_pendulum_ppo_eval: one launch) against _eval_loop(E) for E in `--episodes`.
Nets: freshly initialised (seed 5).  Needs an MI355X; appends one JSON line per measurement to profiles/rollout_pendulum_micro.jsonl.

    python tools/micro_rollout_pendulum.py [--shapes 64x64 4096x64 4096x256] [--steps 200] [--episodes 10 4096] [--repeats 3] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64x64", "4096x64", "4096x256"], help="envs x hidden")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--episodes", type=int, nargs="+", default=[10, 4096])
    ap.add_argument("--eval-hidden", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_pendulum_micro.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from gymrl_amd import _lib, ops
    from gymrl_amd.ppo_pendulum import Config, PPOTrainer
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_rollout_pendulum.py measures on an MI355X: none found")
    sha = _lib.lib_sha256()[:16]

    def emit(line):
        line["lib_sha256"] = sha
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    def timed(call):
        s = []
        for rep in range(args.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = call()
            torch.cuda.synchronize()
            if rep:
                s.append(time.perf_counter() - t0)
        return statistics.median(s), out

    def rounds(variants):
        med, last = {k: [] for k in variants}, {}
        for _ in range(args.rounds):
            for name, call in variants.items():
                m, last[name] = timed(call)
                med[name].append(m)
        return med, last

    def trainer(hidden, N, T, persistent):
        cfg = Config()
        cfg.hidden_dim, cfg.seed, cfg.num_envs, cfg.update_freq, cfg.persistent_rollout = hidden, 5, N, T, persistent
        return PPOTrainer(cfg)

    spread = lambda v: (max(v) - min(v)) / min(v)      # noqa: E731
    T = args.steps
    for shape in args.shapes:
        N, hidden = (int(x) for x in shape.split("x"))
        one, loop = trainer(hidden, N, T, True), trainer(hidden, N, T, False)
        assert one._persistent_ok() and not loop._persistent_ok()
        med, _ = rounds({"one_launch": one.collect_rollout, "step_loop": loop.collect_rollout})
        assert torch.equal(one.buffer.states, loop.buffer.states) and torch.equal(one.buffer.actions, loop.buffer.actions)
        mid = {k: statistics.median(v) for k, v in med.items()}
        emit({"what": "collect_rollout", "env": "Pendulum-v1", "hidden": hidden, "envs": N, "steps": T, "workgroups": (N + 15) // 16,
              "one_launch_us_per_vector_step": [round(m * 1e6 / T, 3) for m in med["one_launch"]],
              "step_loop_us_per_vector_step": [round(m * 1e6 / T, 3) for m in med["step_loop"]],
              "one_launch_round_spread": round(spread(med["one_launch"]), 4), "step_loop_round_spread": round(spread(med["step_loop"]), 4),
              "step_loop_over_one_launch": round(mid["step_loop"] / mid["one_launch"], 3), "repeats": args.repeats, "rounds": args.rounds,
              "timer": "host clock around collect_rollout(), ending in a device synchronise; median of the rounds' medians"})

    tr = trainer(args.eval_hidden, 16, 8, True)
    for E in args.episodes:
        med, last = rounds({"one_launch": lambda: tr.evaluate(E), "step_loop": lambda: tr._eval_loop(E)})
        ret, length, _ = last["one_launch"]
        mid = {k: statistics.median(v) for k, v in med.items()}
        emit({"what": "evaluate", "entry": "gymrl_pendulum_ppo_eval", "env": "Pendulum-v1", "hidden": args.eval_hidden, "episodes": E,
              "workgroups": (E + 15) // 16, "longest_episode": int(length.max()),
              "same_list": last["step_loop"] == ret[0].astype(np.float32).tolist(),
              "one_launch_ms": [round(m * 1e3, 4) for m in med["one_launch"]], "step_loop_ms": [round(m * 1e3, 3) for m in med["step_loop"]],
              "one_launch_round_spread": round(spread(med["one_launch"]), 4), "step_loop_round_spread": round(spread(med["step_loop"]), 4),
              "step_loop_over_one_launch": round(mid["step_loop"] / mid["one_launch"], 2), "repeats": args.repeats, "rounds": args.rounds,
              "timer": "host clock around evaluate() / _eval_loop(), each ending in a device read-back; median of the rounds' medians"})


if __name__ == "__main__":
    main()
