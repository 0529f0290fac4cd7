"""Time of PPO's rollout and evaluation on MountainCar-v0, Acrobot-v1 (and, for the evaluation, CartPole-v1), both ways
gymrl_amd.ppo_lunarlander.PPOTrainer can run them.

  * rollout — collect_rollout() per vector step with Config.persistent_rollout on (gymrl_rollout_classic, csrc/rollout_classic.hip:
    the whole rollout in one launch) and off (the step loop: gymrl_mlp_forward + gymrl_categorical_sample + gymrl_env_step per vector
    step), at N x hidden of `--envs` x `--hidden`, T = `--steps`.  Host clock around a call that ends in a device synchronise; a
    figure is the median of `--repeats` timed calls after one warm-up call; the two variants alternate inside each of `--rounds`
    rounds, and the spread between a variant's rounds is reported beside the ratio it has to be read against.
  * evaluation — evaluate(E) (gymrl_classic_ppo_eval, csrc/eval_classic_ppo.hip: one launch) against _eval_loop(E) (the step loop
    eval() runs without Config.fused_eval) for E in `--episodes`, the same clock and rounds.  Per-step figures divide by the longest
    episode, the number of dependent steps a launch or a loop has to take.
Nets: freshly initialised (seed 5).  Needs an MI355X; appends one JSON line per measurement to profiles/rollout_classic_micro.jsonl
and profiles/classic_ppo_eval_micro.jsonl.

    python tools/micro_rollout_classic.py [--envs 64 4096] [--hidden 64 256] [--steps 256] [--episodes 10 4096] [--repeats 3] [--rounds 2]
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
    ap.add_argument("--envs", type=int, nargs="+", default=[64, 4096])
    ap.add_argument("--hidden", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--episodes", type=int, nargs="+", default=[10, 4096])
    ap.add_argument("--eval-hidden", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-rollout", action="store_true")
    ap.add_argument("--no-eval", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_classic_micro.jsonl"))
    ap.add_argument("--eval-out", default=os.path.join(ROOT, "profiles", "classic_ppo_eval_micro.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from gymrl_amd import _lib, ops
    from gymrl_amd.ppo_lunarlander import Config, PPOTrainer
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_rollout_classic.py measures on an MI355X: none found")
    sha = _lib.lib_sha256()[:16]

    def emit(path, line):
        line["lib_sha256"] = sha
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")

    def timed(call):
        """-> (median seconds of `--repeats` calls after one warm-up call, the last call's result)."""
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
        """name -> call: every variant once per round, in turn -> name -> [median per round], name -> last result."""
        med, last = {k: [] for k in variants}, {}
        for _ in range(args.rounds):
            for name, call in variants.items():
                m, last[name] = timed(call)
                med[name].append(m)
        return med, last

    def trainer(env_name, hidden, N, T, persistent):
        cfg = Config()
        cfg.env_name, cfg.hidden_dim, cfg.seed, cfg.num_envs, cfg.update_freq = env_name, hidden, 5, N, T
        cfg.persistent_rollout = persistent
        return PPOTrainer(cfg)

    spread = lambda v: (max(v) - min(v)) / min(v)      # noqa: E731

    if not args.no_rollout:
        for env_name in ("MountainCar-v0", "Acrobot-v1"):
            for hidden in args.hidden:
                for N in args.envs:
                    T = args.steps
                    one, loop = trainer(env_name, hidden, N, T, True), trainer(env_name, hidden, N, T, False)
                    assert one._persistent_ok() and not loop._persistent_ok()
                    med, _ = rounds({"one_launch": one.collect_rollout, "step_loop": loop.collect_rollout})
                    assert torch.equal(one.buffer.states, loop.buffer.states) and torch.equal(one.buffer.log_probs, loop.buffer.log_probs)
                    best = {k: min(v) for k, v in med.items()}
                    emit(args.out, {"what": "collect_rollout", "env": env_name, "hidden": hidden, "envs": N, "steps": T,
                                    "workgroups": (N + 15) // 16,
                                    "one_launch_us_per_vector_step": [round(m * 1e6 / T, 3) for m in med["one_launch"]],
                                    "step_loop_us_per_vector_step": [round(m * 1e6 / T, 3) for m in med["step_loop"]],
                                    "one_launch_round_spread": round(spread(med["one_launch"]), 4),
                                    "step_loop_round_spread": round(spread(med["step_loop"]), 4),
                                    "step_loop_over_one_launch": round(best["step_loop"] / best["one_launch"], 3),
                                    "slowest_one_launch_beats_fastest_step_loop": max(med["one_launch"]) < min(med["step_loop"]),
                                    "repeats": args.repeats, "rounds": args.rounds,
                                    "timer": "host clock around collect_rollout(), ending in a device synchronise; median per round"})

    if not args.no_eval:
        for env_name in ("CartPole-v1", "MountainCar-v0", "Acrobot-v1"):
            tr = trainer(env_name, args.eval_hidden, 16, 8, True)
            assert tr.cfg.fused_eval is False and tr._eval_net() is not None
            for E in args.episodes:
                med, last = rounds({"one_launch": lambda: tr.evaluate(E), "step_loop": lambda: tr._eval_loop(E)})
                ret, length, _ = last["one_launch"]
                longest = int(length.max())
                best = {k: min(v) for k, v in med.items()}
                emit(args.eval_out, {"what": "evaluate", "entry": "gymrl_classic_ppo_eval", "env": env_name, "hidden": args.eval_hidden,
                                     "episodes": E, "workgroups": (E + 15) // 16, "longest_episode": longest,
                                     "mean_episode": round(float(length.mean()), 1), "env_steps": int(length.sum()),
                                     "same_list": last["step_loop"] == ret[0].astype(np.float32).tolist(),
                                     "one_launch_ms": [round(m * 1e3, 4) for m in med["one_launch"]],
                                     "step_loop_ms": [round(m * 1e3, 3) for m in med["step_loop"]],
                                     "one_launch_us_per_dependent_step": round(best["one_launch"] * 1e6 / longest, 3),
                                     "step_loop_us_per_vector_step": round(best["step_loop"] * 1e6 / longest, 2),
                                     "one_launch_round_spread": round(spread(med["one_launch"]), 4),
                                     "step_loop_round_spread": round(spread(med["step_loop"]), 4),
                                     "step_loop_over_one_launch": round(best["step_loop"] / best["one_launch"], 2),
                                     "repeats": args.repeats, "rounds": args.rounds,
                                     "timer": "host clock around evaluate() / _eval_loop(), each ending in a device read-back; median per round"})


if __name__ == "__main__":
    main()
