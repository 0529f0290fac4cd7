"""Time of a LunarLander-v3 policy evaluation of the two PPO trainers, both ways they can run it.

  * one launch — gymrl_lunar_policy_eval (csrc/eval_lunar.hip) for gymrl_amd.ppo_lunarlander at P x E of 1 x 10, 1 x 4096 and
    8 x 10, hidden 64 and 256; gymrl_lunar_mhc_eval for gymrl_amd.ppo_full_lunarlander at 1 x 10 — device events around `--batch`
    back-to-back launches of the same shape after a warm-up batch, per-launch median and minimum over `--repeats` such batches
    (tools/micro_eval_classic.py's method);
  * the same episodes through the trainer's step loop — eval() with fused_eval = False, which is what these trainers ran before
    the launch existed — for P = 1: host clock around eval(), which ends in a device synchronise.  The loop has no population
    form: P policies are P loops.  PPO-full's list is asserted equal to the launch's; PPO's is recorded as `same_list` (its loop
    runs torch's layers, the launch gymrl_mlp_forward's stages: a logit may differ in its last place).
Nets: freshly initialised (seed 5); the episodes end at their first crash.  Per-step figures divide by the longest episode, the
number of dependent steps a launch or a loop has to take.
Needs an MI355X; appends one JSON line per measurement to profiles/eval_lunar_micro.jsonl.

    python tools/micro_eval_lunar.py [--shapes 1x10 1x4096 8x10] [--hidden 64 256] [--repeats 3] [--batch 4]
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
    ap.add_argument("--shapes", nargs="+", default=["1x10", "1x4096", "8x10"], help="P x E of the MLP launches")
    ap.add_argument("--hidden", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--no-mhc", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_lunar_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_eval_lunar.py measures on an MI355X: none found")
    sha = _lib.lib_sha256()[:16]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(line):
        line["lib_sha256"] = sha
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    def timed_launches(launch):
        ms = []
        for rep in range(args.repeats + 1):                                       # batch 0 warms the shape up
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.batch):
                out = launch()
            stop.record()
            torch.cuda.synchronize()
            if rep:
                ms.append(start.elapsed_time(stop) / args.batch)
        return ms, out

    def timed_loop(tr, E):
        s = []
        for rep in range(args.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            returns = tr.eval(E)                                                  # fused_eval is False: the step loop
            torch.cuda.synchronize()
            if rep:
                s.append(time.perf_counter() - t0)
        return s, returns

    def report(algo, entry, hidden, P, E, ms, length):
        med, longest = statistics.median(ms), int(length.max().item())
        emit({"what": "one_launch", "entry": entry, "algo": algo, "hidden": hidden, "policies": P, "episodes": E,
              "workgroups": P * ((E + 15) // 16), "longest_episode": longest, "mean_episode": round(float(length.float().mean().item()), 1),
              "env_steps": int(length.sum().item()), "launch_ms_median": round(med, 4), "launch_ms_min": round(min(ms), 4),
              "us_per_dependent_step": round(med * 1e3 / longest, 3), "repeats": args.repeats, "launches_per_repeat": args.batch,
              "timer": "device events around a batch of launches, outputs allocated inside"})
        return longest

    def report_loop(algo, hidden, E, s, longest, same):
        med = statistics.median(s)
        emit({"what": "trainer_eval_step_loop", "algo": algo, "hidden": hidden, "policies": 1, "episodes": E, "same_list": same,
              "vector_steps": longest, "loop_ms_median": round(med * 1e3, 3), "loop_ms_min": round(min(s) * 1e3, 3),
              "us_per_vector_step_median": round(med * 1e6 / longest, 2), "repeats": args.repeats,
              "timer": "host clock around eval(), ending in a device synchronise"})

    from gymrl_amd import ppo_full_lunarlander, ppo_lunarlander
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes]
    for hidden in args.hidden:
        cfg = ppo_lunarlander.Config()
        cfg.hidden_dim, cfg.seed, cfg.num_envs, cfg.update_freq = hidden, 5, 16, 8
        tr = ppo_lunarlander.PPOTrainer(cfg)
        assert tr.cfg.fused_eval is False
        net = tr._eval_net()
        seed, id0 = tr.base_seed + tr.EVAL_SEED_OFFSET, tr.EVAL_ENV_ID0
        looped = set()
        for P, E in shapes:
            policy = net if P == 1 else ops.LunarPolicyStack(net, tr.flat_params, tr.flat_params.detach().repeat(P, 1))
            ms, out = timed_launches(lambda: ops.lunar_policy_eval(policy, E, seed, id0, want_terminal_obs=False, device=tr.device))
            longest = report("ppo_lunarlander", "gymrl_lunar_policy_eval", hidden, P, E, ms, out[1])
            if E not in looped and P == 1:
                looped.add(E)
                s, returns = timed_loop(tr, E)
                report_loop("ppo_lunarlander", hidden, E, s, longest, returns == out[0][0].to(torch.float32).tolist())
    if not args.no_mhc:
        cfg = ppo_full_lunarlander.Config()
        cfg.seed, cfg.num_envs, cfg.update_freq = 5, 16, 8
        tr = ppo_full_lunarlander.PPOTrainer(cfg)
        desc = tr._eval_desc()
        assert desc is not None and tr.cfg.fused_eval is False
        seed, id0, E = tr.base_seed + tr.EVAL_SEED_OFFSET, tr.EVAL_ENV_ID0, 10
        ms, out = timed_launches(lambda: ops.lunar_mhc_eval(desc, E, seed, id0, want_terminal_obs=False, device=tr.device))
        longest = report("ppo_full_lunarlander", "gymrl_lunar_mhc_eval", cfg.mhc_dim, 1, E, ms, out[1])
        s, returns = timed_loop(tr, E)
        same = returns == out[0][0].to(torch.float32).tolist()
        assert same, "the step loop is not the launch's episodes"
        report_loop("ppo_full_lunarlander", cfg.mhc_dim, E, s, longest, same)


if __name__ == "__main__":
    main()
