"""Time of the MountainCar-v0 rule baseline's evaluation, both ways the package can run it.

  * one gymrl_mountaincar_rule_eval launch (csrc/mountaincar.hip) for P * E = 10, 4096 and 2^20 episodes of the reference's rule:
    device events around `--batch` back-to-back launches of the same shape after a warm-up launch, per-launch median and
    minimum over `--repeats` such batches;
  * the same episodes through VecEnv.step and a host policy (one launch, one observation copy to the host, a vectorised NumPy
    rule and one action copy to the device per step, until every env's first episode is over) for N = 10 and 4096: host clock
    around the loop, which ends in a device synchronise; the loop's episode lengths are checked against the launch's.
Needs an MI355X; appends one JSON line per measurement to profiles/mountaincar_micro.jsonl.

    python tools/micro_mountaincar.py [--episodes 10 4096 1048576] [--stepped 10 4096] [--repeats 5] [--batch 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SEED, STREAM0 = 42, 1 << 40


def rule_rows(obs, k):
    """The rule on obs f32[N, 2] in float64, powers as products -> i32[N]."""
    p, v = obs[:, 0].astype(np.float64), obs[:, 1].astype(np.float64)
    a = p + k[1]
    l1 = k[0] * (a * a) + k[2]
    b = p + k[4]
    b2 = b * b
    l2 = k[3] * (b2 * b2) - k[5]
    lb = np.where(l1 < l2, l1, l2)
    c = p + k[7]
    ub = k[6] * (c * c) + k[8]
    return np.where((lb < v) & (v < ub), 2, 0).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, nargs="+", default=[10, 4096, 1 << 20])
    ap.add_argument("--stepped", type=int, nargs="+", default=[10, 4096])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mountaincar_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops
    from gymrl_amd.envs import VecEnv
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_mountaincar.py measures on an MI355X: none found")
    dev = torch.device("cuda:0")
    sha = _lib.lib_sha256()[:16]
    lines, lengths = [], {}
    for n in args.episodes:
        ms = []
        for rep in range(args.repeats + 1):                       # batch 0 warms the shape up
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.batch):
                ret, length, reached = ops.mountaincar_rule_eval(n, SEED, STREAM0, 200, dev)
            stop.record()
            torch.cuda.synchronize()
            if rep:
                ms.append(start.elapsed_time(stop) / args.batch)
        lengths[n] = length[0].cpu().numpy()
        steps = int(lengths[n].sum())
        med = statistics.median(ms)
        lines.append({"what": "mountaincar_rule_eval_one_launch", "episodes": n, "env_steps": steps, "longest_episode": int(lengths[n].max()),
                      "reached_share": round(float(reached.float().mean().item()), 4), "launch_ms_median": round(med, 4),
                      "launch_ms_min": round(min(ms), 4), "env_steps_per_s_median": round(steps / (med * 1e-3), 1), "repeats": args.repeats,
                      "launches_per_repeat": args.batch, "timer": "device events around a batch of launches, outputs allocated inside",
                      "lib_sha256": sha})
        print(json.dumps(lines[-1]), flush=True)
    for n in args.stepped:
        s = []
        for rep in range(args.repeats + 1):
            env = VecEnv("MountainCar-v0", n, device=dev, seed=SEED, env_id0=STREAM0)
            obs, rew = torch.empty(n, 2, device=dev), torch.empty(n, device=dev)
            done, ep_len = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.reset(obs)
            over, vector_steps = np.zeros(n, bool), 0
            while not over.all():
                act = torch.from_numpy(rule_rows(obs.cpu().numpy(), ops.MOUNTAINCAR_RULE_COEFS)).to(dev)
                env.step(act, obs, rew, done_out=done, ep_len_out=ep_len)
                over |= done.cpu().numpy().astype(bool)
                vector_steps += 1
            torch.cuda.synchronize()
            if rep:
                s.append(time.perf_counter() - t0)
        if n in lengths:
            assert vector_steps == int(lengths[n].max()), "the stepped loop is not the launch's episodes"
        med = statistics.median(s)
        lines.append({"what": "mountaincar_vecenv_step_host_policy", "envs": n, "vector_steps": vector_steps, "loop_ms_median": round(med * 1e3, 3),
                      "loop_ms_min": round(min(s) * 1e3, 3), "ms_per_vector_step_median": round(med * 1e3 / vector_steps, 4),
                      "repeats": args.repeats, "timer": "host clock around the loop, ending in a device synchronise",
                      "lib_sha256": sha})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
