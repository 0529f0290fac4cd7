"""Time of a LunarLander-v3 policy evaluation of the recurrent trainers (gymrl_amd.ppg_rnn_lunarlander; ppo_rnn_lunarlander runs
the same code without the aux head), both ways they can run it.

  * one launch — gymrl_lunar_mlprnn_eval (csrc/eval_lunar_rnn.hip) at P x E of 1 x 10, 1 x 4096 and 8 x 10: device events around
    `--batch` back-to-back launches of the same shape after a warm-up batch, per-launch median and minimum over `--repeats` such
    batches (tools/micro_eval_classic.py's method);
  * the same episodes through the trainer's step loop — eval() with fused_eval = False, which is what these trainers ran before
    the launch existed — for P = 1: host clock around eval(), which ends in a device synchronise (its per-episode print goes to
    the null device).  The loop has no population form: P policies are P loops.  Its lengths are not returned; its float32
    returns are recorded as `same_list` against the launch's float64 ones cast to float32 (they may differ in the last place).
Net: freshly initialised (seed 5), observation statistics after 256 rows of a random-action rollout (fresh statistics have
std = 0); the episodes end at their first crash.  Per-step figures divide by the longest episode, the number of dependent steps
a launch or a loop has to take.
Needs an MI355X; appends one JSON line per measurement to profiles/eval_mlprnn_micro.jsonl.

    python tools/micro_eval_mlprnn.py [--shapes 1x10 1x4096 8x10] [--repeats 3] [--batch 4]
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1x10", "1x4096", "8x10"], help="P x E of the launches")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_mlprnn_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops, ppg_rnn_lunarlander
    from gymrl_amd.envs import VecEnv
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_eval_mlprnn.py measures on an MI355X: none found")
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
        with open(os.devnull, "w") as null, contextlib.redirect_stdout(null):
            for rep in range(args.repeats + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                returns = tr.eval(E)                                              # fused_eval is False: the step loop
                torch.cuda.synchronize()
                if rep:
                    s.append(time.perf_counter() - t0)
        return s, returns

    cfg = ppg_rnn_lunarlander.Config()
    cfg.seed, cfg.save_path = 5, os.path.join(tempfile.mkdtemp(), "ck.pth")
    tr = ppg_rnn_lunarlander.PPGTrainer(cfg)
    assert tr.cfg.fused_eval is False
    # observation statistics: 16 envs x 16 steps under random actions
    env = VecEnv("LunarLander-v3", 16, device=tr.device, seed=100, env_id0=0)
    gen = torch.Generator(device="cpu").manual_seed(0)
    obs, rew, rows = env.reset(), torch.empty(16, device=tr.device), []
    for _ in range(16):
        rows.append(obs.clone())
        env.step(torch.randint(0, 4, (16,), generator=gen, dtype=torch.int32).to(tr.device), obs, rew)
    env.close()
    stats = tr.state_norm.running_ms.stats
    ops.running_norm_masked(torch.cat(rows), torch.ones(256, dtype=torch.uint8, device=tr.device), stats, update=True)

    seed, id0 = tr.base_seed + tr.EVAL_SEED_OFFSET, tr.EVAL_ENV_ID0
    looped = set()
    for P, E in (tuple(int(v) for v in s.split("x")) for s in args.shapes):
        policy = tr._act_params if P == 1 else ops.MlprnnPolicyStack(tr.net, tr.flat_params, tr.flat_params.detach().repeat(P, 1))
        ms, out = timed_launches(lambda: ops.lunar_mlprnn_eval(policy, E, seed, id0, norm_stats=stats, want_terminal_obs=False))
        length = out[1]
        med, longest = statistics.median(ms), int(length.max().item())
        emit({"what": "one_launch", "entry": "gymrl_lunar_mlprnn_eval", "algo": "ppg_rnn_lunarlander", "threads": 256, "policies": P,
              "episodes": E, "workgroups": P * ((E + 15) // 16), "longest_episode": longest,
              "mean_episode": round(float(length.float().mean().item()), 1), "env_steps": int(length.sum().item()),
              "launch_ms_median": round(med, 4), "launch_ms_min": round(min(ms), 4),
              "us_per_dependent_step": round(med * 1e3 / longest, 3), "repeats": args.repeats, "launches_per_repeat": args.batch,
              "timer": "device events around a batch of launches, outputs allocated inside"})
        if E not in looped and P == 1:
            looped.add(E)
            s, returns = timed_loop(tr, E)
            lmed = statistics.median(s)
            emit({"what": "trainer_eval_step_loop", "algo": "ppg_rnn_lunarlander", "policies": 1, "episodes": E,
                  "same_list": returns == out[0][0].to(torch.float32).tolist(), "vector_steps": longest,
                  "loop_ms_median": round(lmed * 1e3, 3), "loop_ms_min": round(min(s) * 1e3, 3),
                  "us_per_vector_step_median": round(lmed * 1e6 / longest, 2), "loop_over_launch": round(lmed * 1e3 / med, 2),
                  "repeats": args.repeats, "timer": "host clock around eval(), ending in a device synchronise"})


if __name__ == "__main__":
    main()
