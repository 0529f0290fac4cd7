"""Time of one collection round of the recurrent LunarLander trainers (gymrl_amd.ppg_rnn_lunarlander; ppo_rnn_lunarlander runs
the same code without the aux head), both ways collect_round() can run it.

  * the step loop — Config.fused_collect = False, what these trainers ran before the launch existed: per vector step an env
    step, two statistics launches, the acting launch, four elementwise ops and every sixteenth step a read-back;
  * one launch — Config.fused_collect = True, gymrl_lunar_mlprnn_collect (csrc/collect_lunar_rnn.hip), one workgroup.

Two trainers are built from the same seed, one per way, and play the same rounds in lockstep (the launch is the loop bit for
bit, so round r has the same episodes in both): per round the loop is timed, then the launch, alternating, a host clock around
collect_round() — which ends in a read-back of the lengths and the returns, so the device has finished — after `--warmup`
untimed rounds of each.  Every timed round is recorded with its episode lengths; the summary line has the medians, the extremes
and the ratio of the medians.  `same` says the two trainers returned the same lengths and returns in every round.

Policies: "fresh" (freshly initialised, seed 5: episodes end at their first crash after roughly 100 steps) and "trained" (the same
net after `--train-seconds` of PPG training at num_envs = 16, batch_size = 16 on the launch: longer episodes; its parameters
and statistics are copied into every pair of trainers).  num_envs: 1, 4 and 16.
Needs an MI355X; appends one JSON line per round and per summary to profiles/collect_mlprnn_micro.jsonl.

    python tools/micro_collect_mlprnn.py [--envs 1 4 16] [--repeats 7] [--warmup 2] [--train-seconds 90]
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
    ap.add_argument("--envs", nargs="+", type=int, default=[1, 4, 16])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--train-seconds", type=float, default=90.0, help="0: no trained policy")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collect_mlprnn_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops, ppg_rnn_lunarlander as ppg
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_collect_mlprnn.py measures on an MI355X: none found")
    sha = _lib.lib_sha256()[:16]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    tmp = tempfile.mkdtemp()

    def emit(line):
        line["lib_sha256"] = sha
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    def trainer(N, fused, batch=None):
        cfg = ppg.Config()
        cfg.seed, cfg.num_envs, cfg.batch_size, cfg.fused_collect = 5, N, batch or max(4, N), fused
        cfg.save_path = os.path.join(tmp, f"ck_{N}_{int(fused)}.pth")
        with open(os.devnull, "w") as null, contextlib.redirect_stdout(null):
            return ppg.PPGTrainer(cfg)

    def timed_round(tr):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = tr.collect_round()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        tr._batch = []
        return dt * 1e3, out

    policies = {"fresh": None}
    if args.train_seconds > 0:
        tr = trainer(16, True, batch=16)
        t0, updates, lengths = time.perf_counter(), 0, []
        while time.perf_counter() - t0 < args.train_seconds:
            _, lengths = tr.collect_round()
            tr.update()
            updates += 1
        policies["trained"] = (tr.flat_params.clone(), tr.state_norm.running_ms.stats.clone(),
                               tr.reward_scaler.running_ms.stats.clone())
        emit({"what": "trained_policy", "algo": "ppg_rnn_lunarlander", "num_envs": 16, "batch_size": 16, "updates": updates,
              "train_seconds": round(time.perf_counter() - t0, 1), "last_round_lengths": lengths})

    for name, state in policies.items():
        for N in args.envs:
            pair = {"loop": trainer(N, False), "launch": trainer(N, True)}
            for tr in pair.values():
                if state is not None:
                    tr.flat_params.copy_(state[0])
                    tr.state_norm.running_ms.stats.copy_(state[1])
                    tr.reward_scaler.running_ms.stats.copy_(state[2])
            ms, same = {"loop": [], "launch": []}, True
            for r in range(args.warmup + args.repeats):
                outs = {}
                for way, tr in pair.items():                                      # alternating, the loop first
                    dt, outs[way] = timed_round(tr)
                    if r >= args.warmup:
                        ms[way].append(dt)
                same = same and outs["loop"] == outs["launch"]
                if r >= args.warmup:
                    emit({"what": "round", "policy": name, "num_envs": N, "round": r, "lengths": outs["loop"][1],
                          "loop_ms": round(ms["loop"][-1], 3), "launch_ms": round(ms["launch"][-1], 3)})
            med = {w: statistics.median(v) for w, v in ms.items()}
            emit({"what": "collect_round", "algo": "ppg_rnn_lunarlander", "policy": name, "num_envs": N, "same": same,
                  "loop_ms_median": round(med["loop"], 3), "loop_ms_min": round(min(ms["loop"]), 3),
                  "loop_ms_max": round(max(ms["loop"]), 3), "launch_ms_median": round(med["launch"], 3),
                  "launch_ms_min": round(min(ms["launch"]), 3), "launch_ms_max": round(max(ms["launch"]), 3),
                  "loop_over_launch": round(med["loop"] / med["launch"], 2),
                  "per_round_ratio_min": round(min(a / b for a, b in zip(ms["loop"], ms["launch"])), 2),
                  "per_round_ratio_max": round(max(a / b for a, b in zip(ms["loop"], ms["launch"])), 2),
                  "repeats": args.repeats, "warmup": args.warmup,
                  "timer": "host clock around collect_round(), which ends in a read-back; loop and launch alternate"})


if __name__ == "__main__":
    main()
