"""Time of a policy evaluation of the dueling trainers (CartPole-v1) and of SAC-Pendulum, both ways the trainers can run it.

  * one launch — gymrl_classic_duel_eval (csrc/eval_duel.hip) for dueling DDQN+PER, NoisyNet dueling DQN and Rainbow, P x E of
    1 x 10, 1 x 4096 and 8 x 4096; gymrl_classic_policy_eval on (fc1, fc2, mean) for SAC-Pendulum at 1 x 10 — device events around
    `--batch` back-to-back launches of the same shape after a warm-up batch, per-launch median and minimum over `--repeats` such
    batches (tools/micro_eval_classic.py's method);
  * the same episodes through the trainer's step loop — eval() with fused_eval = False, which is what these trainers ran before
    the launch existed — for P = 1: host clock around eval(), which ends in a device synchronise.  Its list is asserted equal to
    the launch's (SAC-Pendulum: recorded as `same_list`; its loop takes torch.tanh, the launch the kernels' tanh epilogue).  The loop
    has no population form: P policies are P loops.
Nets: CartPole — a dueling network that holds the pole to the TimeLimit (a linear controller through a ReLU pair into the
advantage head, the value head zero, the rest of the trunk at its initial values so that it is streamed whole; a fresh net falls
within tens of steps); Pendulum — the freshly initialised actor, 200 steps.  Hidden 64 and 256.
Needs an MI355X; appends one JSON line per measurement to profiles/eval_duel_micro.jsonl.

    python tools/micro_eval_duel.py [--algos ...] [--shapes 1x10 1x4096 8x4096] [--hidden 64 256] [--repeats 3] [--batch 4]
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
DUEL = {"ddqn_per_duel_cartpole": "DDQNPERDuelTrainer", "noisy_dqn_cartpole": "NoisyDQNTrainer", "rainbow_dqn_cartpole": "RainbowDQNTrainer"}


def make_trainer(algo, hidden):
    import importlib
    import torch
    mod = importlib.import_module("gymrl_amd." + algo)
    cfg = mod.Config()
    cfg.hidden_dim, cfg.seed, cfg.memory_capacity = hidden, 5, 4096
    tr = getattr(mod, DUEL.get(algo, "SACTrainer"))(cfg)
    if algo in DUEL:
        trunk, value, adv, _ = tr._eval_duel_policy()
        with torch.no_grad():
            k = torch.tensor(CONTROLLER, device=tr.device)
            trunk[0][0][0], trunk[0][0][1] = k, -k
            trunk[0][1][:2] = 0.0
            if len(trunk) == 2:
                trunk[1][0][:2] = 0.0
                trunk[1][0][0, 0] = trunk[1][0][1, 1] = 1.0
                trunk[1][1][:2] = 0.0
            for t in (*value, *adv):
                t.zero_()
            adv[0][0, 1] = adv[0][1, 0] = 1.0
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1x10", "1x4096", "8x4096"], help="P x E of the dueling launches")
    ap.add_argument("--algos", nargs="+", default=list(DUEL) + ["sac_pendulum"])
    ap.add_argument("--hidden", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_duel_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_eval_duel.py measures on an MI355X: none found")
    sha = _lib.lib_sha256()[:16]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(line):
        line["lib_sha256"] = sha
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes]
    for algo in args.algos:
        for hidden in args.hidden:
            tr = make_trainer(algo, hidden)
            call = tr._eval_call()
            assert call is not None and tr.cfg.fused_eval is False
            seed, id0 = tr.base_seed + tr.EVAL_SEED_OFFSET, tr.EVAL_ENV_ID0
            looped = {}
            for P, E in (shapes if algo in DUEL else [(1, 10)]):
                params = None if P == 1 else call["flat"].repeat(P, 1)
                ms = []
                for rep in range(args.repeats + 1):                               # batch 0 warms the shape up
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    for _ in range(args.batch):
                        ret, length, term = tr._eval_launch(call, n_episodes=E, seed=seed, stream_id0=id0, params=params)
                    stop.record()
                    torch.cuda.synchronize()
                    if rep:
                        ms.append(start.elapsed_time(stop) / args.batch)
                med, longest, steps = statistics.median(ms), int(length.max().item()), int(length.sum().item())
                emit({"what": "one_launch", "entry": "gymrl_classic_duel_eval" if algo in DUEL else "gymrl_classic_policy_eval",
                      "algo": algo, "hidden": hidden, "policies": P, "episodes": E, "workgroups": P * ((E + 15) // 16),
                      "longest_episode": longest, "env_steps": steps, "launch_ms_median": round(med, 4), "launch_ms_min": round(min(ms), 4),
                      "us_per_dependent_step": round(med * 1e3 / longest, 3), "repeats": args.repeats, "launches_per_repeat": args.batch,
                      "timer": "device events around a batch of launches, outputs allocated inside"})
                if E in looped:
                    assert all(ret[p].tolist() == looped[E] for p in range(P)), "a population member is not the loop's episodes"
                    continue
                s = []
                for rep in range(args.repeats + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    loop_returns = tr.eval(E)                                     # fused_eval is False: the step loop
                    torch.cuda.synchronize()
                    if rep:
                        s.append(time.perf_counter() - t0)
                # (SAC-Pendulum: the same episodes under torch.tanh in place of the kernels' tanh — returns equal to six digits, not bits)
                same = loop_returns == ret[0].tolist()
                assert same or algo not in DUEL, "the step loop is not the launch's episodes"
                looped[E] = loop_returns
                med = statistics.median(s)
                emit({"what": "trainer_eval_step_loop", "algo": algo, "hidden": hidden, "policies": 1, "episodes": E, "same_list": same,
                      "vector_steps": longest, "loop_ms_median": round(med * 1e3, 3), "loop_ms_min": round(min(s) * 1e3, 3),
                      "us_per_vector_step_median": round(med * 1e6 / longest, 2), "repeats": args.repeats,
                      "timer": "host clock around eval(), ending in a device synchronise"})


if __name__ == "__main__":
    main()
