"""Time of PPO's update() on Pendulum-v1 under the Gaussian head, both ways gymrl_amd.ppo_pendulum.PPOTrainer can run it.

  * fused    — Config.fused_update on: ppo_net.FusedGaussianUpdate.step (the categorical trainer's hand-scheduled minibatch, the
    heads as gymrl_gauss_heads_loss_fwd_bwd's one pass, d(loss) / d(log_std) written into the flat gradient by the same call)
  * autograd — Config.fused_update off: the two MLPs through torch autograd around gymrl_ppo_gauss_loss_fwd_bwd, the path this
    trainer took before the fused update covered the Gaussian head
at three shapes: the trainer's defaults (64 envs x 200 steps, 10 epochs x 8 minibatches, hidden 64) and 4096 envs x 200 steps,
`--epochs` x 32 minibatches, hidden 64 and 256.  Both trainers hold the same rollout; every call re-runs GAE, the packing, the
minibatch loop and Adam.  Host clock around a call that ends in the update's own host read of the metrics and a device synchronise;
a round's figure is the median of `--repeats` timed calls after one warm-up call; the two variants alternate inside each of
`--rounds` rounds; the line reports the median of the rounds' medians, and each variant's spread between rounds beside it — the
fused path counts as faster where the gap exceeds autograd's own spread.
Nets: freshly initialised (seed 5).  Needs an MI355X; appends one JSON line per shape to profiles/update_pendulum_micro.jsonl.

    python tools/micro_update_pendulum.py [--epochs 2] [--repeats 3] [--rounds 3] [--graphs]
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
    ap.add_argument("--epochs", type=int, default=2, help="epochs per update() at the two large shapes (the default shape keeps the trainer's 10)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--graphs", action="store_true", help="also time the fused path with Config.use_graphs (the minibatch body replayed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_pendulum_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops, ppo_net
    from gymrl_amd.ppo_pendulum import Config, PPOTrainer
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_update_pendulum.py measures on an MI355X: none found")
    sha = _lib.lib_sha256()[:16]

    def host_timed(call):
        """-> median seconds of `--repeats` calls after one warm-up call."""
        s = []
        for rep in range(args.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if rep:
                s.append(time.perf_counter() - t0)
        return statistics.median(s)

    spread = lambda v: (max(v) - min(v)) / min(v)      # noqa: E731
    d = Config()
    shapes = [("default", d.num_envs, d.update_freq, d.num_epochs, d.num_minibatches, d.hidden_dim),
              ("large", 4096, 200, args.epochs, 32, 64), ("large", 4096, 200, args.epochs, 32, 256)]
    for label, envs, steps, epochs, minibatches, hidden in shapes:
        def trainer(fused, graphs=False):
            cfg = Config()
            cfg.hidden_dim, cfg.seed, cfg.num_envs, cfg.update_freq = hidden, 5, envs, steps
            cfg.num_epochs, cfg.num_minibatches, cfg.fused_update, cfg.use_graphs = epochs, minibatches, fused, graphs
            return PPOTrainer(cfg)
        trainers = {"fused": trainer(True), "autograd": trainer(False)}
        if args.graphs:
            trainers["fused_graphs"] = trainer(True, True)
        nv = {k: t.collect_rollout() for k, t in trainers.items()}
        assert all(torch.equal(t.buffer.states, trainers["fused"].buffer.states) for t in trainers.values())
        med = {k: [] for k in trainers}
        for _ in range(args.rounds):
            for k, t in trainers.items():
                med[k].append(host_timed(lambda t=t, k=k: t.update(nv[k])))
        assert isinstance(trainers["fused"]._fused_update, ppo_net.FusedGaussianUpdate) and trainers["autograd"]._fused_update is None
        assert all(bool(torch.isfinite(t.flat_params).all()) for t in trainers.values())
        mid = {k: statistics.median(v) for k, v in med.items()}
        gap = (mid["autograd"] - mid["fused"]) / mid["autograd"]
        line = {"what": "update", "env": "Pendulum-v1", "shape": label, "hidden": hidden, "envs": envs, "steps": steps, "epochs": epochs,
                "minibatches": minibatches, "minibatch_rows": envs * steps // minibatches,
                **{f"{k}_ms": [round(m * 1e3, 3) for m in v] for k, v in med.items()},
                **{f"{k}_median_ms": round(m * 1e3, 3) for k, m in mid.items()},
                **{f"{k}_round_spread": round(spread(v), 4) for k, v in med.items()},
                "autograd_over_fused": round(mid["autograd"] / mid["fused"], 3),
                "fused_gain_over_autograd": round(gap, 4),
                "fused_faster_by_more_than_autograd_spread": gap > spread(med["autograd"]),
                "repeats": args.repeats, "rounds": args.rounds, "lib_sha256": sha,
                "timer": "host clock around update(), ending in its metric read-back and a device synchronise; median of the rounds' medians"}
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        del trainers, nv


if __name__ == "__main__":
    main()
