"""Time of PPO's update() on Acrobot-v1 and MountainCar-v0, both ways gymrl_amd.ppo_lunarlander.PPOTrainer can run it.

  * update — update() with Config.fused_update on (ppo_net.FusedActorCriticUpdate.step: the hand-written f32-MFMA GEMMs of
    csrc/gemm.hip plus the fused passes of csrc/mlp_train.hip, the heads as gymrl_heads_loss_fwd_bwd's one pass) and off (torch
    autograd around gymrl_ppo_loss_fwd_bwd: the path these envs took before the fused update covered three actions), at
    N = `--envs`, T = `--steps`, hidden in `--hidden`, `--epochs` x `--minibatches` minibatches per call.  Both trainers hold the
    same rollout; every call re-runs GAE, the packing, the minibatch loop and Adam.  Host clock around a call that ends in the
    update's own host read of the metrics and a device synchronise; a figure is the median of `--repeats` timed calls after one
    warm-up call; the two variants alternate inside each of `--rounds` rounds, and the spread between a variant's rounds is
    reported beside the ratio it has to be read against.
  * heads — for information: gymrl_heads_loss_fwd_bwd (one pass) against gymrl_heads_fwd_tanh -> gymrl_ppo_loss_fwd_bwd ->
    gymrl_heads_bwd (three passes) at four actions, hidden 64 and 128, `--heads-rows` rows, where step() keeps the three
    passes.  Device events around each variant's launches, the same repeats and rounds.
Nets: freshly initialised (seed 5).  Needs an MI355X; appends one JSON line per measurement to profiles/update_classic_micro.jsonl.

    python tools/micro_update_classic.py [--envs 4096] [--steps 256] [--hidden 64 256] [--epochs 4] [--minibatches 8] [--repeats 3] [--rounds 2]
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
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--hidden", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=8)
    ap.add_argument("--heads-rows", type=int, default=262144)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-update", action="store_true")
    ap.add_argument("--no-heads", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_classic_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops
    from gymrl_amd.ppo_lunarlander import Config, PPOTrainer
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_update_classic.py measures on an MI355X: none found")
    sha = _lib.lib_sha256()[:16]
    dev = torch.device("cuda:0")

    def emit(line):
        line["lib_sha256"] = sha
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")

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

    def event_timed(call):
        s = []
        for rep in range(args.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                s.append(e0.elapsed_time(e1) * 1e-3)
        return statistics.median(s)

    def rounds(variants, timed):
        """name -> call: every variant once per round, in turn -> name -> [median per round]."""
        med = {k: [] for k in variants}
        for _ in range(args.rounds):
            for name, call in variants.items():
                med[name].append(timed(call))
        return med

    spread = lambda v: (max(v) - min(v)) / min(v)      # noqa: E731

    def trainer(env_name, hidden, fused):
        cfg = Config()
        cfg.env_name, cfg.hidden_dim, cfg.seed, cfg.num_envs, cfg.update_freq = env_name, hidden, 5, args.envs, args.steps
        cfg.num_epochs, cfg.num_minibatches, cfg.fused_update = args.epochs, args.minibatches, fused
        return PPOTrainer(cfg)

    if not args.no_update:
        for env_name in ("Acrobot-v1", "MountainCar-v0"):
            for hidden in args.hidden:
                fused, plain = trainer(env_name, hidden, True), trainer(env_name, hidden, False)
                nv = {id(t): t.collect_rollout() for t in (fused, plain)}
                assert torch.equal(fused.buffer.states, plain.buffer.states)
                med = rounds({"fused": lambda: fused.update(nv[id(fused)]), "autograd": lambda: plain.update(nv[id(plain)])}, host_timed)
                assert fused._fused_update is not None and fused._fused_update.one_pass_heads and plain._fused_update is None
                assert bool(torch.isfinite(fused.flat_params).all()) and bool(torch.isfinite(plain.flat_params).all())
                best = {k: min(v) for k, v in med.items()}
                total = args.envs * args.steps
                emit({"what": "update", "env": env_name, "hidden": hidden, "envs": args.envs, "steps": args.steps,
                      "epochs": args.epochs, "minibatches": args.minibatches, "minibatch_rows": total // args.minibatches,
                      "fused_ms": [round(m * 1e3, 3) for m in med["fused"]],
                      "autograd_ms": [round(m * 1e3, 3) for m in med["autograd"]],
                      "fused_round_spread": round(spread(med["fused"]), 4),
                      "autograd_round_spread": round(spread(med["autograd"]), 4),
                      "autograd_over_fused": round(best["autograd"] / best["fused"], 3),
                      "slowest_fused_beats_fastest_autograd": max(med["fused"]) < min(med["autograd"]),
                      "repeats": args.repeats, "rounds": args.rounds,
                      "timer": "host clock around update(), ending in its metric read-back and a device synchronise; median per round"})
                del fused, plain

    if not args.no_heads:
        cfg = (0.2, 3.0, 0.5, 0.01)
        B, A = args.heads_rows, 4
        for C in (64, 128):
            g = torch.Generator(device=dev).manual_seed(C)
            Zac = torch.randn(B, 2 * C, device=dev, generator=g)
            Wa2, ba2 = torch.randn(A, C, device=dev, generator=g) / 8, 0.1 * torch.randn(A, device=dev, generator=g)
            Wc2, bc2 = torch.randn(1, C, device=dev, generator=g) / 16, 0.1 * torch.randn(1, device=dev, generator=g)
            act = torch.randint(0, A, (B,), device=dev, generator=g, dtype=torch.int32)
            lpo = -1.386 + 0.2 * torch.randn(B, device=dev, generator=g)
            adv, ret = torch.randn(B, device=dev, generator=g), torch.randn(B, device=dev, generator=g)
            ws = ops.mlp_train_workspace(C, 8, A, dev)
            Z = Zac.clone()
            logits, value = torch.empty(B, A, device=dev), torch.empty(B, 1, device=dev)
            dl, dv = torch.empty(B, A, device=dev), torch.empty(B, device=dev)
            outs = [torch.empty(2 * C, device=dev), torch.empty(A, C, device=dev), torch.empty(A, device=dev),
                    torch.empty(1, C, device=dev), torch.empty(1, device=dev)]
            parts1 = torch.zeros(ops.heads_loss_blocks(B, C), 5, dtype=torch.float64, device=dev)
            parts3 = torch.zeros(ops.loss_blocks(B), 5, dtype=torch.float64, device=dev)

            # (both variants overwrite Z with dZac and read it again as pre-activations: the values differ, the traffic does not)
            def one():
                ops.heads_loss_fwd_bwd(Z, None, Wa2, ba2, Wc2, bc2, act, lpo, adv, ret, cfg, None, *outs, parts1, ws)

            def three():
                ops.heads_fwd_tanh(Z, Wa2, ba2, Wc2, bc2, logits, value, None, False)
                ops.ppo_loss_fwd_bwd(logits, value.view(-1), act, lpo, adv, ret, cfg, dlogits_out=dl, dvalue_out=dv, workspace=parts3)
                ops.heads_bwd(Z, dl, dv, Wa2, Wc2, Z, *outs, ws, True, None)
            med = rounds({"one_pass": one, "three_passes": three}, event_timed)
            best = {k: min(v) for k, v in med.items()}
            emit({"what": "heads", "hidden": C, "actions": A, "rows": B,
                  "one_pass_us": [round(m * 1e6, 2) for m in med["one_pass"]],
                  "three_passes_us": [round(m * 1e6, 2) for m in med["three_passes"]],
                  "one_pass_round_spread": round(spread(med["one_pass"]), 4),
                  "three_passes_round_spread": round(spread(med["three_passes"]), 4),
                  "three_over_one": round(best["three_passes"] / best["one_pass"], 3),
                  "repeats": args.repeats, "rounds": args.rounds,
                  "timer": "device events around the variant's launches (one pass: 2, three passes: 4); median per round"})


if __name__ == "__main__":
    main()
