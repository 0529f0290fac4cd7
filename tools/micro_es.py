"""Time of one evolution-strategies generation's stages on CartPole-v1 (gymrl_amd/es.py, csrc/es.hip), against a plain-torch
restatement of the same method on the same machine.

For (population, hidden) in (64, 64), (256, 64), (4096, 64), (256, 256), (4096, 256), E = 1 episode per policy:

  * ask    OpenAIES.ask(): gymrl_es_perturb, one launch;
  * eval   the evaluators' launch on the stack (gymrl_classic_policy_eval), for scale;
  * tell   OpenAIES.tell(): gymrl_es_shape_grad (one launch up to 256 policies, two above) + gymrl_adam_step;
  * torch  the same generation without the kernels: torch.randn [P / 2, n], the stack by two strided assignments, ranks by
           argsort + scatter (ties NOT averaged: one pass less than the kernel's rule), the [P / 2] x [P / 2, n] product, the
           SAME FusedAdam.  It materialises the noise and reads it back; it is what a user of evaluate() would write.

Device events around a batch of back-to-back calls after a warm-up batch, per-call median and minimum over `--repeats` batches;
the kernels' batch and torch's alternate inside one repeat, so both see the same machine state.  A batch is 200 calls at the small
shapes and 20 at the large ones: 4 to 40 ms per timed window.  Needs an MI355X; appends one JSON line per shape to profiles/es_micro.jsonl.

    python tools/micro_es.py [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SHAPES = ((64, 64), (256, 64), (4096, 64), (256, 256), (4096, 256))


class TorchES:
    """ask / tell in plain torch on the trainer's centre and an Adam of its own kind."""

    def __init__(self, theta, population, sigma, lr, seed):
        import torch
        from gymrl_amd.flat import FusedAdam
        self.torch, self.theta, self.P, self.sigma = torch, theta, population, sigma
        self.gen = torch.Generator(device=theta.device)
        self.gen.manual_seed(seed)
        self.grad = torch.zeros_like(theta)
        self.opt = FusedAdam(theta, self.grad, lr=lr)
        self.stack = torch.empty(population, theta.numel(), device=theta.device)
        self.arange = torch.arange(population, device=theta.device, dtype=torch.float32)
        self.ranks = torch.empty(population, device=theta.device)
        self.eps = None

    def ask(self):
        torch = self.torch
        self.eps = torch.randn(self.P // 2, self.theta.numel(), generator=self.gen, device=self.theta.device)
        step = self.sigma * self.eps
        self.stack[0::2] = self.theta + step
        self.stack[1::2] = self.theta - step
        return self.stack

    def tell(self, returns):
        torch = self.torch
        fitness = returns.sum(dim=1)
        self.ranks[torch.argsort(fitness)] = self.arange
        w = self.ranks / (self.P - 1) - 0.5
        u = w[0::2] - w[1::2]
        torch.mul(u @ self.eps, -1.0 / (self.P * self.sigma), out=self.grad)
        self.opt.step()


def timed(torch, fn, batch):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(batch):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / batch            # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "es_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops
    from gymrl_amd.es_cartpole import Config, ESTrainer
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_es.py measures on an MI355X: none found")
    sha = _lib.lib_sha256()[:16]
    lines = []
    for P, hidden in SHAPES:
        cfg = Config()
        cfg.seed, cfg.population, cfg.hidden_dim, cfg.episodes_per_policy, cfg.log_freq = 3, P, hidden, 1, 0
        tr = ESTrainer(cfg)
        es, n = tr.es, tr.flat_params.numel()
        ref = TorchES(tr.flat_params.clone(), P, cfg.sigma, cfg.lr, cfg.seed)
        seed, id0 = tr.base_seed + tr.EVAL_SEED_OFFSET, tr.TRAIN_ENV_ID0
        evaluate = lambda: tr._eval_launch(tr._call, n_episodes=1, seed=seed, stream_id0=id0, params=es.stack)     # noqa: E731
        es.ask()
        returns = evaluate()[0]
        ref.ask()
        batch = 200 if P * n < (1 << 22) else 20
        fns = {"ask": es.ask, "tell": lambda: es.tell(returns), "eval": evaluate, "torch_ask": ref.ask,
               "torch_tell": lambda: ref.tell(returns)}
        us = {k: [] for k in fns}
        for rep in range(args.repeats + 1):                      # repeat 0 warms every call of the shape up
            for name, fn in fns.items():
                t = timed(torch, fn, batch)
                if rep:
                    us[name].append(t)
        med = {k: statistics.median(v) for k, v in us.items()}
        ours, theirs = med["ask"] + med["tell"], med["torch_ask"] + med["torch_tell"]
        line = {"what": "es_generation_stages", "env": "CartPole-v1", "population": P, "hidden": hidden, "n_params": n,
                "episodes_per_policy": 1, "pair_chunk": ops.ES_PAIR_CHUNK, "tell_launches": 2 if P <= 256 else 3,
                "perturb_bytes": P * n * 4, "normals_per_stage": P // 2 * n}
        for k in fns:
            line[k + "_us_median"], line[k + "_us_min"] = round(med[k], 2), round(min(us[k]), 2)
        line.update({"ask_plus_tell_us": round(ours, 2), "torch_ask_plus_tell_us": round(theirs, 2),
                     "torch_over_kernels": round(theirs / ours, 3), "repeats": args.repeats, "calls_per_repeat": batch,
                     "timer": "device events around a batch of back-to-back calls, kernels and torch alternating per repeat",
                     "lib_sha256": sha})
        lines.append(line)
        print(json.dumps(line), flush=True)
        del tr, ref, es
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    slower = [(ln["population"], ln["hidden"]) for ln in lines if ln["torch_over_kernels"] < 1.0]
    if slower:
        raise SystemExit(f"ask + tell is slower than the torch restatement at {slower}")


if __name__ == "__main__":
    main()
