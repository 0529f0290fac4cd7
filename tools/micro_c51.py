"""Timings of the categorical (C51) head on an MI355X -> profiles/c51_micro.jsonl, and the learning runs of its two trainers.

    python tools/micro_c51.py                        # the micro-benchmarks below
    python tools/micro_c51.py learn c51_cartpole     # train() at the module's defaults, seed 0 -> profiles/<module>_learning.txt
    python tools/micro_c51.py learn c51_per_cartpole

Micro-benchmarks (device events around `iters` back-to-back calls after a warm-up, best and median of `reps` windows):
  * ops.c51_loss at B in {64, 256, 8192}, A = 2, M = 51 (double-Q, weighted, with the loss sum) against the same loss composed
    from torch ops on the same tensors: softmax, clamp, floor / ceil, index_add_, log_softmax, and autograd's backward;
  * C51Trainer.update() eager (host sync on the loss included, as a user calls it) and update_async() replayed as a hipGraph.
A run with no GPU fails; nothing here falls back.
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_c51_loss(logits, next_target, next_online, act, rew, flag, w, gamma_n, vmin, vmax):
    """The composition a user would write: -> (row_loss, dlogits of mean(w * row_loss))."""
    B, A, M = logits.shape
    z = torch.linspace(vmin, vmax, M, device=logits.device)
    dz = (vmax - vmin) / (M - 1)
    logits = logits.detach().requires_grad_(True)
    with torch.no_grad():
        astar = (torch.softmax(next_online, -1) * z).sum(-1).argmax(1)
        p = torch.softmax(next_target[torch.arange(B, device=logits.device), astar], -1)
        tz = (rew[:, None] + gamma_n * (1 - flag)[:, None] * z[None, :]).clamp(vmin, vmax)
        b = (tz - vmin) / dz
        lo, up = b.floor().long(), b.ceil().long()
        off = (torch.arange(B, device=logits.device) * M)[:, None]
        m = torch.zeros(B * M, device=logits.device)
        m.index_add_(0, (lo + off).view(-1), (p * torch.where(lo == up, torch.ones_like(b), up.float() - b)).view(-1))
        m.index_add_(0, (up + off).view(-1), (p * (b - lo.float())).view(-1))
        m = m.view(B, M)
    logp = torch.log_softmax(logits[torch.arange(B, device=logits.device), act.long()], -1)
    row_loss = -(m * logp).sum(-1)
    (w * row_loss).mean().backward()
    return row_loss.detach(), logits.grad


def timed(fn, iters, reps=7, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / iters)
    return {"best_us": round(min(us), 2), "median_us": round(statistics.median(us), 2), "iters": iters, "reps": reps}


def micro(out_path):
    from gymrl_amd import _lib, ops
    from gymrl_amd.c51_cartpole import C51Trainer, Config
    assert torch.cuda.is_available() and ops.device_ok(), "tools/micro_c51.py needs an MI355X"
    dev = torch.device("cuda:0")
    rows = []
    meta = {"device": torch.cuda.get_device_name(0), "lib_sha256": _lib.lib_sha256()[:16]}
    A, M, vmin, vmax, gamma = 2, 51, 0.0, 100.0, 0.99
    for B in (64, 256, 8192):
        g = torch.Generator(device=dev).manual_seed(B)
        logits, nt, no = (torch.randn(B, A, M, device=dev, generator=g) for _ in range(3))
        act = torch.randint(0, A, (B,), device=dev, generator=g).to(torch.int32)
        rew = torch.ones(B, device=dev)
        flag = (torch.rand(B, device=dev, generator=g) < 0.1).float()
        w = torch.rand(B, device=dev, generator=g) + 0.5
        sums = torch.zeros(1, dtype=torch.float64, device=dev)
        kern = lambda: ops.c51_loss(logits, nt, act, rew, flag, gamma, vmin, vmax, next_online=no, w=w, loss_sum=sums)   # noqa: E731
        comp = lambda: torch_c51_loss(logits, nt, no, act, rew, flag, w, gamma, vmin, vmax)                              # noqa: E731
        (rl_k, dl_k), (rl_t, dl_t) = kern(), comp()
        agree = {"row_loss_maxdiff": float((rl_k - rl_t).abs().max()), "dlogits_maxdiff": float((dl_k - dl_t).abs().max())}
        iters = 200 if B <= 256 else 100
        rows.append({"what": "c51_loss", "B": B, "A": A, "M": M, "kernel": timed(kern, iters), "torch_ops": timed(comp, iters), **agree, **meta})
        print(json.dumps(rows[-1]), flush=True)
    for B in (64, 256):
        cfg = Config()
        cfg.seed, cfg.num_envs, cfg.batch_size, cfg.memory_capacity = 0, 64, B, 65536
        tr = C51Trainer(cfg)
        tr.train(max_vector_steps=-(-B // 64) + 4)                      # fills the ring past one batch
        rows.append({"what": "C51Trainer.update", "B": B, "hidden_dim": cfg.hidden_dim, "eager_with_host_sync": timed(tr.update, 100),
                     "graphed_update_async": timed(tr.update_async, 200), **meta})
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


def learn(module, out_dir, max_vector_steps=None):
    import importlib
    import numpy as np
    mod = importlib.import_module(f"gymrl_amd.{module}")
    cfg = mod.Config()
    cfg.seed = 0
    tr = next(v for k, v in vars(mod).items() if k.endswith("Trainer") and k.startswith("C51"))(cfg)
    t0 = time.time()
    tr.train(max_vector_steps=max_vector_steps)
    torch.cuda.synchronize()
    wall = time.time() - t0
    ev = tr.eval(num_episodes=10)
    lines = [f"python -m gymrl_amd.{module} --seed 0   ({torch.cuda.get_device_name(0)})",
             f"Config: {json.dumps({k: v for k, v in vars(cfg).items() if isinstance(v, (int, float, str, bool, type(None)))}, sort_keys=True)}",
             f"max_vector_steps: {max_vector_steps}",
             f"train(): {wall:.1f} s wall, {tr.sample_count} env steps, {tr.optimizer.step_count} updates, {len(tr.episode_rewards)} of the last episodes kept",
             f"mean return of the last {len(tr.episode_rewards)} training episodes: {float(np.mean(tr.episode_rewards)) if tr.episode_rewards else float('nan'):.1f}"
             f" (max {max(tr.episode_rewards) if tr.episode_rewards else float('nan')})",
             f"greedy eval, 10 episodes: mean {float(np.mean(ev)):.1f}, min {min(ev):.0f}, max {max(ev):.0f}"]
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"{module}_learning.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    out_dir = os.environ.get("GYMRL_PROFILE_DIR", os.path.join(ROOT, "profiles"))
    if len(sys.argv) > 1 and sys.argv[1] == "learn":
        learn(sys.argv[2], out_dir, int(sys.argv[3]) if len(sys.argv) > 3 else None)
    else:
        micro(os.path.join(out_dir, "c51_micro.jsonl"))
