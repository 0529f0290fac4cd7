"""Timings of the quantile-regression (QR-DQN) head on an MI355X -> profiles/qrdqn_micro.jsonl, and the learning runs of its
two trainers.

    python tools/micro_qrdqn.py                                  # the micro-benchmarks below
    python tools/micro_qrdqn.py learn qrdqn_cartpole 60000       # train() at the module's defaults, seed 0, capped at 60000
    python tools/micro_qrdqn.py learn qrdqn_per_cartpole 60000   #   vector steps -> profiles/<module>_learning.txt

Micro-benchmarks (device events around `iters` back-to-back calls after a warm-up, best and median of `reps` windows, `iters`
chosen per side so that a window lasts a fraction of a second.  Each figure is the time of the call as Python issues it —
launches and host dispatch included — not kernel time):
  * ops.qr_loss at B in {64, 256, 1024, 8192}, A = 2, N = 51 (double-Q, weighted, with the loss sum) against the same loss
    composed from torch ops on the same tensors: the [B, N, N] broadcast, huber_loss, the indicator weights, and autograd's
    backward; the two sides' windows alternate;
  * QRDQNTrainer.update() eager (host sync on the loss included, as a user calls it) and update_async() replayed as a hipGraph,
    at B = 64, on ONE trainer: all the eager windows first, then the graph's (not alternated: the graph is captured once).
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


def torch_qr_loss(quant, next_target, next_online, act, rew, flag, w, gamma_n, kappa):
    """The composition a user would write: -> (row_loss, dquant of mean(w * row_loss))."""
    B, A, N = quant.shape
    rows = torch.arange(B, device=quant.device)
    tau = (2.0 * torch.arange(N, device=quant.device) + 1.0) / (2.0 * N)
    quant = quant.detach().requires_grad_(True)
    with torch.no_grad():
        astar = next_online.mean(-1).argmax(1)
        T = rew[:, None] + gamma_n * (1 - flag)[:, None] * next_target[rows, astar]
    theta = quant[rows, act.long()]
    u = T[:, None, :] - theta[:, :, None]
    hub = torch.nn.functional.huber_loss(theta[:, :, None].expand(B, N, N), T[:, None, :].expand(B, N, N), reduction="none", delta=kappa)
    row_loss = ((tau[None, :, None] - (u.detach() < 0).float()).abs() * hub / kappa).sum(2).mean(1)
    (w * row_loss).mean().backward()
    return row_loss.detach(), quant.grad


def timed_pair(fns, iters, reps=7, warmup=20):
    """Each of fns timed over `reps` windows of its own iters[k] calls, the windows of the fns alternating."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters[k]):
                fn()
            b.record()
            torch.cuda.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / iters[k])
    return [{"best_us": round(min(v), 2), "median_us": round(statistics.median(v), 2), "iters": n, "reps": reps} for v, n in zip(us, iters)]


def micro(out_path):
    from gymrl_amd import _lib, ops
    from gymrl_amd.qrdqn_cartpole import Config, QRDQNTrainer
    assert torch.cuda.is_available() and ops.device_ok(), "tools/micro_qrdqn.py needs an MI355X"
    dev = torch.device("cuda:0")
    rows = []
    meta = {"device": torch.cuda.get_device_name(0), "lib_sha256": _lib.lib_sha256()[:16]}
    A, N, kappa, gamma = 2, 51, 1.0, 0.99
    for B in (64, 256, 1024, 8192):
        g = torch.Generator(device=dev).manual_seed(B)
        quant, nt, no = (torch.randn(B, A, N, device=dev, generator=g) for _ in range(3))
        act = torch.randint(0, A, (B,), device=dev, generator=g).to(torch.int32)
        rew = torch.ones(B, device=dev)
        flag = (torch.rand(B, device=dev, generator=g) < 0.1).float()
        w = torch.rand(B, device=dev, generator=g) + 0.5
        sums = torch.zeros(1, dtype=torch.float64, device=dev)
        kern = lambda: ops.qr_loss(quant, nt, act, rew, flag, gamma, kappa, next_online=no, w=w, loss_sum=sums)   # noqa: E731
        comp = lambda: torch_qr_loss(quant, nt, no, act, rew, flag, w, gamma, kappa)                              # noqa: E731
        (rl_k, dq_k), (rl_t, dq_t) = kern(), comp()
        agree = {"row_loss_maxdiff": float((rl_k - rl_t).abs().max()), "dquant_maxdiff": float((dq_k - dq_t).abs().max())}
        tk, tt = timed_pair((kern, comp), (10000, 1000))         # windows of about 0.2 s and 0.3 - 0.6 s
        rows.append({"what": "qr_loss", "B": B, "A": A, "N": N, "kappa": kappa, "kernel": tk, "torch_ops": tt, **agree, **meta})
        print(json.dumps(rows[-1]), flush=True)
    cfg = Config()
    cfg.seed, cfg.num_envs, cfg.batch_size, cfg.memory_capacity = 0, 64, 64, 65536
    tr = QRDQNTrainer(cfg)
    tr.train(max_vector_steps=5)                                        # fills the ring past one batch
    (te,), (tg,) = timed_pair((tr.update,), (1000,)), timed_pair((tr.update_async,), (4000,))      # one trainer: eager first, then its graph
    rows.append({"what": "QRDQNTrainer.update", "B": 64, "hidden_dim": cfg.hidden_dim, "eager_with_host_sync": te, "graphed_update_async": tg, **meta})
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
    tr = next(v for k, v in vars(mod).items() if k.endswith("Trainer") and k.startswith("QRDQN"))(cfg)
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
        micro(os.path.join(out_dir, "qrdqn_micro.jsonl"))
