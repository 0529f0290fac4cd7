"""Time of packing a population of PPO policies into the one-launch forward's weight layout (ops.LunarPolicyStack's buffer):
the ONE gymrl_mlp_pack_stack launch (csrc/pack_stack.hip) against the loop it replaced, restated here — gymrl_mlp_pack plus a
bias copy per layer and policy, 12 P launches for the six layers of ppo_lunarlander's ActorCritic.

For (population, hidden) in (8, 64), (256, 64), (4096, 64), (8, 256), (256, 256):

  * loop    the double loop over a zero-filled buffer that exists already (the allocation is not timed);
  * launch  ops.mlp_pack_stack on the same params and a buffer of the same shape;
  * refill  ops.LunarPolicyStack(..., out=stack): the launch with the constructor's host work (offsets, descriptor).

tools/micro_es.py's method: device events around a batch of back-to-back calls after a warm-up batch, per-call median and
minimum over `--repeats` batches; the loop's batch and the launch's alternate inside one repeat, so both see the same machine
state.  The two buffers are compared bit for bit before anything is timed.  Needs an MI355X; appends one JSON line per shape to
profiles/pack_stack_micro.jsonl.

    python tools/micro_pack_stack.py [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SHAPES = ((8, 64), (256, 64), (4096, 64), (8, 256), (256, 256))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_stack_micro.jsonl"))
    args = ap.parse_args()

    import torch
    from gymrl_amd import _lib, ops, ppo_net
    from gymrl_amd.flat import flatten_module
    from gymrl_amd.ppo_lunarlander import ActorCritic
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("micro_pack_stack.py measures on an MI355X: none found")
    dev = torch.device("cuda", torch.cuda.current_device())
    sha = _lib.lib_sha256()[:16]
    lines = []
    for P, hidden in SHAPES:
        torch.manual_seed(0)
        model = ActorCritic(8, 4, hidden)
        flat, _ = flatten_module(model, dev, order=ppo_net.LAYOUT)
        fused = model._act_net()
        mods = [m for m, _, _, _ in fused.stages]
        L, n = len(mods), flat.numel()
        params = flat.repeat(P, 1) + 0.1 * torch.randn(P, n, device=dev)
        stack = ops.LunarPolicyStack(fused, flat, params)
        offs = [(t.data_ptr() - flat.data_ptr()) // 4 for t in [m.weight for m in mods] + [m.bias for m in mods]]
        sizes = [int(_lib.lib().gymrl_mlp_packed_floats(*m.weight.shape)) for m in mods] + [(m.bias.numel() + 3) // 4 * 4 for m in mods]
        at = [sum(sizes[:k]) for k in range(2 * L)]
        layers = [(*m.weight.shape, offs[k], offs[L + k], at[k], at[L + k]) for k, m in enumerate(mods)]
        by_loop, by_launch = torch.zeros_like(stack.buffer), torch.zeros_like(stack.buffer)

        def loop():                       # the constructor's double loop as it was
            for p in range(P):
                for k, m in enumerate(mods):
                    W = params[p, offs[k]:offs[k] + m.weight.numel()].view(m.weight.shape)
                    ops.mlp_pack(W, by_loop[p, at[k]:at[k] + sizes[k]])
                    by_loop[p, at[L + k]:at[L + k] + m.bias.numel()] = params[p, offs[L + k]:offs[L + k] + m.bias.numel()]

        launch = lambda: ops.mlp_pack_stack(params, layers, by_launch)                                   # noqa: E731
        refill = lambda: ops.LunarPolicyStack(fused, flat, params, out=stack)                            # noqa: E731
        loop()
        launch()
        torch.cuda.synchronize()
        if not (torch.equal(by_loop.view(torch.int32), by_launch.view(torch.int32))
                and torch.equal(by_loop.view(torch.int32), stack.buffer.view(torch.int32))):
            raise SystemExit(f"P = {P}, hidden = {hidden}: the launch's buffer is not the loop's")
        fns = {"loop": (loop, max(1, 1024 // P)), "launch": (launch, 200 if P <= 256 else 20),
               "refill": (refill, 200 if P <= 256 else 20)}
        us = {k: [] for k in fns}
        for rep in range(args.repeats + 1):                      # repeat 0 warms every call of the shape up
            for name, (fn, batch) in fns.items():
                t = timed(torch, fn, batch)
                if rep:
                    us[name].append(t)
        med = {k: statistics.median(v) for k, v in us.items()}
        read = P * sum(m.weight.numel() + m.bias.numel() for m in mods) * 4
        written = P * stack.stride * 4
        line = {"what": "pack_stack", "population": P, "hidden": hidden, "layers": L, "n_params": n,
                "packed_floats_per_policy": stack.stride, "loop_launches": 2 * L * P, "bytes_read": read, "bytes_written": written}
        for k in fns:
            line[k + "_us_median"], line[k + "_us_min"] = round(med[k], 2), round(min(us[k]), 2)
            line[k + "_calls_per_repeat"] = fns[k][1]
        line.update({"loop_over_launch": round(med["loop"] / med["launch"], 2), "loop_over_refill": round(med["loop"] / med["refill"], 2),
                     "launch_gb_per_s": round((read + written) / med["launch"] * 1e-3, 2), "repeats": args.repeats,
                     "timer": "device events around a batch of back-to-back calls, the loop and the launch alternating per repeat",
                     "weight_reads": "strided by in_dim across lanes, not staged through LDS", "lib_sha256": sha})
        lines.append(line)
        print(json.dumps(line), flush=True)
        del stack, by_loop, by_launch, params
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    slower = [(ln["population"], ln["hidden"]) for ln in lines if ln["loop_over_launch"] < 1.0]
    if slower:
        raise SystemExit(f"the one launch is slower than the loop at {slower}")


if __name__ == "__main__":
    main()
