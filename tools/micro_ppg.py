"""Micro-benchmark of the PPG-RNN trainer's pieces (one MI355X; every figure is the median of --reps timed runs):
  (a) act:    gymrl_mlprnn_act (one launch) against the torch-layer composition of the same step (PSCN, rnn_linear,
              nn.GRU step, heads, softmax, + gymrl_categorical_sample for the draw), eager and graph-captured,
              at N in {1, 16, 256, 4096}: microseconds per vector step
  (b) update: one PPGTrainer.update() at the reference config (batch_size 4, epochs 10 + aux_epochs 6, G = 1) on
              LunarLander episodes, split into the GRU kernels (gru_seq fwd + bwd of every optimiser step), the L5 / L6
              launches, and the rest (library GEMMs, autograd, gathers, Adam) = total - GRU - losses
  (c) rounds: collection throughput (acting + env + normalisation + compaction, no update) in episodes/s at
              N in {1, 64, 1024} over --rounds rounds
Prints one JSON line per measurement (profiles/ppg_micro.jsonl)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gymrl_amd import ops  # noqa: E402
from gymrl_amd import ppg_rnn_lunarlander as ppg  # noqa: E402
from gymrl_amd.graphs import capture  # noqa: E402

BOX = f"1x MI355X (gfx950), torch {torch.__version__}"


def median_ms(fn, reps, inner=1):
    out = []
    for _ in range(reps):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        z.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(z) / inner)
    return float(np.median(out))


def torch_step(net, x, h):
    feat = net.fc_head(x)
    out_rnn, hn = net.rnn.rnn(feat.unsqueeze(1), h.unsqueeze(0))
    out = torch.cat([net.rnn.rnn_linear(feat), out_rnn[:, 0]], -1)
    logits, value = net.actor_fc(out), net.critic_fc(out)
    torch.softmax(logits, -1)
    act, logp, _, _ = ops.categorical_sample(logits.contiguous(), value=value.reshape(-1).contiguous())
    return act, logp, hn[0]


def bench_act(reps, inner):
    net = ppg.ActorCriticPPG(8, 4).cuda()
    P = ops.mlprnn_params(net)
    for N in (1, 16, 256, 4096):
        x, h = torch.randn(N, 8, device="cuda"), torch.randn(N, 64, device="cuda")
        hk = h.clone()
        k = median_ms(lambda: ops.mlprnn_act(x, hk, P, 4, h_out=hk), reps, inner)
        with torch.no_grad():
            e = median_ms(lambda: torch_step(net, x, h), reps, inner)
            torch_step(net, x, h)
            g = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                torch_step(net, x, h)
            torch.cuda.current_stream().wait_stream(s)
            with capture(g):
                torch_step(net, x, h)
            gr = median_ms(g.replay, reps, inner)
        print(json.dumps({"what": "act", "N": N, "kernel_us": round(1000 * k, 2), "torch_eager_us": round(1000 * e, 2),
                          "torch_graph_us": round(1000 * gr, 2), "reps": reps, "calls_per_rep": inner, "box": BOX}),
              flush=True)


def _trainer(N, B, G, epochs, aux_epochs, path):
    cfg = ppg.Config()
    cfg.num_envs, cfg.batch_size, cfg.episodes_per_minibatch = N, B, G
    cfg.epochs, cfg.aux_epochs, cfg.seed, cfg.save_path = epochs, aux_epochs, 0, path
    return ppg.PPGTrainer(cfg)


def bench_update(reps, path):
    tr = _trainer(4, 4, 1, 10, 6, path)
    tr.collect_round()
    batch = [dict(c) for c in tr._batch]
    tot, gru, loss = [], [], []
    for _ in range(reps):
        tr._batch = [dict(c) for c in batch]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.update()
        torch.cuda.synchronize()
        tot.append(1000 * (time.perf_counter() - t0))
        b = tr.last_sample
        # the same launches in isolation, one per optimiser step (64 steps of one episode each)
        eps = [ppg._Episodes([n], "cuda") for n in b["lengths"]]
        gis = [torch.randn(e.T, 1, 192, device="cuda") for e in eps]
        W, bb = tr.net.rnn.rnn.weight_hh_l0.detach(), tr.net.rnn.rnn.bias_hh_l0.detach()

        def grus():
            for _ in range(16):
                for e, gi in zip(eps, gis):
                    hs, _ = ops.gru_seq_fwd(gi, W, bb, e.lengths)
                    ops.gru_seq_bwd(gi, W, bb, hs, e.lengths, d_hseq=hs, need_dh0=False)
        parts = []
        for e in range(len(b["lengths"])):
            o0, o1 = b["offsets"][e], b["offsets"][e + 1]
            parts.append((torch.randn(o1 - o0, 4, device="cuda"), torch.randn(o1 - o0, device="cuda"),
                          *(b[k][o0:o1] for k in ("act", "logp", "adv", "v_target")), [0, o1 - o0]))

        def losses():
            for _ in range(10):
                for lg, v, a, lp, ad, vt, off in parts:
                    ops.ppg_policy_loss_fwd_bwd(lg, v, a, lp, ad, vt, off, 0.2, 3.0, 0.5, 0.01)
            for _ in range(6):
                for lg, v, a, lp, ad, vt, off in parts:
                    ops.ppg_aux_loss_fwd_bwd(lg, v, a, lp, vt, off, 1.0)
        gru.append(median_ms(grus, 1))
        loss.append(median_ms(losses, 1))
    T, Gm, Lm = float(np.median(tot)), float(np.median(gru)), float(np.median(loss))
    print(json.dumps({"what": "update", "config": "batch_size 4, epochs 10 + aux_epochs 6, G 1 (64 optimiser steps)",
                      "episode_steps": int(sum(tr.last_sample["lengths"])), "total_ms": round(T, 2), "gru_ms": round(Gm, 2),
                      "losses_ms": round(Lm, 2), "rest_ms": round(T - Gm - Lm, 2), "reps": reps, "box": BOX}), flush=True)


def bench_rounds(rounds, path):
    for N in (1, 64, 1024):
        tr = _trainer(N, N, 1, 1, 1, path)
        tr.collect_round()
        tr._batch = []
        per = []
        steps = 0
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, lens = tr.collect_round()
            torch.cuda.synchronize()
            per.append(time.perf_counter() - t0)
            steps += sum(lens)
            tr._batch = []
        s = float(np.median(per))
        print(json.dumps({"what": "rounds", "N": N, "rounds": rounds, "round_s_median": round(s, 4),
                          "episodes_per_s": round(N / s, 1), "env_steps_per_s": round(steps / sum(per), 1), "box": BOX}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="act,update,rounds")
    args = ap.parse_args()
    path = os.path.join(tempfile.mkdtemp(), "ck.pth")
    only = args.only.split(",")
    if "act" in only:
        bench_act(args.reps, args.inner)
    if "update" in only:
        bench_update(args.reps, path)
    if "rounds" in only:
        bench_rounds(args.rounds, path)


if __name__ == "__main__":
    main()
