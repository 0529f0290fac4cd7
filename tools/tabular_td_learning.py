"""What the four tabular rules learn on CliffWalking-v0, as distributions over a population of runs (no number is promised; the
suite has no learning-outcome test).  For each rule at sarsa_cliffwalking.py's defaults, and again with a constant epsilon
(epsilon_start = epsilon_end = 0.1, the textbook setting): per run the mean return of its last 50 training episodes and the
return of its greedy evaluation, then the quantiles of both over the runs and the share of runs whose greedy path is the
13-step edge path, the 17-step path along the top row, another finished path, or none.  Needs an MI355X.

    python tools/tabular_td_learning.py [--num_runs 4096] [--out profiles/tabular_td_cliffwalking_learning.txt]
"""
import argparse
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def quantiles(x):
    import numpy as np
    q = np.percentile(x, [5, 25, 50, 75, 95])
    return f"mean {x.mean():8.2f}  std {x.std():7.2f}  p5 {q[0]:8.2f}  p25 {q[1]:8.2f}  p50 {q[2]:8.2f}  p75 {q[3]:8.2f}  p95 {q[4]:8.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_runs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tabular_td_cliffwalking_learning.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from gymrl_amd import ops, sarsa_cliffwalking
    if not (torch.cuda.is_available() and ops.device_ok()):
        raise SystemExit("tabular_td_learning.py runs on an MI355X: none found")
    lines = [f"CliffWalking-v0, {args.num_runs} runs per line (run r draws from stream r), 500 episodes of at most 200 steps, lr 0.1, gamma 0.9",
             "train: per run, the mean return of its last 50 training episodes (behaviour policy, exploration included)",
             "eval:  per run, the return of its greedy evaluation (deterministic env: every evaluation episode of a run is the same)",
             "paths: share of runs whose greedy path is the 13-step edge path / the 17-step top-row path / another finished one / unfinished at 200 steps", ""]
    summary = {}
    for label, fixed in (("module defaults: epsilon 0.95 -> 0.01, decay 300", None), ("constant epsilon 0.1", 0.1)):
        lines.append(label)
        for rule in ("qlearning", "sarsa", "expected_sarsa", "double_q"):
            cfg = sarsa_cliffwalking.Config()
            cfg.rule, cfg.num_runs = rule, args.num_runs
            if fixed is not None:
                cfg.epsilon_start = cfg.epsilon_end = fixed
            with contextlib.redirect_stdout(io.StringIO()):
                tr = sarsa_cliffwalking.TDTrainer(cfg)
                tr.train()
                returns, lengths, finished = tr._evaluate(1, cfg.max_steps)
            train = np.asarray(tr.episode_rewards, np.float64).reshape(args.num_runs, -1)[:, -50:].mean(axis=1)
            ev, n, fin = returns[:, 0], lengths[:, 0], finished[:, 0].astype(bool)
            edge, top = fin & (n == 13), fin & (n == 17)
            other = fin & ~edge & ~top
            summary[(fixed, rule)] = (train.mean(), ev.mean(), edge.mean(), top.mean())
            lines += [f"  {rule:15s} train  {quantiles(train)}", f"  {'':15s} eval   {quantiles(ev)}",
                      f"  {'':15s} paths  edge {edge.mean():6.1%}  top row {top.mean():6.1%}  other finished {other.mean():6.1%}  unfinished {(~fin).mean():6.1%}"]
        lines.append("")
    q, s = summary[(0.1, "qlearning")], summary[(0.1, "sarsa")]
    gap = s[0] > q[0] and q[2] > s[2]
    lines.append(f"Textbook gap at constant epsilon 0.1 (SARSA's training return above Q-learning's while Q-learning's greedy path is the edge more often): "
                 f"{'shows' if gap else 'does not show'}: training return {s[0]:.1f} (SARSA) vs {q[0]:.1f} (Q-learning), edge-path share "
                 f"{s[2]:.1%} vs {q[2]:.1%}.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
