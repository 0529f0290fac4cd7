#!/usr/bin/env python3
"""gpurun_out/<ledger>.jsonl (written by tests/conftest.py::bounded under GYMRL_TOL_LEDGER) -> profiles/rNN_trace_tolerances.json:
the observed drift of every multi-step trace bound of an MI355X run next to the bound the test enforces.
usage: python tools/ledger_to_profile.py <ledger.jsonl> <out.json> [<name prefix> [<what>]]
With a name prefix only the bounds whose name starts with it are kept (profiles/onpolicy_edge_tolerances.json: "onpolicy hip"),
and <what> replaces the description written into the file."""
import json
import subprocess
import sys

prefix = sys.argv[3] if len(sys.argv) > 3 else ""
rows = [r for r in (json.loads(l) for l in open(sys.argv[1]) if l.strip()) if r["name"].startswith(prefix)]
best = {}
for r in rows:
    k = r["name"]
    if k not in best or r["observed"] > best[k]["observed"]:
        best[k] = r
try:
    head = subprocess.check_output(["git", "rev-parse", "HEAD"], text=True).strip()
except Exception:
    head = None
what = sys.argv[4] if len(sys.argv) > 4 else None
out = {"what": what or "max observed error per trace bound (|got - want| / max(1, |want|) unless the test says otherwise) on one MI355X run of "
               "pytest -m gpu with GYMRL_TOL_LEDGER set; fixtures are the reference's own train() / update() runs (tests/golden/make_golden.py)",
       "git_head": head, "bounds": sorted(best.values(), key=lambda r: r["name"])}
json.dump(out, open(sys.argv[2], "w"), indent=1)
print(f"{len(best)} bounds; worst observed / bound = {max(r['observed'] / r['bound'] for r in best.values()):.3f}")
