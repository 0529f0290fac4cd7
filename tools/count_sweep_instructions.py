#!/usr/bin/env python3
"""Instruction counts of the LunarLander velocity-sweep loops in a gfx950 assembly listing.

usage: hipcc --offload-arch=gfx950 <the Makefile's flags> --cuda-device-only -S env_lunar.hip -o env_lunar.s
       count_sweep_instructions.py env_lunar.s [kernel-name-substring]

A sweep loop is an innermost loop that holds the joint solve's `v_cmp_nge_f32 vcc` pair.  Per loop: the instructions
in the blocks the listing tags with the loop (the count of the longest path: a lane-divergent branch is walked, not skipped), how many of them
are wait-state nops, lane spills (v_readlane / v_writelane), exec-mask bookkeeping and branches, and whether the loop
holds the block solver (its four-case search is the only code with `v_cmp_le_f32 ... 0,` compares)."""
import re
import sys

lines = open(sys.argv[1]).read().split("\n")
want = sys.argv[2] if len(sys.argv) > 2 else ""
is_ins = re.compile(r"^\s+(v_|s_|ds_|global_|buffer_|flat_)")
kernel, loops, cur = "", {}, None          # loops: (kernel, header block) -> instruction lines of every block the listing tags with it
for i, ln in enumerate(lines):
    m = re.match(r"^(_Z\w+):", ln)
    if m:
        kernel, cur = m.group(1), None
    m = re.match(r"^\.L(BB\d+_\d+):(.*)", ln)
    if m:
        rest, j = m.group(2), i + 1
        while j < len(lines) and lines[j].lstrip().startswith(";"):        # a nested loop's header comment runs over several lines
            rest, j = rest + lines[j], j + 1
        t = re.search(r"in Loop: Header=(BB\d+_\d+)", rest)
        cur = (kernel, m.group(1)) if "This Inner Loop Header" in rest else ((kernel, t.group(1)) if t else None)
    elif cur and is_ins.match(ln):
        loops.setdefault(cur, []).append(ln)
for (kernel, head), ins in loops.items():
    if want not in kernel or sum("v_cmp_nge_f32 vcc" in x for x in ins) < 2:
        continue
    print(f"{kernel[:48]:48s} loop {head}: {len(ins):4d} instructions; s_nop {sum('s_nop' in x for x in ins)}, "
          f"lane spills {sum('v_readlane' in x or 'v_writelane' in x for x in ins)}, "
          f"exec/branch {sum(bool(re.search(r'saveexec|s_or_b64 exec|s_cbranch|s_branch|s_xor_b64|s_andn2', x)) for x in ins)}, "
          f"dpp {sum('quad_perm' in x for x in ins)}, cndmask {sum('v_cndmask' in x for x in ins)}, "
          f"block solver {'yes' if any(re.search(r'v_cmp_le_f32.* 0, v', x) for x in ins) else 'no'}")
