#!/usr/bin/env python3
"""Golden actions of the rule-based MountainCar-v0 baseline, from the REFERENCE's own Python (algorithms/mountaincar_baseline.py).

Needs a checkout of the reference; `gymnasium` is stubbed here (the module touches gym only inside __init__ / run_episode, which
are not called).  RuleBasedAgent.select_action(None, obs) is called on float32 observations, as env.step() hands them out:
  * 20 000 points uniform over [-1.2, 0.6] x [-0.07, 0.07];
  * 4 000 points at random positions with the velocity 1e-6 .. 1e-3 (log-uniform) above or below lb or ub there, which make a
    wrong constant or a wrong min visible.
Recorded: obs f32[K, 2], action i8[K], the NumPy version the reference's expression ran under.  No reference source is copied:
the fixture is data.  Writes mountaincar_rule.npz.

    python tests/golden/make_golden_mountaincar.py <reference checkout>
"""
import importlib.util
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
import mountaincar_ref as ref  # noqa: E402

N_UNIFORM, N_NEAR, SEED = 20000, 4000, 20


def load_agent(ref_root):
    sys.modules.setdefault("gymnasium", types.ModuleType("gymnasium"))
    spec = importlib.util.spec_from_file_location("ref_mountaincar_baseline", os.path.join(ref_root, "algorithms", "mountaincar_baseline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.RuleBasedAgent


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    agent = load_agent(sys.argv[1])
    rng = np.random.default_rng(SEED)
    uniform = np.stack([rng.uniform(-1.2, 0.6, N_UNIFORM), rng.uniform(-0.07, 0.07, N_UNIFORM)], axis=1)
    near = np.empty((N_NEAR, 2))
    for row in near:
        p = float(np.float32(rng.uniform(-1.2, 0.6)))
        edge = ref.bounds(p)[int(rng.integers(0, 2))]
        delta = 10.0 ** rng.uniform(-6.0, -3.0)
        row[:] = p, edge + (delta if rng.integers(0, 2) else -delta)
    obs = np.concatenate([uniform, near]).astype(np.float32)
    action = np.array([agent.select_action(None, o) for o in obs], np.int8)
    path = os.path.join(OUT, "mountaincar_rule.npz")
    np.savez_compressed(path, obs=obs, action=action, n_uniform=np.int64(N_UNIFORM), numpy_version=np.array(np.__version__))
    print(f"wrote {path}  ({os.path.getsize(path)} B); actions: {np.bincount(action, minlength=3).tolist()}")


if __name__ == "__main__":
    main()
