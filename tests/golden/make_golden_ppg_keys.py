#!/usr/bin/env python3
"""The reference networks' state_dict keys and shapes (ppg_rnn_lunarlander.py ActorCriticPPG(8, 4), ppo_rnn_lunarlander.py
ActorCritic(8, 4)), built on the CPU from the REFERENCE's own classes.  Runs only in the build container (needs the
reference checkout; make_golden.py's stub gym and loader).  Writes ppg_rnn_state_dict_keys.json.

    python tests/golden/make_golden_ppg_keys.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, load_ref  # noqa: E402


def main():
    ppg = load_ref("algorithms/ppg_rnn_lunarlander.py", "ref_ppg_rnn_keys")
    ppo = load_ref("algorithms/ppo_rnn_lunarlander.py", "ref_ppo_rnn_keys")
    out = {"ppg": [[k, list(v.shape)] for k, v in ppg.ActorCriticPPG(8, 4).state_dict().items()],
           "ppo": [[k, list(v.shape)] for k, v in ppo.ActorCritic(8, 4).state_dict().items()]}
    with open(os.path.join(OUT, "ppg_rnn_state_dict_keys.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
