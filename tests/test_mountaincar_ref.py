"""MountainCar-v0 and the rule policy as include/gymrl.h states them, pinned on the test reference (tests/mountaincar_ref.py) that
the kernels are compared with bit for bit: the policy against the reference script's own actions (tests/golden/
mountaincar_rule.npz), the dynamics against hand-computed values at their seams, whole episodes against recorded lengths.  No GPU."""
import math

import numpy as np

import mountaincar_ref as ref
from conftest import load_golden

# episode lengths of the rule from pos = linspace(-0.6, -0.4, 41), vel = 0, computed with math.cos in place of the device's cos
# (the smallest policy margin along those episodes, 1.75e-7, is nine orders above a last-bit difference in cos)
RULE_LENGTHS = [106, 106, 105, 105, 105, 105, 105, 105, 105, 105, 105, 105, 104, 104, 104, 104, 104, 104, 104, 103, 103, 145, 147,
                157, 166, 191, 112, 99, 96, 94, 92, 90, 89, 88, 87, 86, 85, 85, 84, 84, 83]
STARTS = np.linspace(-0.6, -0.4, 41)


def test_rule_equals_the_reference_scripts_actions():
    """Every golden point whose float64 distance to lb and ub is at least 1e-7 (the reference's expression may have run in
    float32); the excluded points are at most 0.01 % of the grid."""
    g = load_golden("mountaincar_rule")
    obs, want = g["obs"], g["action"]
    assert obs.dtype == np.float32 and obs.shape == (24000, 2) and int(g["n_uniform"]) == 20000
    act = ref.POLICIES["rule"]
    excluded, seen = 0, set()
    for (p, v), a in zip(obs.tolist(), want.tolist()):
        lb, ub = ref.bounds(p)
        if min(abs(v - lb), abs(v - ub)) < 1e-7:
            excluded += 1
            continue
        assert act(p, v) == a, (p, v, lb, ub)
        seen.add(a)
    assert seen == {0, 2}
    print(f"excluded {excluded} of {len(want)} points (NumPy {g['numpy_version']})")
    assert excluded <= 1e-4 * len(want)
    # the near-boundary part does straddle both boundaries: a wrong constant or a wrong min flips some of it
    near = obs[20000:].astype(np.float64)
    edges = np.array([ref.bounds(p) for p in near[:, 0].tolist()])
    d = np.abs(near[:, 1:2] - edges).min(axis=1)
    assert d.max() <= 1.1e-3 and (d >= 1e-7).mean() > 0.999
    assert 0.3 < (want[20000:] == 2).mean() < 0.7


def test_host_policy_rows_are_the_scalar_policy():
    g = load_golden("mountaincar_rule")
    obs = g["obs"][:500]
    got = ref.actions(obs, ref.POLICIES["rule"])
    assert got.dtype == np.int32 and got.tolist() == [ref.POLICIES["rule"](float(p), float(v)) for p, v in obs]


def test_reset_draw():
    draws = [ref.draw(42, ref.EVAL_STREAM0 + i) for i in range(2000)]
    pos = np.array([d[0] for d in draws])
    assert all(d[1] == 0.0 for d in draws)
    assert (pos >= -0.6).all() and (pos < -0.4).all() and len(set(pos.tolist())) == 2000
    assert abs(pos.mean() + 0.5) < 5 * 0.2 / math.sqrt(12 * 2000)            # five sigma of the mean of U(-0.6, -0.4)
    assert ref.draw(42, 7, 0) != ref.draw(42, 7, 1) and ref.draw(42, 7, 0) != ref.draw(43, 7, 0)


def test_rule_episode_lengths():
    eps = [ref.episode(float(p), 0.0) for p in STARTS]
    assert all(e["reached"] for e in eps)
    assert [e["len"] for e in eps] == RULE_LENGTHS
    assert [e["ret"] for e in eps] == [-float(n) for n in RULE_LENGTHS]
    # the det-cos episodes take the decisions of the libm-cos ones, with room to spare
    libm = [ref.episode(float(p), 0.0, cos=math.cos) for p in STARTS]
    assert [e["len"] for e in libm] == RULE_LENGTHS
    print("smallest policy margin:", min(e["margin"] for e in eps), "libm:", min(e["margin"] for e in libm))
    assert min(e["margin"] for e in eps) > 1e-9


def test_scripted_policies():
    """pump reaches the wall (from -0.6 and -0.5) and then the goal; pump-left reaches the wall and runs into the TimeLimit."""
    eps = [ref.episode(p, 0.0, ref.pump) for p in (-0.6, -0.5, -0.4)]
    assert [e["len"] for e in eps] == [151, 167, 86]
    assert all(e["reached"] for e in eps) and [e["hit_wall"] for e in eps] == [True, True, False]
    for p in (-0.6, -0.5, -0.4):
        e = ref.episode(p, 0.0, ref.pump_left)
        assert e["len"] == 200 and not e["reached"] and e["hit_wall"] and e["ret"] == -200.0


def test_wall_zeroes_the_velocity():
    c = ref.det_cos(3.0 * -1.19)
    assert abs(c - math.cos(-3.57)) < 1e-15
    vel = -0.05 + (-1.0 * 0.001 + c * (-0.0025))
    assert -0.07 < vel < 0.0 and -1.19 + vel < -1.2                           # moving left, through the wall
    assert ref.advance(-1.19, -0.05, 0) == (-1.2, 0.0, False)
    # at rest on the wall, pushing left: gravity (cos(-3.6) < 0) pulls to the right, the car leaves the wall
    pos, vel, _ = ref.advance(-1.2, 0.0, 0)
    assert vel == 0.0 + (-0.001 + ref.det_cos(3.0 * -1.2) * (-0.0025)) and vel > 0.0 and pos == -1.2 + vel


def test_speed_clamp():
    # the start the issue names: at pos = 0 gravity is at its strongest against the push, the speed falls and the clamp is idle
    assert ref.det_cos(0.0) == 1.0
    vel = 0.0699 + (1.0 * 0.001 + 1.0 * (-0.0025))
    assert vel < 0.07
    assert ref.advance(0.0, 0.0699, 2) == (0.0 + vel, vel, False)
    # where the slope helps (cos(3 pos) < 0) the same speed does run into the clamp, and the position into its own
    assert ref.det_cos(3.0 * 0.55) < 0.0
    assert 0.0699 + (0.001 + ref.det_cos(3.0 * 0.55) * (-0.0025)) > 0.07
    assert ref.advance(0.55, 0.0699, 2) == (0.6, 0.07, True)
    assert ref.advance(0.45, 0.0699, 2) == (0.45 + 0.07, 0.07, True)
    # and downwards
    assert -0.0699 + (-0.001 + ref.det_cos(3.0 * -0.5) * (-0.0025)) < -0.07
    assert ref.advance(-0.5, -0.0699, 0) == (-0.5 + -0.07, -0.07, False)


def test_past_the_goal_moving_left_is_not_terminal():
    pos, vel, terminated = ref.advance(0.55, -0.01, 0)
    assert vel == -0.01 + (-0.001 + ref.det_cos(3.0 * 0.55) * (-0.0025)) and vel < 0.0
    assert pos == 0.55 + vel and pos >= 0.5 and not terminated
    assert ref.advance(0.495, 0.01, 2)[2] and ref.advance(0.495, 0.01, 2)[0] >= 0.5      # the same place moving right is


def test_cap_cuts_an_episode_short():
    full = ref.episode(-0.5, 0.0)
    assert full["reached"] and full["len"] > 50
    cut = ref.episode(-0.5, 0.0, cap=50)
    assert cut["len"] == 50 and not cut["reached"] and cut["ret"] == -50.0
    ret, length, reached, final = ref.eval_population(42, ref.EVAL_STREAM0, 3, cap=50)
    assert (length == 50).all() and (reached == 0).all() and (ret == -50.0).all() and final.shape == (1, 3, 2)


def test_stepper_trace_auto_resets_into_the_next_draw():
    t = ref.stepper_trace(42, 5, ref.POLICIES["rule"], 420)
    first = ref.episode(*ref.draw(42, 5, 0))
    ends = np.flatnonzero(t["done"])
    assert len(ends) >= 2 and ends[0] == first["len"] - 1 and t["ep_len_out"][ends[0]] == first["len"]
    assert t["ep_ret_out"][ends[0]] == first["ret"] and t["terminated"][ends[0]] == 1
    assert t["obs"][ends[0]].tolist() == [ref.f32(ref.draw(42, 5, 1)[0]), 0.0]
    assert t["term_obs"][ends[0]].tolist() == [ref.f32(first["pos"]), ref.f32(first["vel"])]
    assert (t["rew"] == -1.0).all() and t["episode"][-1] == len(ends)
    left = ref.stepper_trace(42, 5, ref.pump_left, 420)
    assert np.flatnonzero(left["truncated"]).tolist() == [199, 399] and not left["terminated"].any()
    ab = ref.stepper_trace(42, 5, ref.pump_left, 120, abandon_cap=50)
    assert np.flatnonzero(ab["abandoned"]).tolist() == [49, 99] and not ab["done"].any()
    assert ab["ep_len_out"][49] == 50 and ab["ep_ret_out"][49] == -50.0 and ab["obs"][49].tolist() == [ref.f32(ref.draw(42, 5, 1)[0]), 0.0]
