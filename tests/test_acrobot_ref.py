"""The Acrobot-v1 restatement tests/acrobot_ref.py checked on its own, on the CPU: the RK4 step against an independent integrator,
wrap and clamp at their seams, the fixed trip count of the wrap, reward / termination / TimeLimit, and the pump policy the GPU
tests steer with.  What the kernels are compared with (tests/test_acrobot_gpu.py, tests/test_acrobot_net_eval_gpu.py) is this
file's subject."""
import itertools
import math

import numpy as np

import acrobot_ref as ref

SEED, ID0 = 42, 1 << 40


# ---- (1) the ODE and its RK4 step against scipy ---------------------------------------------------------------------------------
def _book_rhs(t, y, a):
    """gymnasium's AcrobotEnv._dsdt ("book"), written independently of acrobot_ref.deriv: the constants by name, libm."""
    m1 = m2 = l1 = 1.0
    lc1 = lc2 = 0.5
    I1 = I2 = 1.0
    g = 9.8
    th1, th2, w1, w2 = y
    d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * math.cos(th2)) + I1 + I2
    d2 = m2 * (lc2 ** 2 + l1 * lc2 * math.cos(th2)) + I2
    phi2 = m2 * lc2 * g * math.cos(th1 + th2 - math.pi / 2.0)
    phi1 = (-m2 * l1 * lc2 * w2 ** 2 * math.sin(th2) - 2 * m2 * l1 * lc2 * w2 * w1 * math.sin(th2)
            + (m1 * lc1 + m2 * l1) * g * math.cos(th1 - math.pi / 2) + phi2)
    dd2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * w1 ** 2 * math.sin(th2) - phi2) / (m2 * lc2 ** 2 + I2 - d2 ** 2 / d1)
    dd1 = -(d2 * dd2 + phi1) / d1
    return [w1, w2, dd1, dd2]


RK4_GRID_ERROR = 0.016549601914835566


def test_rk4_step_against_an_independent_integrator():
    """One advance before wrap and clamp against scipy's DOP853 at rtol = atol = 1e-12 on the same ODE, over 4 x 4 angles in
    [-3, 3], dth1 in {-2, 0, 2}, dth2 in {-4, 0, 4} and the three torques (432 states).

    Measured here: the largest difference of a component is 0.016549601914835566, at (th1, th2, dth1, dth2) = (-1, 1, 2, 4) under
    action 0 — the local error of RK4 at dt = 0.2, not rounding.  The assertion is ten times that.  It grows steeply with the
    speeds: 0.079 on the same grid with speeds (3, 6), 0.31 with (4, 8), which is about as fast as the pump policy's episodes get
    (7.4, 13.0 in their last steps), and hundreds at the corners of the clamp box (4 pi, 9 pi), where a step of 0.2 turns the
    second link by most of a revolution.  The grid stays where ten times the error still tells a wrong term of the ODE (a sign of
    the 14.7 cos term moves a velocity by about 2 in one step) from the method's error."""
    import scipy.integrate as scipy_integrate
    worst, where = 0.0, None
    for th1, th2, w1, w2, action in itertools.product(np.linspace(-3, 3, 4), np.linspace(-3, 3, 4), (-2.0, 0.0, 2.0),
                                                      (-4.0, 0.0, 4.0), (0, 1, 2)):
        y0 = (float(th1), float(th2), w1, w2)
        got = ref.rk4(y0, action)
        want = scipy_integrate.solve_ivp(_book_rhs, (0.0, 0.2), y0, args=(float(action - 1),), method="DOP853", rtol=1e-12,
                                         atol=1e-12).y[:, -1]
        err = max(abs(got[i] - want[i]) for i in range(4))
        if err > worst:
            worst, where = err, (y0, action)
    print(f"largest |RK4 - DOP853| over the grid: {worst!r} at {where}")
    assert worst <= 10.0 * RK4_GRID_ERROR
    assert worst >= 0.1 * RK4_GRID_ERROR                      # and it is the method's error that was measured, not nothing
    # det_sincos against libm inside the same step: rounding only
    y0 = (1.0, -1.0, 2.0, -4.0)
    assert max(abs(a - b) for a, b in zip(ref.rk4(y0, 2), ref.rk4(y0, 2, ref.libm_sincos))) < 1e-13


def test_deriv_is_the_independent_right_hand_side():
    for y in ((0.3, -0.2, 0.5, -1.0), (3.0, 0.0, 0.0, 0.0), (-2.5, 2.9, -4.0, 9.0), (0.0, 0.0, 0.0, 0.0)):
        for action in (0, 1, 2):
            got, want = ref.deriv(y, float(action - 1)), _book_rhs(0.0, y, float(action - 1))
            assert np.allclose(got, want, rtol=1e-13, atol=1e-13), (y, action)
    assert max(abs(v) for v in ref.deriv((0.0, 0.0, 0.0, 0.0), 0.0)) < 1e-14          # hanging at rest is the equilibrium


# ---- (2) wrap and clamp ---------------------------------------------------------------------------------------------------------
def test_wrap_and_clamp_at_their_seams():
    eps = 1e-9
    for x in (ref.PI + eps, -ref.PI - eps, 3 * ref.PI + eps, -3 * ref.PI - eps, 5.5 * ref.PI, -12.0):
        w, trips = ref.wrap(x)
        assert -ref.PI <= w <= ref.PI and trips >= 1 and abs(math.remainder(w - x, 2 * ref.PI)) < 1e-12, x
    assert ref.wrap(ref.PI) == (ref.PI, 0) and ref.wrap(-ref.PI) == (-ref.PI, 0) and ref.wrap(0.25) == (0.25, 0)
    assert ref.wrap(ref.PI + eps)[0] == (ref.PI + eps) - 2.0 * ref.PI                # gymnasium's subtraction, not a remainder
    # beyond the trip count an angle stays outside, as the header says: 8 trips undo 16 pi
    assert ref.wrap(17.5 * ref.PI)[0] > ref.PI and ref.wrap(16.5 * ref.PI)[0] <= ref.PI
    assert ref.clamp(ref.MAX_VEL_1 + eps, ref.MAX_VEL_1) == 4.0 * ref.PI and ref.clamp(-ref.MAX_VEL_1 - eps, ref.MAX_VEL_1) == -4.0 * ref.PI
    assert ref.clamp(ref.MAX_VEL_2 + eps, ref.MAX_VEL_2) == 9.0 * ref.PI and ref.clamp(-30.0, ref.MAX_VEL_2) == -9.0 * ref.PI
    assert ref.clamp(12.5, ref.MAX_VEL_2) == 12.5 and ref.clamp(12.5, ref.MAX_VEL_1) == 12.5
    # through advance: an angle just below pi moving up comes out wrapped, a velocity driven past its bound comes out ON it
    y, _ = ref.advance((ref.PI - 1e-3, 0.0, 1.0, 0.0), 1)
    assert -ref.PI <= y[0] < -2.5 and ref.rk4((ref.PI - 1e-3, 0.0, 1.0, 0.0), 1)[0] > ref.PI
    y, _ = ref.advance((-ref.PI + 1e-3, 0.0, -1.0, 0.0), 1)
    assert 2.5 < y[0] <= ref.PI
    y, _ = ref.advance((0.0, ref.PI - 1e-3, 0.0, 2.0), 1)
    assert -ref.PI <= y[1] < -2.5
    hit = {}
    for th1, th2 in itertools.product(np.linspace(-3, 3, 7), repeat=2):
        for w1, w2 in ((ref.MAX_VEL_1, ref.MAX_VEL_2), (-ref.MAX_VEL_1, -ref.MAX_VEL_2), (ref.MAX_VEL_1, -ref.MAX_VEL_2)):
            raw = ref.rk4((th1, th2, w1, w2), 2)
            y, _ = ref.advance((th1, th2, w1, w2), 2)
            for k, bound in ((2, ref.MAX_VEL_1), (3, ref.MAX_VEL_2)):
                if abs(raw[k]) > bound:
                    assert y[k] == math.copysign(bound, raw[k])
                    hit[k] = True
                else:
                    assert y[k] == raw[k]
    assert hit == {2: True, 3: True}


def test_the_wrap_never_needs_its_trip_count_inside_the_velocity_box():
    """A 7 x 7 x 5 x 5 grid over [-pi, pi]^2 x the clamped velocity box and 25 x 25 angles at the box's four corners, where the
    angles move furthest, under the three torques: an angle moves by less than 9 pi in a step (8.66 pi at (4 pi, 9 pi) and its
    mirror image; a search over ten million random states of the box found no more) and its wrap takes at most five trips.  The
    header's eight are never reached."""
    box = itertools.product(np.linspace(-ref.PI, ref.PI, 7), np.linspace(-ref.PI, ref.PI, 7), np.linspace(-ref.MAX_VEL_1, ref.MAX_VEL_1, 5),
                            np.linspace(-ref.MAX_VEL_2, ref.MAX_VEL_2, 5))
    corners = itertools.product(np.linspace(-ref.PI, ref.PI, 25), np.linspace(-ref.PI, ref.PI, 25), (-ref.MAX_VEL_1, ref.MAX_VEL_1),
                                (-ref.MAX_VEL_2, ref.MAX_VEL_2))
    worst_move, worst_trips = 0.0, 0
    for th1, th2, w1, w2 in itertools.chain(box, corners):
        for action in (0, 1, 2):
            y = ref.rk4((th1, th2, w1, w2), action)
            for k, th in ((0, th1), (1, th2)):
                w, trips = ref.wrap(y[k])
                assert -ref.PI <= w <= ref.PI
                worst_move, worst_trips = max(worst_move, abs(y[k] - th)), max(worst_trips, trips)
    print(f"largest angle move {worst_move / ref.PI:.3f} pi, most trips {worst_trips}")
    assert 4 <= worst_trips <= 5 < ref.WRAP_TRIPS and 8.0 * ref.PI < worst_move < 9.0 * ref.PI


# ---- (3) reward, termination, episode ends --------------------------------------------------------------------------------------
def test_reward_termination_and_episode_ends():
    # the tip already near the top: terminated on the first step, reward 0
    out = ref.episode((3.0, 0.0, 0.0, 0.0), ref.idle)
    assert (out["ret"], out["len"], out["terminated"]) == (0.0, 1, True)
    assert ref.height_reached(out["state"][0], out["state"][1])
    # hanging: never under torque 0 — truncated at exactly 500 with -500
    start = ref.draw(SEED, ID0)
    assert all(-0.1 <= v < 0.1 for v in start)
    out = ref.episode(start, ref.idle)
    assert (out["ret"], out["len"], out["terminated"]) == (-500.0, 500, False)
    out = ref.episode(start, ref.idle, cap=7)
    assert (out["ret"], out["len"], out["terminated"]) == (-7.0, 7, False)
    # the observation
    o = ref.obs_of((0.5, -0.25, 1.5, -2.5))
    assert o.dtype == np.float32 and np.allclose(o, [math.cos(0.5), math.sin(0.5), math.cos(0.25), -math.sin(0.25), 1.5, -2.5], atol=1e-7)


def test_the_pump_policy_ends_episodes_before_the_time_limit():
    """acrobot_ref.pump — torque against the sign of dth1 — on the 16 reset draws the GPU tests use."""
    eps = [ref.episode(ref.draw(SEED, ID0 + e), ref.pump) for e in range(16)]
    lengths = [o["len"] for o in eps]
    assert lengths == [76, 78, 79, 97, 82, 79, 82, 77, 74, 127, 77, 76, 99, 95, 79, 88]
    assert all(o["terminated"] and o["ret"] == -(o["len"] - 1.0) for o in eps)
    # the opposite sign pumps nothing
    anti = ref.episode(ref.draw(SEED, ID0), lambda o, t: 2 if o[4] >= 0 else 0)
    assert anti["len"] == 500 and not anti["terminated"]


def test_stepper_trace_auto_resets_and_abandons():
    tr = ref.stepper_trace(SEED, 0, ref.pump, 40, start=(3.0, 0.0, 0.0, 0.0))
    assert tr["terminated"][0] == 1 and tr["done"][0] == 1 and tr["rew"][0] == 0.0 and tr["ep_len_out"][0] == 1 and tr["ep_ret_out"][0] == 0.0
    assert tr["episode"][0] == 1 and tr["ep_len"][0] == 0 and tuple(tr["state"][0]) == ref.draw(SEED, 0, 1)
    assert np.array_equal(tr["obs"][0], ref.obs_of(ref.draw(SEED, 0, 1))) and not np.array_equal(tr["obs"][0], tr["term_obs"][0])
    assert (tr["rew"][1:] == -1.0).all() and tr["ep_len"][-1] == 39
    ab = ref.stepper_trace(SEED, 3, ref.cycle, 40, abandon_cap=7)
    assert ab["abandoned"].sum() == 5 and not ab["done"].any() and (ab["ep_len_out"][ab["abandoned"] == 1] == 7).all()
    assert ab["action"].tolist() == [t % 3 for t in range(40)]
    one = ref.stepper_trace(SEED, 3, ref.cycle, 5, abandon_cap=1)
    assert one["abandoned"].all() and one["episode"].tolist() == [1, 2, 3, 4, 5]
    both = ref.stepper_traces(SEED, 0, 2, ref.idle, 3, starts={1: (3.0, 0.0, 0.0, 0.0)})
    assert both["obs"].shape == (3, 2, 6) and both["obs0"].shape == (2, 6) and both["terminated"][0].tolist() == [0, 1]
