"""CPU: the float32 restatement of the QR-DQN kernels (tests/qrdqn_ref.py: qr_q / qr_loss, the bits the GPU tests demand) against
the float64 textbook loss (one [B, N, N] broadcast), the textbook against float64 torch autograd, and the restatement's own
invariants.

The bounds, derived before any run (u = 2^-24, the float32 unit roundoff; per row: G = max_j |gamma_n (1 - flag) nt_j|,
Th = max_i |theta_i|, S = |rew| + G + Th >= |u_ij|; flag is 0 or 1, so 1 - flag is exact):

  u_ij   (float)gamma_n carries u, g * nt_j one more, rew + . one of |T_j| <= |rew| + G:  |dT_j| <= 3 u (|rew| + G);  T_j - theta_i
         rounds once (u |u_ij| <= u S):
             |du_ij| <= 4 u S                                                                                      = DELTA
  wt     tau_i is one division (<= u), 1 - tau_i one subtraction:  |d wt| <= 2 u, wt in (0, 1)
  loss   f(u) = wt(u) H(u) / kappa is continuous (H(0) = 0 where wt jumps) with |f'| = wt |clamp(u)| / kappa <= 1, so DELTA costs
         at most DELTA per term, a sign flip of a tiny u included: N^2 terms over N is N DELTA.  Roundings, all relative to the
         terms' own size: H <= 2 u (one in the quadratic branch, two in the linear), wt 2 u, wt * H u, the serial sum (N - 1) u,
         / kappa and / N 2 u, the 64-slot tree 6 u:
             |d row_loss| <= u (4 N S + (N + 12) row_loss)                                                         = TOL_LOSS
         (proportional to the row's magnitude: the 1e30 row is held relatively)
  grad   t(u) = wt(u) clamp(u, -kappa, kappa) / kappa is nondecreasing with range inside [-(1 - tau), tau], 1 / kappa-Lipschitz
         inside |u| <= kappa and CONSTANT beyond: a pair with |u_ij| > kappa + DELTA keeps its term exactly, any other moves by at
         most min(DELTA / kappa, 1).  near_i = #{j: |u_ij| <= kappa + DELTA}.  Roundings with |t| <= 1: wt 2 u, the product u,
         the serial sum (N - 1) u, / kappa and / N 2 u, and 1 / B, w * ., the last product 3 u:
             |d (B dquant_i / w)| <= near_i min(DELTA / kappa, 1) / N + u (N + 7)                                  = TOL_GRAD
  q      the 64-slot tree over N values (6 u) and one division:  7 u max_i |quant_i|                               = TOL_Q

profiles/qrdqn_tolerances.json records these expressions and the maxima this test measured (GYMRL_QRDQN_TOL_OUT=<file> rewrites it).
"""
import json
import os

import numpy as np
import pytest

import qrdqn_ref
from det_math_ref import bits

U = 2.0 ** -24
SHAPES = [(37, 1, 1, 1.0), (37, 2, 33, 1.0), (37, 2, 51, 1.0), (37, 3, 51, 2.0), (37, 8, 64, 0.5)]
VARIANTS = ["plain", "double_q_weighted", "gamma0"]
BOUNDS = {"delta": "4 u S, S = |rew| + max_j |gamma_n (1 - flag) nt_j| + max_i |theta_i|",
          "row_loss": "u (4 N S + (N + 12) row_loss)",
          "grad": "near_i min(delta / kappa, 1) / N + u (N + 7), near_i = #{j: |u_ij| <= kappa + delta}",
          "q": "7 u max_i |quant_i|"}
_measured = {}


def variant_of(c, variant):
    c = dict(c)
    if variant == "plain":
        c["next_online"] = c["w"] = None
    if variant == "gamma0":
        c["gamma_n"] = 0.0
    return c


@pytest.fixture(scope="module", autouse=True)
def ledger():
    yield
    path = os.environ.get("GYMRL_QRDQN_TOL_OUT")
    if path and _measured:
        doc = {"unit": "u = 2^-24; per row of N quantiles; grad is B dquant / w on the taken action",
               "bounds": BOUNDS, "derivation": "tests/test_qrdqn_ref.py, module docstring", "measured_max_over_bound": _measured}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


@pytest.mark.parametrize("B,A,N,kappa", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_float32_restatement_is_within_the_derived_bounds_of_the_textbook(B, A, N, kappa, variant):
    c = variant_of(qrdqn_ref.case(B, A, N, kappa), variant)
    got, want = qrdqn_ref.qr_loss(**c), qrdqn_ref.textbook_loss(**c)
    assert np.array_equal(got.astar, want.astar)
    rows = np.arange(B)
    S = np.abs(c["rew"].astype(np.float64)) + np.abs(want.gnt).max(axis=1) + np.abs(want.theta).max(axis=1)
    delta = 4 * U * S
    tol_loss = U * (4 * N * S + (N + 12) * want.row_loss)
    near = (np.abs(want.u) <= kappa + delta[:, None, None]).sum(axis=2)
    tol_grad = near * np.minimum(delta / kappa, 1.0)[:, None] / N + U * (N + 7)
    wb = np.ones(B) if c["w"] is None else c["w"].astype(np.float64)
    live = wb > 0
    scale = (B / wb[live])[:, None]
    dg = np.abs(got.dquant[rows, c["act"]][live].astype(np.float64) - want.dquant[rows, c["act"]][live]) * scale
    q32, _ = qrdqn_ref.qr_q(c["quant"])
    q64, _ = qrdqn_ref.textbook_q(c["quant"])
    err = {"row_loss": (np.abs(got.row_loss - want.row_loss) / tol_loss)[S > 0].max(),
           "grad": (dg / tol_grad[live]).max(),
           "q": (np.abs(q32 - q64) / (7 * U * np.abs(c["quant"].astype(np.float64)).max(axis=2)).clip(1e-300)).max()}
    key = f"B{B}_A{A}_N{N}_kappa{kappa:g}_{variant}"
    _measured[key] = {n: float(f"{v:.4g}") for n, v in err.items()}
    print(key, _measured[key])
    assert all(v <= 1.0 for v in err.values()), err
    assert np.isfinite(got.row_loss).all() and np.isfinite(got.dquant).all()      # the 1e30 row included: no overflow reaches an output
    # what the kernel writes outside the taken action, and for a zero weight: exact zeros
    other = np.ones((B, A), bool)
    other[rows, c["act"]] = False
    assert not got.dquant[other].any() and not got.dquant[~live].any() and (~live).sum() == (0 if c["w"] is None else 4)


def test_tolerance_file_states_these_bounds():
    from conftest import ROOT
    doc = json.load(open(os.path.join(ROOT, "profiles", "qrdqn_tolerances.json")))
    assert doc["bounds"] == BOUNDS
    cases = doc["measured_max_over_bound"]
    assert len(cases) == len(SHAPES) * len(VARIANTS) and all(0.0 <= v <= 1.0 for case in cases.values() for v in case.values())


@pytest.mark.parametrize("B,A,N,kappa", SHAPES)
def test_textbook_gradient_is_autograd_of_huber_loss(B, A, N, kappa):
    """float64 torch: F.huber_loss(theta_i, T_j, delta = kappa) weighted by |tau_i - 1{u < 0}| / kappa, summed over j, averaged
    over i, then mean_b(w_b .), differentiated by autograd; rows with some u == 0 (where the indicator's convention shows) left out."""
    torch = pytest.importorskip("torch")
    c = qrdqn_ref.case(B, A, N, kappa)
    want = qrdqn_ref.textbook_loss(**c)
    keep = np.flatnonzero(~(want.u == 0).any(axis=(1, 2)))
    assert 0 < len(keep) < B or N == 1
    quant = torch.tensor(c["quant"].astype(np.float64), requires_grad=True)
    theta = quant[torch.arange(B), torch.from_numpy(c["act"]).long()]
    T = torch.from_numpy(want.T)
    tau = (2.0 * torch.arange(N, dtype=torch.float64) + 1.0) / (2.0 * N)
    u = T[:, None, :] - theta[:, :, None]
    hub = torch.nn.functional.huber_loss(theta[:, :, None].expand(B, N, N), T[:, None, :].expand(B, N, N), reduction="none", delta=kappa)
    row_loss = ((tau[None, :, None] - (u.detach() < 0).double()).abs() * hub / kappa).sum(2).mean(1)
    (torch.from_numpy(c["w"].astype(np.float64))[keep] * row_loss[keep]).sum().div(B).backward()
    g = quant.grad.numpy()
    # relative to each row's own scale: its loss, and w_b / B for a gradient whose terms |t| <= 1 may cancel
    assert (np.abs(row_loss.detach().numpy()[keep] - want.row_loss[keep]) <= 1e-12 * want.row_loss[keep]).all()
    scale = (c["w"].astype(np.float64) / B)[keep, None, None]
    assert (np.abs(g[keep] - want.dquant[keep]) <= 1e-12 * scale).all() and np.abs(want.dquant[keep]).max() > 0


def test_terminal_row_on_its_reward_costs_nothing():
    c = qrdqn_ref.case(37, 3, 51, 2.0)
    got = qrdqn_ref.qr_loss(**c)
    for b in (9, 25):
        assert c["flag"][b] == 1.0 and (c["quant"][b, c["act"][b]] == c["rew"][b]).all()
        assert got.row_loss[b] == 0.0 and not got.dquant[b].any()
    assert got.row_loss[np.arange(37) % 16 != 9].min() > 0.0


def test_edge_rows_are_what_they_claim():
    c = qrdqn_ref.case(37, 3, 51, 2.0)
    tb = qrdqn_ref.textbook_loss(**c)
    plain = qrdqn_ref.qr_loss(**{**c, "next_online": None})
    dq = qrdqn_ref.qr_loss(**c)
    assert dq.astar[1] == 0 and plain.astar[1] == 0                       # row 1: every action ties, the first wins
    assert dq.astar[2] == 0 and plain.astar[2] == 2                       # row 2: the two nets disagree
    f32 = qrdqn_ref.F32
    T3 = c["rew"][3] + f32(c["gamma_n"]) * (f32(1.0) - c["flag"][3]) * c["next_target"][3, 0]
    assert (T3[:, None] == c["quant"][3, c["act"][3]][None, :]).any()      # row 3: u == 0 in float32, on a live row
    assert (np.abs(tb.u[4]) == 2.0).sum() >= 2 * 51 // 3                  # row 4: |u| == kappa exactly
    assert (np.diff(c["quant"][5, c["act"][5]]) <= 0).all()                # row 5: crossed
    assert np.abs(tb.u[6]).min() > 1e25                                   # row 6: the linear branch only
    # at |u| == kappa the two Huber branches agree, in float32 as in float64
    k = f32(2.0)
    assert (f32(0.5) * k) * k == k * (k - f32(0.5) * k)


def test_nan_in_one_row_leaves_the_others_alone():
    c = qrdqn_ref.case(37, 2, 51)
    clean = qrdqn_ref.qr_loss(**c)
    q_clean, a_clean = qrdqn_ref.qr_q(c["quant"])
    for key in ("quant", "next_target", "next_online", "rew"):
        d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        d[key][10] = np.nan
        got = qrdqn_ref.qr_loss(**d)
        keep = np.arange(37) != 10
        assert np.array_equal(bits(got.row_loss[keep]), bits(clean.row_loss[keep])) and np.array_equal(bits(got.dquant[keep]), bits(clean.dquant[keep]))
        assert np.array_equal(got.astar[keep], clean.astar[keep])
        assert np.isnan(got.row_loss[10]) or key == "next_online"
    d = c["quant"].copy()
    d[10] = np.nan
    q, a = qrdqn_ref.qr_q(d)
    assert np.array_equal(bits(np.delete(q, 10, 0)), bits(np.delete(q_clean, 10, 0))) and np.array_equal(np.delete(a, 10), np.delete(a_clean, 10))
    assert a[10] == 0                                                     # `q > best` is false for a NaN: the first action stays
