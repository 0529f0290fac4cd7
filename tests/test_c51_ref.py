"""CPU: the float32 restatement of the C51 kernels (tests/c51_ref.py: c51_q / c51_loss, the bits the GPU tests demand) against
the float64 textbook algorithm (floor / ceil scatter with the l == u fix, log_softmax), and the textbook's own invariants.

The bounds, derived before any run (u = 2^-24, the float32 unit roundoff; R = vmax - vmin, V = max(|vmin|, |vmax|),
kappa = V / R; every case here has kappa <= 1):

  b_j   z_j = vmin + j dz carries the roundings of R, dz, j dz and the sum (<= 4 u V); (float)gamma_n, g z_j and rew + g z_j add
        <= 3 u V where the clamp does not replace the value (where it does, both sides hold vmin or vmax exactly); Tz - vmin
        rounds once (u R) and the division by dz carries dz's 2 u and its own u, all relative to b <= M - 1:
            |db| <= (M - 1) u (7 kappa + 4)
  p_j   d = x - max is rounded (u |d|), det_expf is within 1.0103 ulp, so |de_j| <= 3 u e_j + u |d_j| e_j <= 3 u e_j + 0.37 u;
        the 64-slot tree adds 6 u, the division u:  sum_j |dp_j| <= 13 u + 0.37 M u
  m_i   = sum_j p*_j max(0, 1 - |b_j - i|), 1-Lipschitz in b_j, sum_j p*_j = 1, M serial additions and 3 roundings per term:
            |dm_i| <= |db| + (13 + 0.37 M) u + (M + 2) u  <=  u ((M - 1)(7 kappa + 6) + 18)                      = TOL_M
        (the issue's estimate: the rounding of b alone is about (M - 1) 2^-23 — the first term with kappa ~ 1/2), and over a row
            sum_i |dm_i| <= 2 |db| + (13 + 0.37 M) u + (M + 2) u  <=  u ((M - 1)(14 kappa + 9.4) + 17)
  loss  with L = max_i |logp_i| of the row (float64 side): |dlogp_i| <= u (2 L + 14) (d, the sum, det_logf's 0.83 ulp, the
        subtraction), the tree of products 7 u L:
            |d row_loss| <= u (((M - 1)(14 kappa + 9.4) + 26) L + 14)                                              = TOL_LOSS(L)
  grad  B dlogits / w = p - m:  TOL_M + 14 u                                                                      = TOL_GRAD
  q     = sum_j p_j z_j:  V (13 + 0.37 M) u for p, 4 u V for z, 7 u V for the tree:  u V (0.37 M + 24)             = TOL_Q

profiles/c51_tolerances.json records these expressions and the maxima this test measured (GYMRL_C51_TOL_OUT=<file> rewrites it).
"""
import json
import os

import numpy as np
import pytest

import c51_ref

U = 2.0 ** -24
SHAPES = [(37, 1, 2, 0.0, 1.0), (37, 2, 33, -10.0, 10.0), (37, 2, 51, 0.0, 100.0), (37, 3, 51, -100.0, 0.0), (37, 8, 64, 0.0, 10.0)]
_measured = {}


def kappa(vmin, vmax):
    return max(abs(vmin), abs(vmax)) / (vmax - vmin)


def tol_m(M, k):
    return U * ((M - 1) * (7 * k + 6) + 18)


def tol_loss(M, k, L):
    return U * (((M - 1) * (14 * k + 9.4) + 26) * L + 14)


def tol_q(M, vmin, vmax):
    return U * max(abs(vmin), abs(vmax)) * (0.37 * M + 24)


@pytest.fixture(scope="module", autouse=True)
def ledger():
    yield
    path = os.environ.get("GYMRL_C51_TOL_OUT")
    if path and _measured:
        doc = {"unit": "u = 2^-24; kappa = max(|vmin|, |vmax|) / (vmax - vmin); L = max_i |log_softmax_i| of the row",
               "bounds": {"m": "u ((M - 1)(7 kappa + 6) + 18)", "row_loss": "u (((M - 1)(14 kappa + 9.4) + 26) L + 14)",
                          "grad": "bound(m) + 14 u", "q": "u max(|vmin|, |vmax|) (0.37 M + 24)"},
               "derivation": "tests/test_c51_ref.py, module docstring",
               "measured_max_over_bound": _measured}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


@pytest.mark.parametrize("B,A,M,vmin,vmax", SHAPES)
@pytest.mark.parametrize("variant", ["plain", "double_q_weighted", "gamma0"])
def test_float32_restatement_is_within_the_derived_bounds_of_the_textbook(B, A, M, vmin, vmax, variant):
    c = c51_ref.case(B, A, M, vmin, vmax)
    if variant == "plain":
        c["next_online"] = c["w"] = None
    if variant == "gamma0":
        c["gamma_n"] = 0.0
    got, want = c51_ref.c51_loss(**c), c51_ref.textbook_loss(**c)
    k = kappa(vmin, vmax)
    assert np.array_equal(got.astar, want.astar)
    L = np.abs(want.logp).max(axis=1)
    err = {"m": np.abs(got.m - want.m).max() / tol_m(M, k),
           "row_loss": (np.abs(got.row_loss - want.row_loss) / tol_loss(M, k, L)).max()}
    wb = np.ones(B) if c["w"] is None else c["w"].astype(np.float64)
    live = wb > 0
    rows = np.arange(B)
    scale = (B / wb[live])[:, None]
    err["grad"] = (np.abs(got.dlogits[rows, c["act"]][live] - want.dlogits[rows, c["act"]][live]) * scale).max() / (tol_m(M, k) + 14 * U)
    q32, _ = c51_ref.c51_q(c["logits"], vmin, vmax)
    q64, _ = c51_ref.textbook_q(c["logits"], vmin, vmax)
    err["q"] = np.abs(q32 - q64).max() / tol_q(M, vmin, vmax)
    key = f"B{B}_A{A}_M{M}_[{vmin:g},{vmax:g}]_{variant}"
    _measured[key] = {n: float(f"{v:.4g}") for n, v in err.items()}
    print(key, _measured[key])
    assert all(v <= 1.0 for v in err.values()), err
    # what the kernel writes outside the taken action, and for a zero weight: exact zeros
    other = np.ones((B, A), bool)
    other[rows, c["act"]] = False
    assert not got.dlogits[other].any() and not got.dlogits[~live].any()


@pytest.mark.parametrize("B,A,M,vmin,vmax", SHAPES)
def test_textbook_projection_keeps_the_mass(B, A, M, vmin, vmax):
    c = c51_ref.case(B, A, M, vmin, vmax)
    for gamma_n in (c["gamma_n"], 0.0, 1.0):
        m = c51_ref.textbook_loss(**{**c, "gamma_n": gamma_n}).m
        assert np.abs(m.sum(axis=1) - 1.0).max() <= 1e-12 and m.min() >= 0.0


@pytest.mark.parametrize("M,vmin,vmax", [(2, 0.0, 1.0), (33, -16.0, 16.0), (51, 0.0, 100.0), (64, 0.0, 63.0)])
def test_textbook_terminal_reward_on_an_atom_puts_mass_one_there(M, vmin, vmax):
    """Supports whose atoms are exact in binary: b is an integer, l == u, and the unfixed textbook code would drop the row's mass."""
    z = np.linspace(vmin, vmax, M)
    rng = np.random.default_rng(M)
    pstar = rng.random((M, M))
    pstar /= pstar.sum(axis=1, keepdims=True)
    m = c51_ref.textbook_project(pstar, rew=z, flag=np.ones(M), gamma_n=0.97, M=M, vmin=vmin, vmax=vmax)
    assert np.abs(m - np.eye(M)).max() <= 1e-15 * M
    # and the float32 gather form agrees exactly: weight 1 on the atom, 0 on its neighbours
    logits = np.log(pstar)[:, None, :].astype(np.float32)
    got = c51_ref.c51_loss(logits, logits, np.zeros(M, np.int32), z.astype(np.float32), np.ones(M, np.float32), 0.97, vmin, vmax)
    assert np.abs(got.m - np.eye(M)).max() <= (1.37 * M + 15) * U      # sum_j p*_j in float32, nothing else: the p and sum terms above


def test_tolerance_file_states_these_bounds():
    from conftest import ROOT
    doc = json.load(open(os.path.join(ROOT, "profiles", "c51_tolerances.json")))
    assert doc["bounds"]["m"] == "u ((M - 1)(7 kappa + 6) + 18)"
    assert doc["measured_max_over_bound"] and all(v <= 1.0 for case in doc["measured_max_over_bound"].values() for v in case.values())
