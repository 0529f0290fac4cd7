"""The CPU twin of tests/test_gae_edges_gpu.py: the C oracle's GAE, moments and normalise restatements against the
definitional longdouble references of tests/gae_refs.py, on the cases the GPU file runs.  The GPU tests hold the kernels
to the oracle bit for bit; this file ties the oracle to something that shares no code with it.

Bounds: the float64 oracles (G1, G3) must meet the float32 rounding of the exact result, rel_close <= 1e-6; the float32
oracle (G2) the 1e-5 of tests/test_hip_parity.py."""
import numpy as np
import pytest

import gae_refs as R
from conftest import rel_close

TOL = 1e-5          # tests/test_hip_parity.py
TOL64 = 1e-6


def _cases():
    yield "structured", R.structured_case
    for T in R.CARRY_T:
        yield f"carry_{T}", lambda T=T: R.carry_case(T, 4)


@pytest.mark.parametrize("name,build", list(_cases()), ids=[n for n, _ in _cases()])
def test_float64_oracles_vs_longdouble(oracle, name, build):
    c = build()
    adv, ret, mom = oracle.gae(c["rew"], c["val"], c["done"], c["nv"], *R.G1, want_moments=True)
    assert rel_close(adv, c["g1_adv"], TOL64) <= TOL64 and rel_close(ret, c["g1_ret"], TOL64) <= TOL64
    assert mom[0] == adv.size and rel_close(mom[1:], c["g1_sums"], 1e-9) <= 1e-9
    adv, ret = oracle.gae_decoupled(c["rew"], c["val"], c["done"], c["nv"], *R.G3)
    assert rel_close(adv, c["g3_adv"], TOL64) <= TOL64 and rel_close(ret, c["g3_ret"], TOL64) <= TOL64


def test_structured_columns(oracle):
    """What each pinned pattern means, asserted on the reference and on the oracle: every step done gives A = r - V
    exactly; a done at T - 1 makes the bootstrap value irrelevant; the byte 255 is a done like the byte 1."""
    c = R.structured_case()
    rew, val, done, nv = c["rew"], c["val"], c["done"], c["nv"]
    assert R.STRUCT_T % 16 == 1 and set(np.unique(done[:, 7])) == {0, 255}
    delta = (rew[:, 4].astype(np.float64) - val[:, 4].astype(np.float64)).astype(np.float32)
    other = nv + np.float32(1000.0)
    for adv, ret in (oracle.gae(rew, val, done, nv, *R.G1), oracle.gae_decoupled(rew, val, done, nv, *R.G3)):
        assert np.array_equal(adv[:, 4], delta)
        assert np.array_equal(adv[:, 7], adv[:, 0]) and np.array_equal(ret[:, 7], ret[:, 0])
    a0, r0 = oracle.gae(rew, val, done, nv, *R.G1)
    a1, r1 = oracle.gae(rew, val, done, other, *R.G1)
    for col in (1, 2, 4):                                              # done at T - 1 (column 1: T - 1 is a chunk's first step)
        assert np.array_equal(a0[:, col], a1[:, col]) and np.array_equal(r0[:, col], r1[:, col])
    assert (a0[-1, [0, 3, 5, 6]] != a1[-1, [0, 3, 5, 6]]).all()   # ... and only there
    assert np.array_equal(c["g1_adv"][:, 4], rew[:, 4].astype(R.LD) - val[:, 4].astype(R.LD))
    assert np.array_equal(c["g1_adv"][:, 7], c["g1_adv"][:, 0])


@pytest.mark.parametrize("N", R.DW_N)
@pytest.mark.parametrize("T", R.DW_T)
def test_gae_dw_oracle_vs_references(oracle, T, N):
    c = R.dw_case(T, N)
    if T * N >= 15:
        assert ((c["dw"] != 0) & (c["done"] == 0)).any() and ((c["dw"] == 0) & (c["done"] != 0)).any()
    adv, vt, mom = oracle.gae_dw(c["rew"], c["val"], c["nval"], c["done"], c["dw"], *R.G1)
    assert np.array_equal(adv, c["adv32"]) and np.array_equal(vt, c["vt32"])       # the float32 restatement: bit for bit
    assert rel_close(adv, c["adv"]) <= TOL and rel_close(vt, c["vt"]) <= TOL
    assert mom[0] == T * N and rel_close(mom[1:], c["sums"], 1e-9) <= 1e-9


@pytest.mark.parametrize("name", R.NORM_SMALL)
def test_moments_normalize_oracle_vs_two_pass(oracle, name):
    """orc_moments against longdouble sums, and orc_normalize's one-pass variance `sum x^2 - n mean^2` against the two-pass
    reference when it is handed correctly rounded sums: at mean / spread = 1e4 the subtraction cancels 8 of a double's 16
    digits and still meets 1e-6.  (Handed orc_moments' own sums it does not, 5.2e-6 at ddof 0: one chain of 100003
    additions leaves sum x^2 = 1e13 off by more than the 1e-12 bound on the sums forbids the kernel's tree to be; the GPU
    file holds the kernel's moments -> normalise pipeline to 1e-6 there.)"""
    x = R.norm_input(name)
    ref = R.moments_ref(x)
    assert rel_close(oracle.moments(x), ref, 1e-12) <= 1e-12
    for ddof in R.NORM_CASES[name][1]:
        y = oracle.normalize(x, ref.astype(np.float64), ddof=ddof)
        if "const" in name:
            assert np.array_equal(y, np.zeros_like(x))
        else:
            assert R.two_pass(x, ddof)[1] > 0
            assert rel_close(y, R.normalize_ref(x, ddof), TOL64) <= TOL64
