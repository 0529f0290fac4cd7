"""The CPU twin of tests/test_onpolicy_edges_gpu.py: the float64 autograd references of tests/onpolicy_refs.py against the C
oracle (oracle/gymrl_oracle.c), which restates ppo.hip / policy_device.hpp line by line — the same builder, the same seam,
planted and degenerate-mask cases, the same bounds.  It validates the references, the margin condition and the tolerances on
a machine without a GPU; a disagreement here is a finding about the oracle, and so about the kernel it restates."""
import numpy as np
import pytest

pytest.importorskip("torch")

import onpolicy_refs as R  # noqa: E402

TAG = "onpolicy oracle"


@pytest.fixture(scope="module")
def run(oracle):
    def call(c):
        args, kw = R.case_args(c)
        if c.kind == "ppo":
            return oracle.ppo_loss_fwd_bwd(*args, **kw)
        if c.kind == "ppo_full":
            dev = kw.pop("entropy_coef_dev")                           # the oracle has no device memory: the value the kernel
            if dev is not None:                                        # would read there goes into its cfg
                args[-1] = tuple(args[-1][:5]) + (float(dev[0]),)
            return oracle.ppo_full_loss_fwd_bwd(*args, **kw)
        return oracle.ppo_rnn_loss_fwd_bwd(*args, **kw)
    return call


@pytest.fixture(scope="module")
def sample(oracle):
    return lambda logits, q, det: oracle.categorical_sample(logits, noise_exp=q, deterministic=det)[:3]


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("B,A", R.SEAM_SHAPES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_seams(run, kind, B, A, with_idx):
    R.check_seam(run, TAG, kind, B, A, with_idx)


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("B,A", R.SEAM_SHAPES)
def test_seams_ppo_adv_moments(run, B, A, with_idx):
    R.check_seam(run, TAG, "ppo", B, A, with_idx, "rollout")


@pytest.mark.parametrize("A", R.PLANTED_A)
@pytest.mark.parametrize("kind", R.KINDS)
def test_planted_rows(run, kind, A):
    c = R.check_planted(run, TAG, kind, A)
    assert c.moved < c.B                                               # rows moved off a threshold stay in the comparison


@pytest.mark.parametrize("A", R.PLANTED_A)
def test_planted_rows_ppo_tiny_variance_moments(run, A):
    R.check_planted(run, TAG, "ppo", A, "tiny")


@pytest.mark.parametrize("A", R.PLANTED_A)
def test_ppo_full_entropy_coef_dev(run, A):
    R.check_entropy_coef_dev(run, TAG, A)


def test_degenerate_masks(run):
    R.check_full_all_out(run, TAG)
    R.check_rnn_empty(run, TAG)
    R.check_rnn_one_live(run, TAG, 0)
    R.check_rnn_one_live(run, TAG, -1)


@pytest.mark.parametrize("A,n", R.SAMPLE_SHAPES)
def test_categorical_sample(sample, A, n):
    R.check_sample(sample, TAG, A, n)


def test_margin_builder_moves_rows_and_excludes_none():
    """At 4099 rows some random row does land within 1e-3 of a threshold: the builder moves it and keeps it, and every decision
    quantity of every row ends outside its margin (make_case asserts that; this re-derives it)."""
    c = R.get_case("ppo_rnn", 4099, 4, True)
    assert c.moved > 0
    for name, q, thr, rows, _ in R.decisions(c):
        assert q.shape == (c.B,) and not R._near(q, thr, rows).any(), name
    assert np.unique(c.idx).size == c.B and c.idx.max() < c.M
