"""The on-policy loss kernels of csrc/ppo.hip / policy_device.hpp — L1 gymrl_ppo_loss_fwd_bwd, L3
gymrl_ppo_full_loss_fwd_bwd, L4 gymrl_ppo_rnn_loss_fwd_bwd — and gymrl_categorical_sample against the float64 autograd
references of tests/onpolicy_refs.py, at the sizes where the kernels change path:

  seams        one wave / one block / several blocks (B = 1 .. 1025), the float2 (A = 2), float4 (A = 4) and scalar row forms
  grid stride  B > 1024 blocks x 256 threads: the second and third turn of the row loop, L1's barrier after the first turn,
               and in L4's count pass a per-thread count above 1 (the ballot loop over bits >= 1)
  planted rows saturated logits, ratio beyond the dual clip and below 1 - eps, adv == 0, the entropy band's two sides,
               corr_mul zeros, the value clip's four cases, advantage moments with a variance of 1e-10
  masks        all rows outside the entropy band, an empty L4 mask, a single live row

Every comparison goes through conftest.bounded; profiles/onpolicy_edge_tolerances.json holds one run's observed errors.
tests/test_onpolicy_edges.py runs the same cases against the C oracle on the CPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import onpolicy_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
TAG = "onpolicy hip"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def run(dev):
    from gymrl_amd import ops
    fns = {"ppo": ops.ppo_loss_fwd_bwd, "ppo_full": ops.ppo_full_loss_fwd_bwd, "ppo_rnn": ops.ppo_rnn_loss_fwd_bwd}

    def call(c):
        args, kw = R.case_args(c, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        met = torch.zeros(R.N_METRICS[c.kind], dtype=torch.float64, device=dev)
        dz, dv = fns[c.kind](*args, metrics_sum=met, **kw)
        assert dz.shape == (c.B, c.A) and dv.shape == (c.B,)
        return dz.cpu().numpy(), dv.cpu().numpy(), met.cpu().numpy()
    return call


@pytest.fixture(scope="module")
def sample(dev):
    from gymrl_amd import ops

    def call(logits, q, det):
        t = lambda a: None if a is None else torch.from_numpy(a).to(dev)   # noqa: E731
        return [x.cpu().numpy() for x in ops.categorical_sample(t(logits), noise_exp=t(q), deterministic=det)[:3]]
    return call


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("B,A", R.SEAM_SHAPES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_seams(run, kind, B, A, with_idx):
    R.check_seam(run, TAG, kind, B, A, with_idx)


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("B,A", R.SEAM_SHAPES)
def test_seams_ppo_adv_moments(run, B, A, with_idx):
    R.check_seam(run, TAG, "ppo", B, A, with_idx, "rollout")


@pytest.mark.parametrize("B,A", R.GRID_SHAPES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_grid_stride(run, kind, B, A):
    """262145: one thread takes a second row; 262144 + 300: a second turn with a partial block; 524293: some threads hold
    three rows.  compare() holds L4's metric 9, the sum of corr, to the reference's mask count exactly: the integer
    erc_count_kernel adds up bit by bit is the 1 / count every gradient was scaled by."""
    c = R.check_seam(run, f"{TAG} grid stride", kind, B, A, True)
    if kind == "ppo_rnn":
        assert 0 < R.reference(c)[2][9] < B


@pytest.mark.parametrize("A", R.PLANTED_A)
@pytest.mark.parametrize("kind", R.KINDS)
def test_planted_rows(run, kind, A):
    R.check_planted(run, TAG, kind, A)


@pytest.mark.parametrize("A", R.PLANTED_A)
def test_planted_rows_ppo_tiny_variance_moments(run, A):
    R.check_planted(run, TAG, "ppo", A, "tiny")


@pytest.mark.parametrize("A", R.PLANTED_A)
def test_ppo_full_entropy_coef_dev(run, A):
    R.check_entropy_coef_dev(run, TAG, A)


def test_ppo_full_all_rows_out_of_band(run):
    R.check_full_all_out(run, TAG)


def test_ppo_rnn_empty_mask(run):
    R.check_rnn_empty(run, TAG)


@pytest.mark.parametrize("row", [0, -1])
def test_ppo_rnn_one_live_row(run, row):
    R.check_rnn_one_live(run, TAG, row)


@pytest.mark.parametrize("A,n", R.SAMPLE_SHAPES)
def test_categorical_sample(sample, A, n):
    R.check_sample(sample, TAG, A, n)
