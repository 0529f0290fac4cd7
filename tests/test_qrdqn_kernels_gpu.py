"""GPU: gymrl_qr_q / gymrl_qr_loss bit for bit against tests/qrdqn_ref.py's float32 restatement, on NaN-poisoned output
buffers, at the batch sizes where the kernels' row-to-wave dealing changes (qrdqn.hip: one wave per row, four rows per
workgroup, a grid-stride loop past 4096 workgroups) and at the head's edge rows (qrdqn_ref.case: tied actions, the two nets
disagreeing on a*, terminal rows, u == 0, |u| == kappa, crossed quantiles, magnitudes near 1e30, zero weights)."""
import math

import numpy as np
import pytest
import torch

import qrdqn_ref
from det_math_ref import bits

pytestmark = pytest.mark.gpu

ROWS, WRAP = qrdqn_ref.ROWS_PER_BLOCK, qrdqn_ref.ROWS_PER_BLOCK * qrdqn_ref.MAX_BLOCKS
# one row; a wave's row + 1; a workgroup's rows - 1 and + 1 (the second workgroup: partials + finalize); 257
SEAM_B = [1, 2, ROWS - 1, ROWS + 1, 257]
HEADS = [(1, 1, 1.0), (2, 51, 1.0), (3, 33, 2.0), (8, 64, 0.5)]
PREFILL = 3.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


def run_q(dev, quant, argmax=True):
    """gymrl_qr_q through the C-ABI on poisoned outputs -> (q, argmax)"""
    from gymrl_amd import _lib, ops
    B, A, N = quant.shape
    x = t(quant, dev)
    q = torch.full((B, A), float("nan"), device=dev)
    arg = torch.full((B,), -7, dtype=torch.int32, device=dev)
    rc = _lib.lib().gymrl_qr_q(ops._ptr(x), B, A, N, ops._ptr(q), ops._ptr(arg if argmax else None, None, True), ops._stream())
    assert rc == 0
    return q.cpu().numpy(), arg.cpu().numpy()


def run_loss(dev, c, loss_sum=None):
    """gymrl_qr_loss through the C-ABI on poisoned outputs -> (row_loss, dquant)"""
    from gymrl_amd import _lib, ops
    B, A, N = c["quant"].shape
    d = {k: t(c[k], dev) for k in ("quant", "next_online", "next_target", "act", "rew", "flag", "w")}
    row_loss = torch.full((B,), float("nan"), device=dev)
    dquant = torch.full((B, A, N), float("nan"), device=dev)
    ws = ops._reduce_ws(dev) if loss_sum is not None else None
    rc = _lib.lib().gymrl_qr_loss(ops._ptr(d["quant"]), ops._ptr(d["next_online"], None, True), ops._ptr(d["next_target"]),
                                  ops._ptr(d["act"], torch.int32), ops._ptr(d["rew"]), ops._ptr(d["flag"]), ops._ptr(d["w"], None, True),
                                  B, A, N, c["kappa"], c["gamma_n"], ops._ptr(row_loss), ops._ptr(dquant),
                                  ops._ptr(loss_sum, torch.float64, True), ops._ptr(ws, None, True), ops._stream())
    assert rc == 0
    return row_loss.cpu().numpy(), dquant.cpu().numpy()


def check_loss(dev, c, muted=False):
    """Row outputs: the restatement's bits.  The float64 loss sum: tests/test_c51_kernels_gpu.py's two checks (the exact sum of
    the SAME float32 terms at 1e-12 relative; the all-float64 textbook value at 1e-5 * max(1, |ref|)), `+=` on a prefilled slot,
    and the same rows with no loss sum.
    The 1e30 rows' terms (about 1e32 each) swamp every other row's in those sums: next to them an ordinary row is below one
    float64 ulp of the total, and a sum that lost it would pass.  So a batch that holds such rows is checked a second time with
    w = 0 on them (`muted`): the same checks then hold the sum of the ORDINARY rows, of every workgroup and of every trip of
    the grid-stride loop, at 1e-12 and 1e-5 of a total of ordinary size."""
    B = len(c["act"])
    large = qrdqn_ref.large_rows(B)
    want = qrdqn_ref.qr_loss(**c)
    sums = torch.zeros(1, dtype=torch.float64, device=dev)
    row_loss, dquant = run_loss(dev, c, sums)
    assert same(row_loss, want.row_loss), np.flatnonzero(bits(row_loss) != bits(want.row_loss))[:8]
    assert same(dquant, want.dquant), np.argwhere(bits(dquant) != bits(want.dquant))[:8]
    s0 = float(sums.item())
    exact = math.fsum(want.terms.astype(np.float64).tolist())
    print("loss_sum", s0, "fsum of the float32 terms", exact)
    assert abs(s0 - exact) <= 1e-12 * abs(exact), (s0, exact)
    ref64 = 0.0
    for lo in range(0, len(c["act"]), 2048):                              # (rows are independent: the [B, N, N] broadcast in slices)
        part = {k: (v[lo:lo + 2048] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        ref64 += float((qrdqn_ref.textbook_loss(**part).row_loss * (1.0 if c["w"] is None else part["w"].astype(np.float64))).sum())
    print("float64 textbook", ref64)
    assert abs(s0 - ref64) <= 1e-5 * max(1.0, abs(ref64)), (s0, ref64)
    pre = torch.full((1,), PREFILL, dtype=torch.float64, device=dev)
    again = run_loss(dev, c, pre)
    assert float(pre.item()) == PREFILL + s0 and same(again[0], row_loss) and same(again[1], dquant)
    none = run_loss(dev, c)                                               # no loss sum: no workspace, the same rows
    assert same(none[0], row_loss) and same(none[1], dquant)
    if muted:
        # a total of ordinary size in which every row counts: the smallest non-zero term is 1000 times the 1e-12 tolerance
        live = want.terms[want.terms > 0]
        assert 0.0 < exact < 1e3 * B and live.min() > 1e3 * 1e-12 * exact and not want.terms[large].any()
    elif large.any():
        w = np.ones(B, np.float32) if c["w"] is None else c["w"].copy()
        w[large] = 0.0
        check_loss(dev, {**c, "w": w}, muted=True)


@pytest.mark.parametrize("A,N,kappa", HEADS)
@pytest.mark.parametrize("B", SEAM_B)
def test_qr_q_matches_the_restatement(dev, B, A, N, kappa):
    c = qrdqn_ref.case(B, A, N, kappa)
    for quant in (c["quant"], c["next_target"], c["next_online"]):
        q, arg = run_q(dev, quant)
        wq, warg = qrdqn_ref.qr_q(quant)
        assert same(q, wq) and np.array_equal(arg, warg)
    assert np.array_equal(run_q(dev, c["quant"], argmax=False)[1], np.full(B, -7))       # absent: not touched
    if B > 1 and A > 1:
        assert qrdqn_ref.qr_q(c["next_target"])[1][1] == 0                # row 1: every action ties, the first wins


@pytest.mark.parametrize("A,N,kappa", HEADS)
@pytest.mark.parametrize("B", SEAM_B)
def test_qr_loss_matches_the_restatement(dev, B, A, N, kappa):
    c = qrdqn_ref.case(B, A, N, kappa)
    check_loss(dev, c)                                                    # double-Q, weighted
    if B > 2 and A > 1:
        both = qrdqn_ref.qr_loss(**c).astar, qrdqn_ref.qr_loss(**{**c, "next_online": None}).astar
        assert both[0][2] == 0 and both[1][2] == A - 1                    # row 2: the two nets disagree on a*
    check_loss(dev, {**c, "next_online": None, "w": None})                # plain target selection, weight 1
    check_loss(dev, {**c, "gamma_n": 0.0})                                # every T_j is the reward


def test_qr_past_one_grid_pass(dev):
    """One row more than 4096 workgroups of four rows: the grid-stride loops' second trip."""
    c = qrdqn_ref.case(WRAP + 1, 2, 51)
    check_loss(dev, c)
    q, arg = run_q(dev, c["quant"])
    wq, warg = qrdqn_ref.qr_q(c["quant"])
    assert same(q, wq) and np.array_equal(arg, warg)


def test_qr_rows_do_not_depend_on_the_batch_around_them(dev):
    """The same rows alone and as the prefix of a larger batch: identical q, argmax and row_loss; dquant identical up to the
    1 / B factor — exactly, for two power-of-two batch sizes (values of order 1, so nothing is denormal)."""
    rng = np.random.default_rng(51)
    for small, big, A, N in ((8, 2 * WRAP, 2, 51), (5, 257, 3, 33)):
        mk = lambda *shape: rng.normal(size=shape).astype(np.float32)    # noqa: E731
        c = dict(quant=mk(big, A, N), next_target=mk(big, A, N), next_online=mk(big, A, N), act=rng.integers(0, A, size=big).astype(np.int32),
                 rew=mk(big), flag=(rng.random(big) < 0.2).astype(np.float32), w=rng.uniform(0.5, 1.5, size=big).astype(np.float32),
                 gamma_n=0.99, kappa=1.0)
        head = {k: (v[:small] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        (rl_b, dl_b), (rl_s, dl_s) = run_loss(dev, c), run_loss(dev, head)
        assert same(rl_b[:small], rl_s)
        if big % small == 0:
            assert same(dl_b[:small] * np.float32(big // small), dl_s)
        (q_b, a_b), (q_s, a_s) = run_q(dev, c["quant"]), run_q(dev, head["quant"])
        assert same(q_b[:small], q_s) and np.array_equal(a_b[:small], a_s)


def test_qr_loss_with_an_action_out_of_range_touches_nothing_else(dev):
    c = qrdqn_ref.case(9, 3, 51)
    c["act"][[0, 4, 8]] = [-1, 3, 1 << 30]
    want = qrdqn_ref.qr_loss(**c)
    row_loss, dquant = run_loss(dev, c)
    assert same(row_loss, want.row_loss) and same(dquant, want.dquant)
    assert np.isnan(row_loss[[0, 4, 8]]).all() and not dquant[[0, 4, 8]].any()
    assert np.isfinite(np.delete(row_loss, [0, 4, 8])).all() and np.isfinite(dquant).all()


def test_ops_wrappers(dev):
    """ops.qr_q / ops.qr_loss: the entry points' outputs, an empty batch, and ValueError for a refused shape."""
    from gymrl_amd import ops
    c = qrdqn_ref.case(6, 2, 51)
    d = {k: t(v, dev) for k, v in c.items() if isinstance(v, np.ndarray)}
    q, arg = ops.qr_q(d["quant"].view(6, 102), 2, 51, argmax=True)
    wq, warg = qrdqn_ref.qr_q(c["quant"])
    assert same(q.cpu().numpy(), wq) and np.array_equal(arg.cpu().numpy(), warg)
    assert same(ops.qr_q(d["quant"], 2, 51).cpu().numpy(), wq)
    sums = torch.zeros(1, dtype=torch.float64, device=dev)
    row_loss, dquant = ops.qr_loss(d["quant"], d["next_target"], d["act"], d["rew"], d["flag"], c["gamma_n"], c["kappa"],
                                   next_online=d["next_online"], w=d["w"], loss_sum=sums)
    want = qrdqn_ref.qr_loss(**c)
    assert same(row_loss.cpu().numpy(), want.row_loss) and same(dquant.cpu().numpy(), want.dquant) and sums.item() > 0
    plain = ops.qr_loss(d["quant"], d["next_target"], d["act"], d["rew"], d["flag"], c["gamma_n"])      # kappa defaults to 1
    assert same(plain[0].cpu().numpy(), qrdqn_ref.qr_loss(**{**c, "next_online": None, "w": None}).row_loss)
    empty = torch.empty(0, 2, 51, device=dev)
    e1 = torch.empty(0, device=dev)
    rl, dl = ops.qr_loss(empty, empty, e1.to(torch.int32), e1, e1, 0.99)
    assert rl.shape == (0,) and dl.shape == (0, 2, 51) and ops.qr_q(empty, 2, 51).shape == (0, 2)
    with pytest.raises(ValueError):
        ops.qr_q(torch.zeros(4, 65, device=dev), 1, 65)
    with pytest.raises(ValueError):
        ops.qr_loss(torch.zeros(4, 9, 51, device=dev), torch.zeros(4, 9, 51, device=dev), d["act"][:4], d["rew"][:4], d["flag"][:4], 0.99)
    with pytest.raises(ValueError):
        ops.qr_loss(d["quant"], d["next_target"], d["act"], d["rew"], d["flag"], 0.99, kappa=0.0)
