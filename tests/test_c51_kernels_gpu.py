"""GPU: gymrl_c51_q / gymrl_c51_loss bit for bit against tests/c51_ref.py's float32 restatement, on NaN-poisoned output
buffers, at the batch sizes where the kernels' row-to-wave dealing changes (c51.hip: one wave per row, four rows per
workgroup, a grid-stride loop past 4096 workgroups) and at the head's edge rows (c51_ref.case: tied actions, saturated
softmaxes, clamped and terminal rows, zero weights, the two nets disagreeing on a*)."""
import math

import numpy as np
import pytest
import torch

import c51_ref
from det_math_ref import bits

pytestmark = pytest.mark.gpu

ROWS, WRAP = c51_ref.ROWS_PER_BLOCK, c51_ref.ROWS_PER_BLOCK * c51_ref.MAX_BLOCKS
# one row; a wave's row + 1; a workgroup's rows - 1 and + 1 (the second workgroup: partials + finalize); 257
SEAM_B = [1, 2, ROWS - 1, ROWS + 1, 257]
HEADS = [(1, 2, 0.0, 1.0), (2, 51, 0.0, 100.0), (3, 33, -100.0, 0.0), (8, 64, -10.0, 10.0)]
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


def run_q(dev, logits, vmin, vmax, argmax=True):
    """gymrl_c51_q through the C-ABI on poisoned outputs -> (q, argmax)"""
    from gymrl_amd import _lib, ops
    B, A, M = logits.shape
    x = t(logits, dev)
    q = torch.full((B, A), float("nan"), device=dev)
    arg = torch.full((B,), -7, dtype=torch.int32, device=dev)
    rc = _lib.lib().gymrl_c51_q(ops._ptr(x), B, A, M, vmin, vmax, ops._ptr(q), ops._ptr(arg if argmax else None, None, True), ops._stream())
    assert rc == 0
    return q.cpu().numpy(), arg.cpu().numpy()


def run_loss(dev, c, loss_sum=None):
    """gymrl_c51_loss through the C-ABI on poisoned outputs -> (row_loss, dlogits)"""
    from gymrl_amd import _lib, ops
    B, A, M = c["logits"].shape
    d = {k: t(c[k], dev) for k in ("logits", "next_online", "next_target", "act", "rew", "flag", "w")}
    row_loss = torch.full((B,), float("nan"), device=dev)
    dlogits = torch.full((B, A, M), float("nan"), device=dev)
    ws = ops._reduce_ws(dev) if loss_sum is not None else None
    rc = _lib.lib().gymrl_c51_loss(ops._ptr(d["logits"]), ops._ptr(d["next_online"], None, True), ops._ptr(d["next_target"]),
                                   ops._ptr(d["act"], torch.int32), ops._ptr(d["rew"]), ops._ptr(d["flag"]), ops._ptr(d["w"], None, True),
                                   B, A, M, c["vmin"], c["vmax"], c["gamma_n"], ops._ptr(row_loss), ops._ptr(dlogits),
                                   ops._ptr(loss_sum, torch.float64, True), ops._ptr(ws, None, True), ops._stream())
    assert rc == 0
    return row_loss.cpu().numpy(), dlogits.cpu().numpy()


def check_loss(dev, c):
    """Row outputs: the restatement's bits.  The float64 loss sum: tests/test_offpolicy_edges_gpu.py's two checks (the exact sum of
    the SAME float32 terms at 1e-12 relative; the all-float64 textbook value at 1e-5 * max(1, |ref|)), `+=` on a prefilled slot."""
    want = c51_ref.c51_loss(**c)
    sums = torch.zeros(1, dtype=torch.float64, device=dev)
    row_loss, dlogits = run_loss(dev, c, sums)
    assert same(row_loss, want.row_loss), np.flatnonzero(bits(row_loss) != bits(want.row_loss))[:8]
    assert same(dlogits, want.dlogits), np.argwhere(bits(dlogits) != bits(want.dlogits))[:8]
    s0 = float(sums.item())
    exact = math.fsum(want.terms.astype(np.float64).tolist())
    assert abs(s0 - exact) <= 1e-12 * abs(exact), (s0, exact)
    tb = c51_ref.textbook_loss(**c)
    ref64 = float((tb.row_loss * (1.0 if c["w"] is None else c["w"].astype(np.float64))).sum())
    assert abs(s0 - ref64) <= 1e-5 * max(1.0, abs(ref64)), (s0, ref64)
    pre = torch.full((1,), PREFILL, dtype=torch.float64, device=dev)
    again = run_loss(dev, c, pre)
    assert float(pre.item()) == PREFILL + s0 and same(again[0], row_loss) and same(again[1], dlogits)
    none = run_loss(dev, c)                                               # no loss sum: no workspace, the same rows
    assert same(none[0], row_loss) and same(none[1], dlogits)


@pytest.mark.parametrize("A,M,vmin,vmax", HEADS)
@pytest.mark.parametrize("B", SEAM_B)
def test_c51_q_matches_the_restatement(dev, B, A, M, vmin, vmax):
    c = c51_ref.case(B, A, M, vmin, vmax)
    for logits in (c["logits"], c["next_target"], c["next_online"]):
        q, arg = run_q(dev, logits, vmin, vmax)
        wq, warg = c51_ref.c51_q(logits, vmin, vmax)
        assert same(q, wq) and np.array_equal(arg, warg)
    assert np.array_equal(run_q(dev, c["logits"], vmin, vmax, argmax=False)[1], np.full(B, -7))       # absent: not touched
    if B > 1 and A > 1:
        assert c51_ref.c51_q(c["next_target"], vmin, vmax)[1][1] == 0                                 # row 1: every action ties, the first wins


@pytest.mark.parametrize("A,M,vmin,vmax", HEADS)
@pytest.mark.parametrize("B", SEAM_B)
def test_c51_loss_matches_the_restatement(dev, B, A, M, vmin, vmax):
    c = c51_ref.case(B, A, M, vmin, vmax)
    check_loss(dev, c)                                                    # double-Q, weighted
    if B > 2 and A > 1:
        both = c51_ref.c51_loss(**c).astar, c51_ref.c51_loss(**{**c, "next_online": None}).astar
        assert both[0][2] == 0 and both[1][2] == A - 1                    # row 2: the two nets disagree on a*
    check_loss(dev, {**c, "next_online": None, "w": None})                # plain target selection, weight 1
    check_loss(dev, {**c, "gamma_n": 0.0})                                # every atom lands on the reward


def test_c51_past_one_grid_pass(dev):
    """One row more than 4096 workgroups of four rows: the grid-stride loops' second trip."""
    c = c51_ref.case(WRAP + 1, 2, 51)
    check_loss(dev, c)
    q, arg = run_q(dev, c["logits"], c["vmin"], c["vmax"])
    wq, warg = c51_ref.c51_q(c["logits"], c["vmin"], c["vmax"])
    assert same(q, wq) and np.array_equal(arg, warg)


def test_c51_rows_do_not_depend_on_the_batch_around_them(dev):
    """The same rows alone and as the prefix of a larger batch: identical q, argmax and row_loss; dlogits identical up to the
    1 / B factor — exactly, for two power-of-two batch sizes (rows without saturated softmaxes, so nothing is denormal)."""
    rng = np.random.default_rng(51)
    for small, big, A, M in ((8, 2 * WRAP, 2, 51), (5, 257, 3, 33)):
        mk = lambda *shape: rng.normal(size=shape).astype(np.float32)    # noqa: E731
        c = dict(logits=mk(big, A, M), next_target=mk(big, A, M), next_online=mk(big, A, M), act=rng.integers(0, A, size=big).astype(np.int32),
                 rew=mk(big), flag=(rng.random(big) < 0.2).astype(np.float32), w=rng.uniform(0.5, 1.5, size=big).astype(np.float32),
                 gamma_n=0.99, vmin=-10.0, vmax=10.0)
        head = {k: (v[:small] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        (rl_b, dl_b), (rl_s, dl_s) = run_loss(dev, c), run_loss(dev, head)
        assert same(rl_b[:small], rl_s)
        if big % small == 0:
            assert same(dl_b[:small] * np.float32(big // small), dl_s)
        (q_b, a_b), (q_s, a_s) = run_q(dev, c["logits"], -10.0, 10.0), run_q(dev, head["logits"], -10.0, 10.0)
        assert same(q_b[:small], q_s) and np.array_equal(a_b[:small], a_s)


def test_c51_loss_with_an_action_out_of_range_touches_nothing_else(dev):
    c = c51_ref.case(9, 3, 51)
    c["act"][[0, 4, 8]] = [-1, 3, 1 << 30]
    want = c51_ref.c51_loss(**c)
    row_loss, dlogits = run_loss(dev, c)
    assert same(row_loss, want.row_loss) and same(dlogits, want.dlogits)
    assert np.isnan(row_loss[[0, 4, 8]]).all() and not dlogits[[0, 4, 8]].any() and np.isfinite(np.delete(row_loss, [0, 4, 8])).all()


def test_ops_wrappers(dev):
    """ops.c51_q / ops.c51_loss: the entry points' outputs, an empty batch, and ValueError for a refused shape."""
    from gymrl_amd import ops
    c = c51_ref.case(6, 2, 51)
    d = {k: t(v, dev) for k, v in c.items() if isinstance(v, np.ndarray)}
    q, arg = ops.c51_q(d["logits"].view(6, 102), 2, 51, 0.0, 100.0, argmax=True)
    wq, warg = c51_ref.c51_q(c["logits"], 0.0, 100.0)
    assert same(q.cpu().numpy(), wq) and np.array_equal(arg.cpu().numpy(), warg)
    assert same(ops.c51_q(d["logits"], 2, 51, 0.0, 100.0).cpu().numpy(), wq)
    sums = torch.zeros(1, dtype=torch.float64, device=dev)
    row_loss, dlogits = ops.c51_loss(d["logits"], d["next_target"], d["act"], d["rew"], d["flag"], c["gamma_n"], 0.0, 100.0,
                                     next_online=d["next_online"], w=d["w"], loss_sum=sums)
    want = c51_ref.c51_loss(**c)
    assert same(row_loss.cpu().numpy(), want.row_loss) and same(dlogits.cpu().numpy(), want.dlogits) and sums.item() > 0
    empty = torch.empty(0, 2, 51, device=dev)
    e1 = torch.empty(0, device=dev)
    rl, dl = ops.c51_loss(empty, empty, e1.to(torch.int32), e1, e1, 0.99, 0.0, 100.0)
    assert rl.shape == (0,) and dl.shape == (0, 2, 51) and ops.c51_q(empty, 2, 51, 0.0, 100.0).shape == (0, 2)
    with pytest.raises(ValueError):
        ops.c51_q(torch.zeros(4, 65, device=dev), 1, 65, 0.0, 1.0)
    with pytest.raises(ValueError):
        ops.c51_loss(torch.zeros(4, 9, 51, device=dev), torch.zeros(4, 9, 51, device=dev), d["act"][:4], d["rew"][:4], d["flag"][:4], 0.99, 0.0, 1.0)
