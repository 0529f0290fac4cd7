"""The seams of csrc/per.hip and csrc/replay.hip: the branches of gymrl_per_update's dispatch and of the launch geometry
that one shape per kernel (tests/test_hip_parity_offpolicy.py, tests/test_step_chunk_gpu.py) does not reach.

Every case goes through the C-ABI wrappers of gymrl_amd/ops.py and is compared with the CPU oracle (oracle.SumTree,
oracle.per_priorities, oracle.ReplayRing, oracle.NStepWindows) — never with another kernel path.  The float64 tree, the
indices, the ring and the window arrays are compared bit for bit; only the importance weights carry a tolerance, the
rel_close <= 1e-6 of test_sumtree_update_order_exact (the device's pow against libm's).  tests/test_replay_edges.py ties
the oracle, at these cases, to plain Python.

  branch (condition in the code)                                              reached by
  per_leaf_kernel / per_ancestor_kernel, use_lds = 0 (B > kLdsB)              test_explicit_batches_past_8192
  the store's chunk loop, o > 0 (B > per::kStoreChunk)                        test_stores_past_one_chunk, test_max_leaf_grid_stride
  td_priority's clip; SMALL_FUSED with nb = 0; SMALL_LEAF + SMALL_ANC         test_update_td_vs_oracle
  small_max_block with two blocks, the second partial (cap = 8193)            test_update_td_vs_oracle, test_update_td_directed_maxima
  per_sample_kernel: normalize_here (nb == 1), padding lanes, beta = 0        test_sample_edges
  gymrl_per_max_leaf's grid clamp (cdiv(cap, 2048) > 1024)                    test_max_leaf_grid_stride
  nstep_push_kernel past one block, n_steps = 1 and 2, terminal == NULL       test_nstep_windows_past_one_block, test_nstep_inline_terminal
  replay_append_kernel / replay_gather_kernel's stride (nb > 4096), AW = 2    test_ring_*"""
import numpy as np
import pytest

import replay_refs as R
from conftest import rel_close

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ALPHA, EPS = 0.6, 0.01


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)              # (a copy: the shared inputs are read-only)


def new_tree(cap, dev):
    return torch.zeros(2 * cap - 1, dtype=torch.float64, device=dev)


def same_tree(tree, ref):
    return np.array_equal(tree.cpu().numpy(), ref.tree)


# ============================================================ 1. explicit indices past 8192 ==========
@pytest.mark.parametrize("cap,B,spread,idx_is_tree", [(20000, 8193, 20000, False), (20000, 9000, 200, True),
                                                      (5, 8200, 5, False)])
def test_explicit_batches_past_8192(dev, oracle, cap, B, spread, idx_is_tree):
    """B > kLdsB: gymrl_per_update falls through to per_leaf_kernel / per_ancestor_kernel with use_lds = 0, which search
    the batch in global memory.  Twice on the same tree (the second call starts from non-zero nodes), with indices from
    the whole capacity, from a narrow range (every leaf hit ~45 times), and on a 5-leaf tree whose leaves lie at two
    depths (every leaf hit ~1640 times): float64 tree == the reference's sequential loop, bit for bit."""
    from gymrl_amd import ops
    rng = np.random.default_rng(cap + B)
    tree, ref = new_tree(cap, dev), oracle.SumTree(cap)
    ws = ops.per_workspace(B, dev)
    for rnd in range(2):
        idx = rng.integers(0, spread, size=B).astype(np.int32) + (cap - 1 if idx_is_tree else 0)
        pr = rng.random(B) * 3 + 1e-3
        ops.per_update(tree, cap, B, ws, idx=t(idx, dev), idx_is_tree=idx_is_tree, prio=t(pr, dev))
        ref.update_many(idx=idx, prio=pr, idx_is_tree=idx_is_tree)
        assert same_tree(tree, ref), rnd
    assert len(np.unique(idx)) < B                                      # duplicates were there


# ============================================================ 2. stores past one chunk ===============
@pytest.mark.parametrize("cap,n,start,scalar", [(20000, 8193, 123, None), (20000, 16384, 19000, None),
                                                (20000, 20000, 15000, None), (16384, 16384, 1, 2.5)])
def test_stores_past_one_chunk(dev, oracle, cap, n, start, scalar):
    """n > per::kStoreChunk: the chunk loop launches a second (and third) sub-store with offset > 0 and prio + o, on the
    same ws.change / ws.partial (rule 4 of the store's definition, oracle/offpolicy_oracle.c).  (20000, 20000) from 15000
    wraps inside its second sub-store.  Each store is followed by an explicit update of 300 indices; then the same store
    again, from another cursor, onto the tree that is now full."""
    from gymrl_amd import ops
    rng = np.random.default_rng(cap + n)
    tree, ref = new_tree(cap, dev), oracle.SumTree(cap)
    ws = ops.per_workspace(n, dev)
    for rnd, s in enumerate((start, (start + 7777) % cap)):
        pr = None if scalar is not None else rng.random(n) * 3 + 1e-3
        ops.per_update(tree, cap, n, ws, idx_start=s, prio=None if pr is None else t(pr, dev), prio_scalar=scalar or 0.0)
        ref.update_many(idx_start=s, prio=pr, prio_scalar=scalar or 0.0, B=n)
        assert same_tree(tree, ref), ("store", rnd)
        idx = rng.integers(0, cap, size=300).astype(np.int32)
        pr = rng.random(300) * 3 + 1e-3
        ops.per_update(tree, cap, 300, ws, idx=t(idx, dev), prio=t(pr, dev))
        ref.update_many(idx=idx, prio=pr)
        assert same_tree(tree, ref), ("update", rnd)


# ============================================================ 3. per_update_td against the oracle ====
class TdPair:
    """A device tree and the oracle's, filled by one store, and gymrl_per_update_td beside the oracle's
    per_priorities -> update_many -> max_leaf."""

    def __init__(self, dev, oracle, cap, fill):
        from gymrl_amd import ops
        self.ops, self.dev, self.oracle, self.cap = ops, dev, oracle, cap
        self.tree, self.ref = new_tree(cap, dev), oracle.SumTree(cap)
        self.ws = ops.per_workspace(max(8192, cap), dev)
        self.mx = torch.full((1,), -1.0, dtype=torch.float64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        fill = np.broadcast_to(np.asarray(fill, np.float64), (cap,)).copy()
        ops.per_update(self.tree, cap, cap, self.ws, idx_start=0, prio=t(fill, dev))
        self.ref.update_many(idx_start=0, prio=fill)
        assert same_tree(self.tree, self.ref)

    def plant(self, leaf, value):
        self.ops.per_update(self.tree, self.cap, 1, self.ws, idx=t(np.array([leaf], np.int32), self.dev),
                            prio=t(np.array([value]), self.dev))
        self.ref.update(leaf, value)

    def update_td(self, idx, td, mode, clip=0.0):
        """mode: "max" (ticket and max_out: one launch with the maximum blocks), "ticket" (one launch, nb = 0),
        "plain" (neither: a leaf launch and a depth launch).  Returns (device maximum or None, oracle maximum, priorities)."""
        idx, td = np.asarray(idx, np.int32), np.asarray(td, np.float32)
        self.mx.fill_(-1.0)
        self.ops.per_update_td(self.tree, self.cap, t(idx, self.dev), t(td, self.dev), ALPHA, EPS, self.ws, clip=clip,
                               max_out=self.mx if mode == "max" else None, ticket=None if mode == "plain" else self.ticket)
        p = self.oracle.per_priorities(td, ALPHA, EPS, clip)
        self.ref.update_many(idx=idx, prio=p)
        assert same_tree(self.tree, self.ref), mode
        assert int(self.ticket.item()) == 0, mode                       # the ticket reads 0 after every fused call
        want = self.ref.max_leaf()
        if mode != "max":
            assert self.mx.item() == -1.0                                # max_out == NULL: not written
            return None, want, p
        assert self.mx.item() == want, (self.mx.item(), want)
        return self.mx.item(), want, p


MODES = ("max", "ticket", "plain")


@pytest.mark.parametrize("B", [1, 64, 65, 512])
@pytest.mark.parametrize("cap", [1, 2, 3, 300, 8193])
def test_update_td_vs_oracle(dev, oracle, cap, B):
    """Caps with no ancestor (1), one depth (2), leaves at two depths (3), 300, and 8193 = two maximum blocks, the second
    with one leaf; batches of one lane, one wave, one wave + 1 and the largest.  In each argument form consecutive calls
    on one tree with one ticket tensor (five with the maximum), the clip off and on (|td| + eps on both sides of it)."""
    rng = np.random.default_rng(100 * cap + B)
    for mode in MODES:
        pair = TdPair(dev, oracle, cap, rng.random(cap) + 0.1)
        for call in range(5 if mode == "max" else 3):
            idx = rng.integers(0, cap, size=B)
            if B > 8:
                idx[5] = idx[B - 1] = idx[2]                             # a leaf three times, its last element the batch's last
            td = (rng.normal(size=B) * 3).astype(np.float32)
            clip = 1.0 if call % 2 else 0.0
            if clip and B >= 64:
                e = np.abs(td) + np.float32(EPS)
                assert (e > 1.0).any() and (e < 1.0).any()
            _, _, p = pair.update_td(idx, td, mode, clip)
            assert not clip or p.max() <= 1.0


@pytest.mark.parametrize("cap", [3, 300, 8193])
def test_update_td_batch_of_one_leaf(dev, oracle, cap):
    """512 elements on the last leaf: one run of 512 ordered additions per ancestor, 511 superseded leaf writes."""
    rng = np.random.default_rng(cap)
    for mode in MODES:
        pair = TdPair(dev, oracle, cap, rng.random(cap) + 0.1)
        for _ in range(2):
            td = (rng.normal(size=512) * 3).astype(np.float32)
            _, _, p = pair.update_td(np.full(512, cap - 1), td, mode)
            assert pair.ref.tree[-1] == p[-1]


@pytest.mark.parametrize("cap", [300, 8193])
def test_update_td_directed_maxima(dev, oracle, cap):
    """What a fused maximum gets wrong when it reads a leaf this launch overwrites.
    (a) the old maximum, 1e6 on one leaf, is overwritten by a small value: the maximum is the oracle's, below 1e6;
    (b) a leaf twice in one batch, |td| = 1e3 first and 0 last, every other leaf small: the maximum ignores the 1e3;
    (c) the maximum lives outside the batch on the last leaf (cap = 8193: alone in the second maximum block)."""
    last = cap - 1
    pair = TdPair(dev, oracle, cap, 0.25)                                # (a)
    pair.plant(last, 1e6)
    assert pair.ref.max_leaf() == 1e6
    idx, td = np.array([3, last, 40]), np.array([0.5, 0.1, 0.2], np.float32)
    got, want, p = pair.update_td(idx, td, "max")
    assert got == want == p[0] < 1e6 and pair.ref.tree[-1] == p[1]
    pair = TdPair(dev, oracle, cap, 0.25)                                # (b)
    idx, td = np.array([last, 5, 9, last]), np.array([1e3, 0.1, 0.2, 0.0], np.float32)
    got, want, p = pair.update_td(idx, td, "max")
    assert p[0] > 50.0 and got == want == p[2] and pair.ref.tree[-1] == p[3] < 0.25
    pair = TdPair(dev, oracle, cap, 0.25)                                # (c)
    pair.plant(last, 7.0)
    rng = np.random.default_rng(cap)
    idx, td = rng.integers(0, last, size=64), (rng.normal(size=64) * 3).astype(np.float32)
    got, want, p = pair.update_td(idx, td, "max")
    assert p.max() < 7.0 and got == want == 7.0


# ============================================================ 4. per_sample ==========================
def _sample_both(dev, oracle, cap, size, B, edge, beta, variant_b):
    from gymrl_amd import ops
    ref = oracle.SumTree(cap)
    ref.tree[:] = R.sample_tree(cap, size)
    u = R.sample_u(B, edge)
    want = ref.sample(B, size, beta, u=u, variant_b=variant_b)
    got = ops.per_sample(t(ref.tree, dev), cap, B, size, beta, ops.per_workspace(B, dev), u=t(u, dev), variant_b=variant_b)
    return [g.cpu().numpy() for g in got], want


@pytest.mark.parametrize("cap,size", R.SAMPLE_TREES)
@pytest.mark.parametrize("B", R.SAMPLE_B)
def test_sample_edges(dev, oracle, B, cap, size):
    """B = 1; B = 256 (one block: normalised inside the draw); B = 257 (the second block has one live lane and 255
    padding lanes in its maximum); B = 513.  u is exactly 0 and exactly 1 - 2^-53 in the first, a middle and the last
    stratum; beta = 0 gives weights of exactly 1; the tree is part filled (size < cap) or a full one of 2^12 + 1 leaves.
    On these inputs every sampled priority is positive (asserted on the oracle's output first)."""
    for edge in (0.0, R.U_LAST):
        for variant_b in (False, True):
            for beta in R.SAMPLE_BETA:
                (idx, prio, w), (i_ref, p_ref, w_ref) = _sample_both(dev, oracle, cap, size, B, edge, beta, variant_b)
                assert np.all(p_ref > 0.0) and np.all(np.isfinite(w_ref))
                assert np.array_equal(idx, i_ref) and np.array_equal(prio, p_ref), (edge, variant_b, beta)
                assert rel_close(w, w_ref, 1e-6) <= 1e-6, (edge, variant_b, beta)
                if beta == 0.0:
                    assert np.all(w == 1.0)


@pytest.mark.parametrize("cap,size", R.SAMPLE_TREES_EMPTY_LEAF)
@pytest.mark.parametrize("B", R.SAMPLE_B)
def test_sample_onto_an_empty_leaf_by_index(dev, oracle, B, cap, size):
    """A part-filled tree whose capacity is no power of two: v = 0 walks down the left edge to a leaf that holds nothing
    (the reference's own behaviour: priority 0, weight inf, NaN after the normalisation) — indices and priorities only."""
    for edge in (0.0, R.U_LAST):
        for variant_b in (False, True):
            (idx, prio, _), (i_ref, p_ref, _) = _sample_both(dev, oracle, cap, size, B, edge, 0.55, variant_b)
            assert np.array_equal(idx, i_ref) and np.array_equal(prio, p_ref), (edge, variant_b)
            assert edge != 0.0 or p_ref[0] == 0.0


# ============================================================ 5. per_max_leaf ========================
def test_max_leaf_grid_stride(dev):
    """cap = 2^21 + 3: the clamp engages, nb = 1024 != cdiv(cap, 2048) = 1025, and the three leaves at and past 2^21, which
    block 1025 would have read, fall to block 0's ninth turn of the stride of max_leaf_partial_kernel (the stride itself
    already runs at every cap above nb * 256 leaves).  One store of the constant 0.5 (257 sub-stores; every sum is exact, so the bottom-up tree is
    the reference whatever the order), then the maximum planted on the last leaf, the first and leaf 2^21."""
    from gymrl_amd import ops
    cap = 2 ** 21 + 3
    tree, ws = new_tree(cap, dev), ops.per_workspace(cap, dev)
    ops.per_update(tree, cap, cap, ws, idx_start=cap - 5, prio_scalar=0.5)
    ref = R.dyadic_tree(cap, 0.5)
    assert ref[0] == 0.5 * cap and np.array_equal(tree.cpu().numpy(), ref)
    mx = torch.zeros(1, dtype=torch.float64, device=dev)
    assert ops.per_max_leaf(tree, cap, mx, ws).item() == 0.5
    for leaf, value in ((cap - 1, 2.0), (0, 3.0), (2 ** 21, 4.0)):
        ops.per_update(tree, cap, 1, ws, idx=t(np.array([leaf], np.int32), dev), prio=t(np.array([value]), dev))
        node = leaf + cap - 1
        ref[node] = value
        while node:
            node = (node - 1) // 2
            ref[node] += value - 0.5
        assert ops.per_max_leaf(tree, cap, mx, ws).item() == value
    assert np.array_equal(tree.cpu().numpy(), ref)


# ============================================================ 6. n-step windows ======================
def _windows(n_steps, N, D, dev):
    return (torch.zeros(n_steps, N, D, device=dev), torch.zeros(n_steps, N, dtype=torch.int32, device=dev),
            torch.zeros(n_steps, N, device=dev), torch.zeros(n_steps, N, D, device=dev),
            torch.zeros(n_steps, N, dtype=torch.uint8, device=dev), torch.zeros(n_steps, N, dtype=torch.uint8, device=dev))


def _ring(cap, D, AW, dev):
    return (torch.zeros(cap, D, device=dev), torch.zeros(cap, AW, dtype=torch.int32, device=dev),
            torch.zeros(cap, device=dev), torch.zeros(cap, D, device=dev), torch.zeros(cap, dtype=torch.uint8, device=dev))


def same_ring(ring, ref):
    """All five ring arrays (the action words by bit pattern)."""
    want = (ref.state, ref.action, ref.reward, ref.next_state, ref.flag)
    got = [g.cpu().numpy() for g in ring]
    got[1] = got[1].view(np.uint32)
    return [k for k, (g, w) in enumerate(zip(got, want)) if g.shape != w.shape or not np.array_equal(g, w)] == []


def same_windows(win, ref):
    want = (ref.w_state, ref.w_action, ref.w_reward, ref.w_next, ref.w_terminal, ref.w_done)
    return all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(win, want))


def _push_all(dev, oracle, n_steps, N, D, inline_terminal):
    from gymrl_amd import ops
    cap, limit = 2 * N + 5, 3
    win, ring = _windows(n_steps, N, D, dev), _ring(cap, D, 1, dev)
    ref_ring, ref_win = oracle.ReplayRing(cap, D), oracle.NStepWindows(n_steps, N, D, R.NSTEP_GAMMA)
    rng = np.random.default_rng(N + n_steps)
    cursor = 0
    for p, (obs, act, rew, nxt, term, done) in enumerate(R.nstep_inputs(N, D)):
        if inline_terminal:                                              # terminal == NULL: done and not at the step limit
            ep_len = rng.integers(1, 6, size=N).astype(np.int32)
            term = (done.astype(bool) & (ep_len != limit)).astype(np.uint8)
            assert term.any() and (done.astype(bool) & (ep_len == limit)).any()
            emit = ops.nstep_push(win, n_steps, p, R.NSTEP_GAMMA, t(obs, dev), t(act, dev), t(rew, dev), t(nxt, dev), None,
                                  t(done, dev), ring, cursor, ep_len=t(ep_len, dev), max_episode_steps=limit)
        else:
            emit = ops.nstep_push(win, n_steps, p, R.NSTEP_GAMMA, t(obs, dev), t(act, dev), t(rew, dev), t(nxt, dev),
                                  t(term, dev), t(done, dev), ring, cursor)
        assert emit == ref_win.push(ref_ring, obs, act, rew, nxt, term, done) == (p + 1 >= n_steps), p
        if emit:
            cursor = (cursor + N) % cap
        assert cursor == ref_ring.cursor
        assert same_windows(win, ref_win), p
        assert same_ring(ring, ref_ring), p
    assert ref_ring.size == cap and cursor != 0                          # the ring wrapped


@pytest.mark.parametrize("D", R.NSTEP_D)
@pytest.mark.parametrize("n_steps", R.NSTEP_STEPS)
@pytest.mark.parametrize("N", R.NSTEP_N)
def test_nstep_windows_past_one_block(dev, oracle, N, n_steps, D):
    """One lane per env in 256-lane blocks: N = 256, 257 (one live lane in the second block), 600 (a partial third).
    n_steps = 1 (oldest == slot: push 0 emits), 2, 5; 12 pushes into a ring of 2N + 5 rows, which wraps; episode ends by
    replay_refs.nstep_done (windows whose oldest entry is done and windows that are all done, in the first and in the last
    block).  All six window arrays, all five ring arrays and the return value after every push."""
    _push_all(dev, oracle, n_steps, N, D, inline_terminal=False)


@pytest.mark.parametrize("n_steps", R.NSTEP_STEPS)
def test_nstep_inline_terminal(dev, oracle, n_steps):
    """terminal == NULL: the kernel forms done && ep_len != max_episode_steps itself; the oracle is handed that byte."""
    _push_all(dev, oracle, n_steps, 257, 3, inline_terminal=True)


# ============================================================ 7. the ring ============================
def _rows(rng, n, D, AW, float_actions):
    s, s2 = (rng.normal(size=(n, D)).astype(np.float32) for _ in range(2))
    a = rng.normal(size=(n, AW)).astype(np.float32) if float_actions else rng.integers(0, 1 << 30, size=(n, AW)).astype(np.int32)
    return s, a, rng.normal(size=n).astype(np.float32), s2, (rng.random(n) < 0.3).astype(np.uint8)


def _filled_ring(dev, oracle, rng, cap, D, AW, float_actions=False):
    """A device ring and the oracle's with the same random contents in every row."""
    ref = oracle.ReplayRing(cap, D, AW)
    s, a, r, s2, f = _rows(rng, cap, D, AW, float_actions)
    ref.state[:], ref.action[:], ref.reward[:], ref.next_state[:], ref.flag[:] = s, a.view(np.uint32), r, s2, f
    ring = (t(ref.state, dev), t(ref.action.view(np.int32), dev), t(ref.reward, dev), t(ref.next_state, dev), t(ref.flag, dev))
    assert same_ring(ring, ref)
    return ring, ref


def _append(dev, ring, ref, cursor, rows):
    from gymrl_amd import ops
    s, a, r, s2, f = rows
    ref.cursor = cursor
    ops.replay_append(ring, cursor, t(s, dev), t(a, dev).view(torch.int32), t(r, dev), t(s2, dev), t(f, dev))
    ref.append(s, a, r, s2, f)
    assert same_ring(ring, ref)


def _gather(dev, ring, ref, idx, action_dtype=torch.int32):
    from gymrl_amd import ops
    got = ops.replay_gather(ring, t(idx.astype(np.int32), dev), action_dtype=action_dtype)
    want = ref.gather(idx)
    assert got[1].dtype == action_dtype and got[4].dtype == torch.float32
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        g = g.view(np.uint32) if k == 1 else g
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), k


def test_ring_append_gather_strided(dev, oracle):
    """(cap, D, AW, n) = (70000, 8, 1, 65536): 65536 * 19 words > 4096 * 256 lanes, so the grid clamp of
    replay_append_kernel engages and lanes stride; from cursor 60000 the append wraps.  Then a gather of 60000 rows
    (60000 * 19 > 4096 * 256: replay_gather_kernel strides) with repeated indices, row 0 and row cap - 1, and a gather of
    one row."""
    rng = np.random.default_rng(70)
    cap, D, n = 70000, 8, 65536
    ring, ref = _filled_ring(dev, oracle, rng, cap, D, 1)
    _append(dev, ring, ref, 60000, _rows(rng, n, D, 1, False))
    assert ref.cursor == (60000 + n) % cap
    idx = rng.integers(0, cap, size=60000)
    idx[:4] = (0, cap - 1, 0, cap - 1)
    idx[-3:] = idx[100]                                                  # repeats in the strided part as well
    assert len(np.unique(idx)) < idx.size
    _gather(dev, ring, ref, idx)
    for row in (0, cap - 1, 60000):
        _gather(dev, ring, ref, np.array([row]))


def test_ring_float_action_words(dev, oracle):
    """AW = 2 float32 action words (the continuous-action trainers): appended as their int32 view, gathered as float32,
    compared by bit pattern; three appends of 96 rows from cursor 900 wrap the 1000-row ring."""
    rng = np.random.default_rng(71)
    cap, D, AW, n = 1000, 3, 2, 96
    ring, ref = _filled_ring(dev, oracle, rng, cap, D, AW, float_actions=True)
    cursor = 900
    for _ in range(3):
        rows = _rows(rng, n, D, AW, True)
        rows[1][0, 0], rows[1][1, 1] = -0.0, np.float32(np.nan)           # bit patterns, not values
        _append(dev, ring, ref, cursor, rows)
        cursor = (cursor + n) % cap
    idx = rng.integers(0, cap, size=300)
    idx[:3] = (0, cap - 1, 900)
    _gather(dev, ring, ref, idx, action_dtype=torch.float32)


def test_ring_full_overwrite(dev, oracle):
    """n == cap: one append from cursor 17 replaces every row of the 64-row ring."""
    rng = np.random.default_rng(72)
    cap, D = 64, 4
    ring, ref = _filled_ring(dev, oracle, rng, cap, D, 1)
    rows = _rows(rng, cap, D, 1, False)
    _append(dev, ring, ref, 17, rows)
    assert ref.cursor == 17 and np.array_equal(ring[2].cpu().numpy(), np.roll(rows[2], 17))
    _gather(dev, ring, ref, np.arange(cap)[::-1].copy())
