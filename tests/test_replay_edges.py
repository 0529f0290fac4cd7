"""The CPU twin of tests/test_replay_edges_gpu.py: the C oracle's sum-tree store, n-step window and stratified draw
against the plain Python of tests/replay_refs.py, at the cases the GPU file runs.  The GPU tests hold the kernels to the
oracle bit for bit; this file ties the oracle to something that shares no code with it."""
import numpy as np
import pytest

import replay_refs as R
from conftest import rel_close


# ------------------------------------------------------------------ the N-row store past one chunk ----
@pytest.mark.parametrize("cap,n,start,scalar", [(20000, 8193, 123, None), (20000, 16384, 19000, None),
                                                (20000, 20000, 15000, None), (16384, 16384, 1, 2.5)])
def test_store_chunks_are_consecutive_stores(oracle, cap, n, start, scalar):
    """update_many(idx_start = s, n rows) == one update_many per 8192 rows, in order (rule 4 of the store's definition,
    oracle/offpolicy_oracle.c), bit for bit and from a tree that is not empty; after the store and after an explicit
    update of 300 indices every internal node is the sum of its children to n * eps * root."""
    rng = np.random.default_rng(cap + n)
    one, parts = oracle.SumTree(cap), oracle.SumTree(cap)
    first = rng.random(cap) + 0.5
    for tr in (one, parts):
        tr.update_many(idx=np.arange(cap, dtype=np.int32), prio=first)
    assert np.array_equal(one.tree, parts.tree)
    prio = None if scalar is not None else rng.random(n) * 3 + 1e-3
    one.update_many(idx_start=start, prio=prio, prio_scalar=scalar or 0.0, B=n)
    sizes = []
    for o in range(0, n, R.STORE_CHUNK):
        m = min(R.STORE_CHUNK, n - o)
        sizes.append(m)
        parts.update_many(idx_start=(start + o) % cap, prio=None if prio is None else prio[o:o + m], prio_scalar=scalar or 0.0, B=m)
    if n == 20000:
        assert sizes == [8192, 8192, 3616]
    assert len(sizes) >= 2 and np.array_equal(one.tree, parts.tree)
    rows = (start + np.arange(n)) % cap                                  # the leaves: the rows' priorities, the others untouched
    want = first.copy()
    want[rows] = scalar if scalar is not None else prio
    assert np.array_equal(one.tree[cap - 1:], want)
    assert R.tree_sums_ok(one.tree, cap, cap + n) <= 1.0
    idx = rng.integers(0, cap, size=300).astype(np.int32)
    one.update_many(idx=idx, prio=rng.random(300) * 3 + 1e-3)
    assert R.tree_sums_ok(one.tree, cap, cap + n + 300) <= 1.0


def test_store_of_a_dyadic_constant_is_exact(oracle):
    """Priorities 0.5 on every leaf: all sums are exact, so the oracle's store equals the bottom-up tree whatever the
    order — the reference tests/test_replay_edges_gpu.py uses at cap = 2^21 + 3, where the oracle's store is slow."""
    for cap in (1, 2, 3, 5, 4097, 20000):
        tr = oracle.SumTree(cap)
        tr.update_many(idx_start=cap // 3, prio_scalar=0.5, B=cap)
        assert np.array_equal(tr.tree, R.dyadic_tree(cap, 0.5)) and tr.tree[0] == 0.5 * cap


# ------------------------------------------------------------------ update_priorities from TD errors ----
def test_priorities_clip_and_directed_maxima(oracle):
    """per_priorities with a clip against float64 min(|td| + eps, clip) ** alpha on both sides of the clip, and the two
    directed sequences of the GPU file on the oracle: the planted maximum is gone once its leaf is overwritten, and a
    duplicated leaf ends at its LAST element's priority."""
    td = np.array([0.0, -0.3, 0.98, 0.99, 1.0, -1.5, 40.0, -1e6], np.float32)
    alpha, eps, clip = 0.6, 0.01, 1.0
    got = oracle.per_priorities(td, alpha, eps, clip)
    want = np.minimum(np.abs(td.astype(np.float64)) + eps, clip) ** alpha
    assert rel_close(got, want, 1e-6) <= 1e-6 and np.all(got[4:] == 1.0) and np.all(got[:3] < 1.0)
    cap = 300
    tr = oracle.SumTree(cap)
    tr.update_many(idx_start=0, prio_scalar=0.25, B=cap)
    tr.update(17, 1e6)
    assert tr.max_leaf() == 1e6
    idx = np.array([3, 17, 40], np.int32)
    p = oracle.per_priorities(np.array([0.5, 0.1, 0.2], np.float32), alpha, eps)
    tr.update_many(idx=idx, prio=p)
    assert tr.max_leaf() == p.max() < 1e6
    idx = np.array([9, 5, 9], np.int32)
    p = oracle.per_priorities(np.array([1e3, 0.0, 0.0], np.float32), alpha, eps)
    tr.update_many(idx=idx, prio=p)
    assert tr.tree[cap - 1 + 9] == p[2] and p[0] > 50 and tr.max_leaf() < 1.0


# ------------------------------------------------------------------ n-step windows ----
def test_done_patterns_reach_both_blocks():
    """What the structured pattern is for: with 5-entry windows over pushes 4 .. 11, windows whose oldest entry is done
    but not all, windows that are all done and windows with no done lie in lanes 0 .. 255 and in the last block."""
    for N in R.NSTEP_N:
        done = np.stack([R.nstep_done(N, p) for p in range(R.NSTEP_PUSHES)]).astype(bool)      # [push, env]
        blocks = [np.arange(min(N, 256)), np.arange(256 * ((N - 1) // 256), N)]
        for n in R.NSTEP_STEPS:
            oldest = alld = none = np.zeros(N, bool)
            for p in range(n - 1, R.NSTEP_PUSHES):
                w = done[p - n + 1:p + 1]
                oldest = oldest | (w[0] & ~w.all(0))
                alld = alld | w.all(0)
                none = none | ~w.any(0)
            for lanes in blocks:
                assert alld[lanes].any()
                if len(lanes) >= 64:                                     # (N = 257: the last block is the one always-done env)
                    assert none[lanes].any() and (n == 1 or oldest[lanes].any())


@pytest.mark.parametrize("N", R.NSTEP_N)
@pytest.mark.parametrize("n_steps", R.NSTEP_STEPS)
def test_nstep_oracle_vs_forward_rule(oracle, n_steps, N):
    """orc_nstep_push (a backward recursion over the window, one env at a time) == the n-step rule stated forward in
    replay_refs.NStepRef (first ended entry, discounted sum up to it): every ring array after every push, and the emit
    flag (n_steps = 1 emits on push 0)."""
    D, cap = 3, 2 * N + 5
    ring, win = oracle.ReplayRing(cap, D), oracle.NStepWindows(n_steps, N, D, R.NSTEP_GAMMA)
    ref = R.NStepRef(n_steps, N, D, R.NSTEP_GAMMA, cap)
    for p, (obs, act, rew, nxt, term, done) in enumerate(R.nstep_inputs(N, D)):
        emit = win.push(ring, obs, act, rew, nxt, term, done)
        assert emit == ref.push(obs, act, rew, nxt, term, done) == (p + 1 >= n_steps)
        assert np.array_equal(ring.state, ref.state) and np.array_equal(ring.next_state, ref.next_state)
        assert np.array_equal(ring.action.view(np.int32)[:, 0], ref.action) and np.array_equal(ring.flag, ref.flag)
        assert np.array_equal(ring.reward, ref.reward), p
        assert ring.cursor == ref.cursor
    assert ring.cursor != 0 and ring.size == cap                          # 12 pushes of N rows wrapped the ring


# ------------------------------------------------------------------ the stratified draw ----
@pytest.mark.parametrize("cap,size", R.SAMPLE_TREES)
@pytest.mark.parametrize("B", R.SAMPLE_B)
def test_sample_inputs_are_well_posed(oracle, B, cap, size):
    """The condition under which the GPU file compares weights: on these trees, with u = 0 and u = 1 - 2^-53 in the first,
    a middle and the last stratum, every sampled priority is positive and every weight finite; and the oracle's draw is
    replay_refs.sample_ref's stratified descent in Python (indices and priorities exact, weights to 1e-6)."""
    tr = oracle.SumTree(cap)
    tr.tree[:] = R.sample_tree(cap, size)
    for edge in (0.0, R.U_LAST):
        u = R.sample_u(B, edge)
        assert u[0] == u[B // 2] == u[-1] == edge
        for variant_b in (False, True):
            for beta in R.SAMPLE_BETA:
                idx, prio, w = tr.sample(B, size, beta, u=u, variant_b=variant_b)
                assert np.all(prio > 0.0) and np.all(np.isfinite(w)) and w.max() == 1.0
                i_ref, p_ref, w_ref = R.sample_ref(tr.tree, cap, u, size, beta, variant_b)
                assert np.array_equal(idx, i_ref) and np.array_equal(prio, p_ref)
                assert rel_close(w, w_ref, 1e-6) <= 1e-6
                if beta == 0.0:
                    assert np.all(w == 1.0)
                data = idx - (cap - 1) if variant_b else idx
                assert data.min() >= 0 and data.max() < size


@pytest.mark.parametrize("cap,size", R.SAMPLE_TREES_EMPTY_LEAF)
def test_sample_of_a_part_filled_tree_can_end_on_an_empty_leaf(oracle, cap, size):
    """The reference's behaviour that the GPU file compares by index only: a partly filled tree of a capacity that is no
    power of two sends v = 0 down the left edge to a leaf that holds nothing (priority 0, weight inf)."""
    tr = oracle.SumTree(cap)
    tr.tree[:] = R.sample_tree(cap, size)
    for B in R.SAMPLE_B:
        u = R.sample_u(B, 0.0)
        idx, prio, _ = tr.sample(B, size, 0.55, u=u)
        i_ref, p_ref, _ = R.sample_ref(tr.tree, cap, u, size, 0.55, False)
        assert np.array_equal(idx, i_ref) and np.array_equal(prio, p_ref)
        assert prio[0] == 0.0 and idx[0] >= size
