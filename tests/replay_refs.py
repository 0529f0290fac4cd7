"""Input builders and plain-Python references shared by tests/test_replay_edges.py (CPU) and tests/test_replay_edges_gpu.py.

The GPU file holds the kernels of csrc/per.hip and csrc/replay.hip to the C oracle bit for bit; the CPU file ties the
oracle, at the same cases, to the few lines of Python below, which share no code with it.  The builders are seeded and
cached read-only: both files see the same inputs."""
import functools

import numpy as np

STORE_CHUNK = 8192                       # rows per sub-store of an N-row store (per_store_device.hpp kStoreChunk)
U_LAST = 1.0 - 2.0 ** -53                # the largest double below 1
SAMPLE_B = (1, 256, 257, 513)            # one lane; one full block (normalised in the draw); one live lane in block 2; 3 blocks
SAMPLE_BETA = (0.0, 0.55, 1.0)
SAMPLE_TREES = ((1000, 300), (4097, 4097))       # (cap, size): no stratum of SAMPLE_B ends on an empty leaf
SAMPLE_TREES_EMPTY_LEAF = ((5, 3), (20, 7))      # the reference's own descent ends on empty leaves at B >= 256

NSTEP_N = (256, 257, 600)                # one full block; one lane in block 2; a partial third block
NSTEP_STEPS = (1, 2, 5)
NSTEP_D = (3, 8)
NSTEP_PUSHES = 12
NSTEP_GAMMA = 0.9


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------ sum-tree ----
def tree_sums_ok(tree, cap, n_adds):
    """Every internal node against the sum of its two children, |node - (l + r)| <= n_adds * eps * root: a node and its
    children each carry at most n_adds roundings of values bounded by the root.  Returns the worst ratio to that bound."""
    k = np.arange(cap - 1)
    err = np.abs(tree[k] - (tree[2 * k + 1] + tree[2 * k + 2]))
    bound = n_adds * np.finfo(np.float64).eps * tree[0]
    return float(err.max() / bound) if cap > 1 else 0.0


def tree_of_leaves(leaves):
    """The sum-tree over these leaf values (node k's children are 2k + 1 and 2k + 2, the leaves are the last `cap`
    nodes), every internal node formed once as left + right, deepest level first."""
    cap = len(leaves)
    tree = np.zeros(2 * cap - 1, np.float64)
    tree[cap - 1:] = leaves
    for level in range((cap - 1).bit_length(), -1, -1):                  # internal nodes are 0 .. cap - 2
        k = np.arange(2 ** level - 1, min(2 ** (level + 1) - 1, cap - 1))
        tree[k] = tree[2 * k + 1] + tree[2 * k + 2]
    return tree


def dyadic_tree(cap, value):
    """The sum-tree whose `cap` leaves all hold `value`.  With `value` a small power of two every sum is exact, so any
    order of additions gives these bits."""
    return tree_of_leaves(np.full(cap, value, np.float64))


@functools.lru_cache(maxsize=None)
def sample_tree(cap, size):
    """A tree to draw from: leaves [0, size) hold priorities in [0.1, 5), the rest are empty.  (An input, not a
    reference: any tree whose nodes are the sums of their children will do.)"""
    leaves = np.zeros(cap, np.float64)
    leaves[:size] = np.random.default_rng(7000 + cap + size).random(size) * 4.9 + 0.1
    return _frozen(tree_of_leaves(leaves))[0]


@functools.lru_cache(maxsize=None)
def sample_u(B, edge):
    """B draws in [0, 1) with `edge` (exactly 0.0 or U_LAST) in the first, a middle and the last stratum."""
    u = np.random.default_rng(7100 + B).random(B)
    for i in (0, B // 2, B - 1):
        u[i] = edge
    return _frozen(u)[0]


def sample_ref(tree, cap, u, size, beta, variant_b):
    """PrioritizedNStepBuffer.sample (rainbow_dqn_cartpole.py:228-241; ddqn_per_cartpole.py:119-138 for variant B) with
    the uniform draw made explicit, v = a + (b - a) u: indices, priorities and normalised float32 weights."""
    B = len(u)
    tcap, total = 2 * cap - 1, float(tree[0])
    segment = total / B
    idx, prio, w = np.empty(B, np.int64), np.empty(B, np.float64), np.empty(B, np.float64)
    for i in range(B):
        a, b = segment * i, segment * (i + 1)
        v = a + (b - a) * float(u[i])
        p = 0
        while 2 * p + 1 < tcap:
            left = 2 * p + 1
            if v <= tree[left]:
                p = left
            else:
                v -= tree[left]
                p = left + 1
        idx[i] = p if variant_b else p - cap + 1
        prio[i] = tree[p]
        with np.errstate(divide="ignore"):
            w[i] = np.float64(size * (prio[i] / total)) ** -beta
    with np.errstate(invalid="ignore"):                                   # (an empty leaf: inf / inf)
        if variant_b:
            return idx, prio, (w / w.max()).astype(np.float32)
        w32 = w.astype(np.float32)
        return idx, prio, w32 / w32.max()


# ------------------------------------------------------------------ n-step windows ----
def nstep_done(N, p):
    """Structured episode ends of push p: the first and the last 8 envs are done at every push, the 8 next to them never,
    env e of the rest when (e + p) % 3 == 0 — so windows whose oldest entry is done, and windows that are all done, lie
    in the first and in the last 256-lane block."""
    e = np.arange(N)
    done = ((e + p) % 3 == 0)
    done[(e < 8) | (e >= N - 8)] = True
    done[((e >= 8) & (e < 16)) | ((e >= N - 16) & (e < N - 8))] = False
    return done.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def nstep_inputs(N, D):
    """NSTEP_PUSHES pushes of N envs: (obs, action, reward, next_obs, terminal, done) per push."""
    rng = np.random.default_rng(8000 + 10 * N + D)
    out = []
    for p in range(NSTEP_PUSHES):
        obs, nxt = (rng.normal(size=(N, D)).astype(np.float32) for _ in range(2))
        act = rng.integers(0, 4, size=N).astype(np.int32)
        rew = rng.normal(size=N).astype(np.float32)
        done = nstep_done(N, p)
        term = (done & ((np.arange(N) * 7 + p) % 5 < 3)).astype(np.uint8)
        out.append(_frozen(obs, act, rew, nxt, term, done))
    return tuple(out)


class NStepRef:
    """The n-step transition that the reference's PrioritizedNStepBuffer emits (rainbow_dqn_cartpole.py:179-218), stated
    forward and for all envs at once.  Once an env has n_steps entries, its window is the last n_steps pushes; with j the
    FIRST entry whose episode ended (the last entry if none did), the emitted row is

        state, action      of entry 0
        reward             r_0 + gamma (r_1 + gamma (... + gamma r_j)), in float64, rounded once to float32
        next_state, flag   of entry j

    and the rows of one push go to ring rows (cursor + e) % cap."""

    def __init__(self, n_steps, N, D, gamma, cap):
        self.n, self.N, self.gamma, self.cap, self.cursor = n_steps, N, gamma, cap, 0
        self.history = []
        self.state, self.next_state = np.zeros((cap, D), np.float32), np.zeros((cap, D), np.float32)
        self.action, self.reward, self.flag = np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(cap, np.uint8)

    def push(self, obs, act, rew, nxt, term, done):
        self.history.append((obs, act, rew, nxt, term, done))
        if len(self.history) < self.n:
            return False
        window = self.history[-self.n:]
        envs = np.arange(self.N)
        ended = np.stack([w[5] for w in window]).astype(bool)                                # [entry, env]
        j = np.where(ended.any(axis=0), ended.argmax(axis=0), self.n - 1)                    # argmax: the first True
        rewards = np.stack([w[2] for w in window]).astype(np.float64)
        ret = rewards[j, envs]
        for k in range(self.n - 2, -1, -1):                                                  # entries before j, nearest first
            ret = np.where(k < j, rewards[k] + self.gamma * ret, ret)
        rows = (self.cursor + envs) % self.cap
        self.state[rows], self.action[rows], self.reward[rows] = window[0][0], window[0][1], ret
        self.next_state[rows] = np.stack([w[3] for w in window])[j, envs]
        self.flag[rows] = np.stack([w[4] for w in window])[j, envs]
        self.cursor = (self.cursor + self.N) % self.cap
        return True
