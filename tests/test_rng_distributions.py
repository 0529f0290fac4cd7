"""The in-kernel random draws against the distributions the reference's calls promise.

The bit-exact tests pin every kernel's draw to the oracle's restatement of the same Philox and the same mapping, and the
trainer traces inject the reference's own draws; neither sees a draw whose DESIGN is off.  Here each draw the product
uses is compared with its exact law (float64 or exact combinatorics): random.sample / np.random.shuffle (keyed
permutation), np.random.uniform (PER strata, env resets), torch.randn (Box-Muller), Categorical and epsilon-greedy.

Most tests run twice: on the CPU oracle and, marked gpu, on the kernels through gymrl_amd.ops.  The exceptions: the
2^23 shuffle and SAC's fused acting draw are GPU-only (too slow on the oracle / no oracle form), the small-domain
co-membership sweep is oracle-only (the GPU's bits at those sizes are pinned to the oracle's by
test_keyed_permutation_bit_exact_at_the_construction_switches).  Seeds and counters are fixed, so a pass is deterministic.
Thresholds sit at p = 1e-6 of the statistic's law (chi-square by Wilson-Hilferty, normal and Kolmogorov tails in closed
form) where that law is exact or asymptotic; the few statistics whose null variance is only bounded say so where they
are used, and there the limit is set on the conservative side of the bound.
"""
import math

import numpy as np
import pytest

P_FAIL = 1e-6
BACKENDS = [pytest.param("cpu"), pytest.param("gpu", marks=pytest.mark.gpu)]


# ------------------------------------------------------------- thresholds ---
def normal_upper(p):
    """z with P(N(0,1) > z) = p (bisection on erfc)."""
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(mid / math.sqrt(2.0)) > p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


Z1 = normal_upper(P_FAIL)          # one-sided
Z2 = normal_upper(P_FAIL / 2)      # two-sided


def chi2_limit(df):
    """Upper p = 1e-6 quantile of chi-square(df), Wilson-Hilferty."""
    h = 2.0 / (9.0 * df)
    return df * (1.0 - h + Z1 * math.sqrt(h)) ** 3


def ks_limit(n):
    """D_n above which P < 1e-6 (Kolmogorov's limit law, 2 exp(-2 n d^2))."""
    return math.sqrt(-math.log(P_FAIL / 2.0) / (2.0 * n))


def chi2(counts, expected, min_expected=5.0):
    """Pearson's statistic and degrees of freedom; cells expected below min_expected are pooled into one."""
    counts = np.asarray(counts, np.float64).ravel()
    expected = np.asarray(expected, np.float64).ravel()
    small = expected < min_expected
    if small.any():
        counts = np.append(counts[~small], counts[small].sum())
        expected = np.append(expected[~small], expected[small].sum())
        if expected[-1] == 0.0:
            counts, expected = counts[:-1], expected[:-1]
    return float(((counts - expected) ** 2 / expected).sum()), len(expected) - 1


def assert_chi2(counts, expected, what, constraints=1):
    stat, cells = chi2(counts, expected)
    df = cells - (constraints - 1)
    assert stat < chi2_limit(df), f"{what}: chi2 = {stat:.1f} on {df} df (limit {chi2_limit(df):.1f})"


def ks_stat(x, cdf):
    x = np.sort(np.asarray(x, np.float64))
    n = len(x)
    F = cdf(x)
    return float(max((np.arange(1, n + 1) / n - F).max(), (F - np.arange(n) / n).max()))


def normal_cdf(x):
    import torch
    return (0.5 * torch.erfc(-torch.from_numpy(np.asarray(x, np.float64)) / math.sqrt(2.0))).numpy()


def assert_standard_normal(x, what):
    """KS against N(0,1) in float64, plus the mean, variance and excess kurtosis to their sampling sd."""
    x = np.asarray(x, np.float64).ravel()
    n = len(x)
    D = ks_stat(x, normal_cdf)
    assert D < ks_limit(n), f"{what}: KS D = {D:.5f} (limit {ks_limit(n):.5f}, n = {n})"
    m, v = x.mean(), x.var()
    k = ((x - m) ** 4).mean() / v ** 2 - 3.0
    assert abs(m) < Z2 * math.sqrt(1.0 / n), (what, "mean", m)
    assert abs(v - 1.0) < Z2 * math.sqrt(2.0 / n), (what, "variance", v)
    assert abs(k) < Z2 * math.sqrt(24.0 / n), (what, "excess kurtosis", k)


def assert_uncorrelated(a, b, what):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    r = float(np.corrcoef(a, b)[0, 1])
    assert abs(r) < Z2 / math.sqrt(len(a)), f"{what}: correlation {r:.5f} over {len(a)}"


def assert_uniform(x, lo, hi, what):
    x = np.asarray(x, np.float64).ravel()
    assert x.min() >= lo and x.max() <= hi, (what, x.min(), x.max())
    D = ks_stat(x, lambda t: (t - lo) / (hi - lo))
    assert D < ks_limit(len(x)), f"{what}: KS D = {D:.5f} (limit {ks_limit(len(x)):.5f})"


# --------------------------------------------------------------- backends ---
class Cpu:
    def __init__(self, orc):
        self.orc = orc

    def permutations(self, seed, counters, M):
        return np.stack([self.orc.permutation(seed, int(c), M) for c in counters])

    def uniform_indices(self, seed, counters, size, B):
        return np.stack([self.orc.uniform_indices(seed, int(c), size, B) for c in counters])

    def categorical(self, logits, seed, counter, env_id0=0):
        return self.orc.categorical_sample(logits, seed=seed, counter=counter, env_id0=env_id0)[0]

    def epsilon_greedy(self, q, eps, seed, counter):
        return self.orc.epsilon_greedy(q, eps, seed=seed, counter=counter)

    def noisy_noise(self, nin, nout, seed, counter):
        return self.orc.noisy_noise(nin, nout, seed=seed, counter=counter)

    def noisy_action(self, n, seed, counter):
        return self.orc.noisy_action(np.zeros(n, np.float32), 1.0, 1e30, seed=seed, counter=counter)

    def reset(self, kind, n, seed):
        return self.orc.Env(kind, n, seed=seed).reset()

    def resets(self, kind, n, seed):
        """(episode 0 of envs 0..n-1, their episode 1, episode 0 of envs n..2n-1 through env_id0 = n)"""
        env = self.orc.Env(kind, n, seed=seed)
        o0 = env.reset()
        act = np.zeros(n, np.int32) if kind == 0 else np.zeros((n, 1), np.float32)
        o1, flag, _, _ = env.abandon(1, env.step(act)["obs"])      # one step, then a cap of 1: every env restarts
        assert flag.all()
        return o0, o1, self.orc.Env(kind, n, seed=seed, env_id0=n).reset()

    def per(self, prio, cap):
        tree = self.orc.SumTree(cap)
        tree.update_many(idx=np.arange(len(prio)), prio=prio)
        return lambda B, size, beta, seed, counter: tree.sample(B, size, beta, seed=seed, counter=counter), tree.tree[0]


class Gpu:
    def __init__(self):
        import torch
        from gymrl_amd import ops
        if not (torch.cuda.is_available() and ops.device_ok()):
            pytest.fail("gpu test without a usable MI355X")
        self.torch, self.ops, self.dev = torch, ops, torch.device("cuda:0")

    def permutations(self, seed, counters, M):
        buf = self.torch.empty(len(counters), M, dtype=self.torch.int32, device=self.dev)
        for k, c in enumerate(counters):
            self.ops.permutation(seed, int(c), M, self.dev, out=buf[k])
        return buf.cpu().numpy()

    def uniform_indices(self, seed, counters, size, B):
        buf = self.torch.empty(len(counters), B, dtype=self.torch.int32, device=self.dev)
        for k, c in enumerate(counters):
            self.ops.uniform_indices(seed, int(c), size, B, self.dev, out=buf[k])
        return buf.cpu().numpy()

    def categorical(self, logits, seed, counter, env_id0=0):
        lg = self.torch.from_numpy(np.ascontiguousarray(logits, np.float32)).to(self.dev)
        return self.ops.categorical_sample(lg, seed=seed, counter=counter, env_id0=env_id0)[0].cpu().numpy()

    def epsilon_greedy(self, q, eps, seed, counter):
        qd = self.torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(self.dev)
        return self.ops.epsilon_greedy(qd, eps, seed=seed, counter=counter).cpu().numpy()

    def noisy_noise(self, nin, nout, seed, counter):
        w = self.torch.empty(nout, nin, device=self.dev)
        b = self.torch.empty(nout, device=self.dev)
        self.ops.noisy_noise(nin, nout, w, b, seed=seed, counter=counter)
        return w.cpu().numpy(), b.cpu().numpy()

    def noisy_action(self, n, seed, counter):
        mu = self.torch.zeros(n, device=self.dev)
        return self.ops.noisy_action(mu, 1.0, 1e30, seed=seed, counter=counter).cpu().numpy()

    def reset(self, kind, n, seed):
        state = self.ops.env_state(kind, n, self.dev)
        obs = self.torch.empty(n, {0: 4, 1: 3, 2: 8}[kind], device=self.dev)
        self.ops.env_reset(kind, state, n, seed, 0, obs)
        return obs.cpu().numpy()

    def resets(self, kind, n, seed):
        torch = self.torch
        from gymrl_amd.envs import VecEnv
        name = {0: "CartPole-v1", 1: "Pendulum-v1"}[kind]
        env = VecEnv(name, n, device=self.dev, seed=seed)
        o0 = env.reset().clone()
        o1, rew = torch.empty_like(o0), torch.empty(n, device=self.dev)
        act = (torch.zeros(n, dtype=torch.int32, device=self.dev) if kind == 0
               else torch.zeros(n, 1, device=self.dev))
        env.step(act, o1, rew)
        flag = torch.zeros(n, dtype=torch.uint8, device=self.dev)
        env.abandon(1, o1, flag)                                        # one step, then a cap of 1: every env restarts
        assert bool(flag.all())
        off = VecEnv(name, n, device=self.dev, seed=seed, env_id0=n).reset()
        return o0.cpu().numpy(), o1.cpu().numpy(), off.cpu().numpy()

    def per(self, prio, cap):
        torch, ops = self.torch, self.ops
        tree = torch.zeros(2 * cap - 1, dtype=torch.float64, device=self.dev)
        ws = ops.per_workspace(8192, self.dev)
        ops.per_update(tree, cap, len(prio), ws, idx=torch.arange(len(prio), dtype=torch.int32, device=self.dev),
                       prio=torch.from_numpy(prio).to(self.dev))

        def sample(B, size, beta, seed, counter):
            return (x.cpu().numpy() for x in ops.per_sample(tree, cap, B, size, beta, ws, seed=seed, counter=counter))
        return sample, float(tree[0].item())


@pytest.fixture
def draw(request, oracle):
    return Cpu(oracle) if request.param == "cpu" else Gpu()


def backends(fn):
    return pytest.mark.parametrize("draw", BACKENDS, indirect=True)(fn)


# ------------------------------------------------------------------ Philox ---
def test_philox_known_answers(oracle):
    """Philox4x32-10, the generator every draw here rests on, against the Random123 known-answer vectors."""
    assert list(oracle.philox(0, 0, 0, 0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFF
    assert list(oracle.philox((ones << 32) | ones, ones, ones, ones, ones)) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6,
                                                                                   0x6D5451FD]
    assert list(oracle.philox((0x299F31D0 << 32) | 0xA4093822, 0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344)) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


# ----------------------------------------------------- keyed permutation ---
def _sizes_around_powers():
    return sorted({m for k in range(2, 17) for m in ((1 << k) - 1, 1 << k, (1 << k) + 1)} | set(range(1, 301)))


@backends
def test_permutation_is_a_bijection_at_every_size(draw):
    """gymrl_permutation is a bijection of [0, M) for M = 1..300 and around every power of two up to 2^16 (the
    Fisher-Yates / Feistel switch between 16 and 17, the 12 / 6 round switch between 512 and 513, the cycle walk above
    2^k)."""
    for M in _sizes_around_powers():
        p = draw.permutations(11, [5], M)[0]
        assert np.array_equal(np.sort(p), np.arange(M)), M


@backends
@pytest.mark.parametrize("M", [3, 5, 6, 9, 17, 100])
def test_permutation_position_by_value(draw, M):
    """np.random.shuffle: every value equally likely at every position, over consecutive counters.  The position x
    value table of a uniform permutation has (M - 1)^2 degrees of freedom."""
    N = 20000
    p = draw.permutations(3, range(N), M)
    counts = np.zeros((M, M))
    for pos in range(M):
        counts[pos] = np.bincount(p[:, pos], minlength=M)
    assert_chi2(counts, np.full((M, M), N / M), f"permutation M={M} position x value", constraints=2 * M - 1)
    if M > 17:
        return
    # the first two positions jointly: an ordered pair of distinct values, uniform over M (M - 1) cells
    pair = np.bincount(p[:, 0] * M + p[:, 1], minlength=M * M).reshape(M, M)
    off = ~np.eye(M, dtype=bool)
    assert_chi2(pair[off], np.full(off.sum(), N / (M * (M - 1))), f"permutation M={M} (perm[0], perm[1])")


def _co_membership(pos, pairs_a, pairs_b, blocks):
    """Fraction of row pairs (a, b) whose positions fall into the same of `blocks` equal slices."""
    M = pos.shape[-1]
    shift = (M // blocks).bit_length() - 1
    return float(((pos[..., pairs_a] >> shift) == (pos[..., pairs_b] >> shift)).mean())


def _assert_co_membership(pos, blocks, what):
    """Rows i, j of a uniform permutation of M = 2^k land in the same of `blocks` minibatches with probability
    (M / blocks - 1) / (M - 1), for every fixed pair — here the structured ones a Feistel network could favour: i and
    i + 1, i and i ^ 1, and i and i ^ 2^(a-1) / i ^ 2^a (the top bit of the low Feistel half / the low bit of the
    high one, so the pair shares the other half)."""
    n_perm, M = pos.shape
    bits = M.bit_length() - 1
    a = bits // 2
    q = (M / blocks - 1) / (M - 1)
    i = np.arange(M)
    for name, j in (("i+1", i + 1), ("i^1", i ^ 1), ("i^2^(a-1)", i ^ (1 << (a - 1))), ("i^2^a", i ^ (1 << a))):
        keep = (j < M) & (j > i)
        f = _co_membership(pos, i[keep], j[keep], blocks)
        n = n_perm * keep.sum()
        # pairs of one permutation are not independent; the i + 1 pairs overlap, so the count's variance is bounded by
        # twice the binomial one (adjacent pairs' indicators are nearly uncorrelated), not equal to it
        sd = math.sqrt(2.0 * q * (1 - q) / n)
        assert abs(f - q) < Z2 * sd, f"{what} {name}: co-membership {f:.6f} vs {q:.6f} (sd {sd:.2e})"


@pytest.mark.gpu
def test_permutation_minibatch_co_membership_at_rollout_size():
    """PPO's epoch shuffle at the rollout size (M = 2^23, 32 minibatches): structured pairs of rows share a minibatch
    with the probability of a uniform shuffle."""
    g = Gpu()
    torch = g.torch
    M, n_perm = 1 << 23, 4
    pos = np.empty((n_perm, M), np.int32)
    for c in range(n_perm):
        perm = g.ops.permutation(3, (1 << 40) + c, M, g.dev)
        inv = torch.empty_like(perm)
        inv[perm.long()] = torch.arange(M, dtype=torch.int32, device=g.dev)     # row -> position
        pos[c] = inv.cpu().numpy()
    _assert_co_membership(pos, 32, "M=2^23")


def test_permutation_minibatch_co_membership_small(oracle):
    """The same law at 2^6 .. 2^12 on the oracle, where a 6-round Feistel network was measurably off."""
    for bits, n_perm in ((6, 20000), (8, 4000), (10, 1000), (12, 200)):
        p = Cpu(oracle).permutations(3, range(n_perm), 1 << bits)
        pos = np.argsort(p, axis=1).astype(np.int32)
        _assert_co_membership(pos, 32, f"M=2^{bits}")


# ---------------------------------------------------------- replay sample ---
@backends
def test_uniform_indices_distinct_and_whole_set(draw):
    for size, B in ((1, 1), (2, 2), (5, 3), (16, 16), (17, 17), (33, 8), (1000, 64), (1 << 20, 256)):
        idx = draw.uniform_indices(7, range(40), size, B)
        assert idx.min() >= 0 and idx.max() < size, size
        assert all(len(set(r.tolist())) == B for r in idx), size
        if B == size:
            assert all(np.array_equal(np.sort(r), np.arange(size)) for r in idx), size


@backends
@pytest.mark.parametrize("size", [4, 5, 8, 16, 33])
def test_uniform_indices_ordered_pair(draw, size):
    """random.sample(buffer, 2): the ordered pair is uniform over the size (size - 1) pairs of distinct rows."""
    N = 20000
    idx = draw.uniform_indices(7, range(N), size, 2)
    pair = np.bincount(idx[:, 0] * size + idx[:, 1], minlength=size * size).reshape(size, size)
    off = ~np.eye(size, dtype=bool)
    assert pair[~off].sum() == 0
    assert_chi2(pair[off], np.full(off.sum(), N / (size * (size - 1))), f"uniform_indices size={size} ordered pair")


@backends
@pytest.mark.parametrize("size,B,N", [(1000, 64, 2000), (4097, 256, 1000), (1 << 20, 512, 4000)])
def test_uniform_indices_marginals(draw, size, B, N):
    """Every row equally likely to be drawn; at 2^20, structured pairs of rows drawn together as often as in a uniform
    sample without replacement."""
    idx = draw.uniform_indices(5, range(N), size, B)
    counts = np.bincount(idx.ravel(), minlength=size)
    # each row appears at most once per draw: the count is a sum of N Bernoulli(B / size), var N p (1 - p); the
    # normalised sum is chi-square-like on size - 1 df, with heavier tails than that when N p is small (2^20: N p ~ 2),
    # so at 2^20 the limit's real tail is nearer 1e-5 than 1e-6 — still deterministic with the fixed seeds
    p = B / size
    stat = float(((counts - N * p) ** 2).sum() / (N * p * (1 - p)))
    assert stat < chi2_limit(size - 1), f"size={size}: marginal chi2 {stat:.1f} on {size - 1} df"
    if size == 1 << 20:
        # replay at 2^20: a drawn row's structured neighbour (i ^ 1, i ^ 2^9 across the low Feistel half's top bit,
        # i ^ 2^10 across the high half's low bit) is drawn with it with probability (B - 1) / (size - 1); each
        # unordered pair is met twice, so the total is ~ 2 Poisson(N B (B - 1) / (2 (size - 1)))
        for flip in (1, 1 << 9, 1 << 10):
            hits = sum(int(np.isin(r ^ flip, r, assume_unique=True).sum()) for r in idx)
            lam = N * B * (B - 1) / (size - 1)
            assert abs(hits - lam) < Z2 * math.sqrt(2.0 * lam), (flip, hits, lam)


@pytest.mark.gpu
def test_uniform_indices_device_cursor_matches_host():
    """The device-cursor form (dev = {counter, size}) draws the host form's bits, on both sides of the Fisher-Yates /
    Feistel and round-count switches."""
    import struct
    g = Gpu()
    torch = g.torch
    for size in (1, 3, 16, 17, 100, 1023, 1024, 5000, 1 << 20):
        B = min(size, 64)
        host = g.ops.uniform_indices(5, 12345, size, B, g.dev)
        blob = torch.frombuffer(bytearray(struct.pack("Qq", 12345, size)), dtype=torch.uint8).to(g.dev)
        dev = g.ops.uniform_indices(5, 0, 1 << 20, B, g.dev, dev=blob)
        assert torch.equal(host, dev), size


# ---------------------------------------------------------------- PER draw ---
@backends
def test_per_sample_leaf_frequencies_and_weights(draw):
    """Stratified PER draw with in-kernel uniforms: over many counters, leaf frequency proportional to priority
    (priorities spanning 1e-6 .. 1e3, zero leaves, size < cap); zero leaves and leaves at or past `size` never drawn;
    IS weights (N P)^-beta / max recomputed in float64."""
    cap, size, B, beta, N = 1024, 1000, 4096, 0.4, 200
    rng = np.random.default_rng(21)
    prio = np.exp(rng.uniform(math.log(1e-6), math.log(1e3), size))
    prio[rng.choice(size, 50, replace=False)] = 0.0
    sample, total = draw.per(prio, cap)
    counts = np.zeros(cap)
    for c in range(N):
        idx, pr, w = sample(B, size, beta, 17, c)
        assert idx.min() >= 0 and idx.max() < size, c
        assert np.array_equal(pr, prio[idx]), c
        counts += np.bincount(idx, minlength=cap)
        want = (size * pr / total) ** -beta
        want = want / want.max()
        assert np.max(np.abs(w - want) / want) < 1e-6, c
    assert counts[size:].sum() == 0 and counts[:size][prio == 0].sum() == 0
    expected = np.append(N * B * prio / total, np.zeros(cap - size))
    # stratification makes the counts LESS variable than multinomial ones: the chi-square limit is conservative
    pos = expected > 0
    assert_chi2(counts[pos], expected[pos], "PER leaf frequency")


# ---------------------------------------------------------- Gaussian draws ---
@backends
def test_noisy_noise_streams_are_standard_normal(draw):
    """NoisyLinear's factorised noise: f^-1(y) = sign(y) y^2 of bias_epsilon recovers the N(0,1) draws of stream 1
    (output side); w_eps[0, :] / f(out_0) those of stream 0 (input side).  Both standard normal, the two streams and
    consecutive elements uncorrelated."""
    n = 1 << 18 if isinstance(draw, Cpu) else 1 << 20
    _, b = draw.noisy_noise(1, n, seed=9, counter=4)
    out_side = np.sign(b.astype(np.float64)) * b.astype(np.float64) ** 2
    w, b1 = draw.noisy_noise(n, 1, seed=9, counter=4)
    f_in = w[0].astype(np.float64) / float(b1[0])
    in_side = np.sign(f_in) * f_in ** 2
    assert_standard_normal(out_side, "noisy_noise stream 1")
    assert_standard_normal(in_side, "noisy_noise stream 0")
    assert_uncorrelated(in_side, out_side, "streams 0 / 1, same element")
    assert_uncorrelated(out_side[:-1], out_side[1:], "stream 1, consecutive elements")
    _, b2 = draw.noisy_noise(1, n, seed=9, counter=5)
    assert_uncorrelated(b, b2, "stream 1, consecutive counters")


@backends
def test_noisy_action_stream_is_standard_normal(draw):
    """Gaussian exploration noise (stream 2): mu = 0, std = 1, no clipping gives the raw draws."""
    n = 1 << 18 if isinstance(draw, Cpu) else 1 << 20
    x = draw.noisy_action(n, seed=13, counter=2)
    assert_standard_normal(x, "noisy_action stream 2")
    assert_uncorrelated(x[:-1], x[1:], "stream 2, consecutive elements")
    assert_uncorrelated(x, draw.noisy_action(n, seed=13, counter=3), "stream 2, consecutive counters")
    _, b = draw.noisy_noise(1, n, seed=13, counter=2)
    assert_uncorrelated(x, np.sign(b) * b.astype(np.float64) ** 2, "streams 1 / 2, same counter")


# ------------------------------------------------------------- Categorical ---
def _softmax64(logits):
    z = np.asarray(logits, np.float64)
    e = np.exp(z - z.max())
    return e / e.sum()


@backends
@pytest.mark.parametrize("A", [2, 3, 4, 6, 8])
def test_categorical_frequencies_match_softmax(draw, A):
    rng = np.random.default_rng(A)
    n = 200000
    for logits in (rng.normal(size=A) * 2.0, np.linspace(0.0, -math.log(1e5), A), 80.0 * np.sign(rng.normal(size=A))
                   + rng.normal(size=A)):
        logits = logits.astype(np.float32)
        act = draw.categorical(np.tile(logits, (n, 1)), seed=31, counter=A)
        assert act.min() >= 0 and act.max() < A
        p = _softmax64(logits)
        assert_chi2(np.bincount(act, minlength=A), n * p, f"categorical A={A} logits={logits}")


@backends
def test_categorical_draws_independent_across_envs(draw):
    """Envs env_id0 + i and env_id0 + i + 1 of one launch, and one env at consecutive counters: the joint action table
    is the product of the marginals."""
    A, n = 4, 200000
    logits = np.tile(np.array([0.3, -0.2, 1.1, 0.0], np.float32), (n, 1))
    p = _softmax64(logits[0])
    a = draw.categorical(logits, seed=8, counter=3, env_id0=1000)
    for x, y, what in ((a[0::2], a[1::2], "neighbouring envs"),
                       (a, draw.categorical(logits, seed=8, counter=4, env_id0=1000), "consecutive counters")):
        joint = np.bincount(x * A + y, minlength=A * A)
        assert_chi2(joint, len(x) * np.outer(p, p).ravel(), what)


# ---------------------------------------------------------- epsilon-greedy ---
@backends
@pytest.mark.parametrize("A,eps", [(2, 0.1), (3, 0.5), (6, 0.9)])
def test_epsilon_greedy_rates(draw, A, eps):
    """P(greedy) = (1 - eps) + eps / A; the non-greedy actions uniform."""
    n = 400000
    q = np.zeros((n, A), np.float32)
    q[:, A - 1] = 1.0
    act = draw.epsilon_greedy(q, eps, seed=4, counter=11)
    p = np.full(A, eps / A)
    p[A - 1] += 1.0 - eps
    assert_chi2(np.bincount(act, minlength=A), n * p, f"epsilon-greedy A={A} eps={eps}")


# -------------------------------------------------------------- env resets ---
@backends
def test_classic_resets_are_uniform(draw):
    """CartPole: U(-0.05, 0.05)^4; Pendulum: theta ~ U(-pi, pi), theta_dot ~ U(-1, 1).  Neighbouring envs, the coordinates
    of one env, an env's first and second episode (VecEnv on the GPU: reset, one step, then every env restarted by a
    step cap of 1) and envs reached
    through an env_id0 offset: uncorrelated, each uniform."""
    n = 1 << 16 if isinstance(draw, Cpu) else 1 << 18
    s = draw.reset(0, n, seed=12)
    for k in range(4):
        assert_uniform(s[:, k], -0.05, 0.05, f"CartPole state[{k}]")
        assert_uncorrelated(s[:-1, k], s[1:, k], f"CartPole state[{k}], neighbouring envs")
    for k in range(3):
        assert_uncorrelated(s[:, k], s[:, k + 1], f"CartPole state[{k}] / [{k + 1}]")
    o = draw.reset(1, n, seed=12).astype(np.float64)
    th = np.arctan2(o[:, 1], o[:, 0])
    assert_uniform(th, -math.pi, math.pi, "Pendulum theta")
    assert_uniform(o[:, 2], -1.0, 1.0, "Pendulum theta_dot")
    assert_uncorrelated(th, o[:, 2], "Pendulum theta / theta_dot")
    assert_uncorrelated(th[:-1], th[1:], "Pendulum theta, neighbouring envs")
    s2 = draw.reset(0, n, seed=13)
    assert_uncorrelated(s[:, 0], s2[:, 0], "CartPole, neighbouring seeds")
    for kind, name in ((0, "CartPole"), (1, "Pendulum")):
        e0, e1, off = draw.resets(kind, n, seed=12)
        assert np.array_equal(e0, draw.reset(kind, n, seed=12)), name        # the VecEnv / Env path: the same draw
        lo, hi = (-0.05, 0.05) if kind == 0 else (-1.0, 1.0)
        col = 0 if kind == 0 else 2
        for x, what in ((e1, "second episode"), (off, "env_id0 offset")):
            assert_uniform(x[:, col], lo, hi, f"{name} {what}")
            assert_uncorrelated(e0[:, col], x[:, col], f"{name} first episode / {what}")


# --------------------------------------------------- SAC's fused acting draw ---
@pytest.mark.gpu
def test_sac_act_step_fused_draws_are_standard_normal():
    """gymrl_sac_act_step with no explicit eps draws N(0,1) in the launch (stream 2, element i * A + j, counter from the
    host or from the device).  With the actor's mean and log_std heads zeroed, mean = 0 and std = 1, so the action is
    bound * tanh(eps) and atanh(action / bound) gives the draws back: standard normal, uncorrelated across envs and
    across consecutive noise counters, and the device-counter form draws the host form's bits.  (The update's streams
    3 / 4 only reach the losses and the parameters, not an output a law can be read from.)"""
    g = Gpu()
    torch, ops = g.torch, g.ops
    from gymrl_amd.sac_pendulum import Config, SACTrainer
    cfg = Config()
    cfg.num_envs, cfg.batch_size, cfg.hidden_dim, cfg.seed = 4096, 128, 32, 3
    cfg.max_episodes, cfg.memory_capacity = 10 ** 9, 1 << 14
    tr = SACTrainer(cfg)
    assert tr._fused_ok()
    with torch.no_grad():
        for layer in (tr.actor.mean, tr.actor.log_std):
            layer.weight.zero_()
            layer.bias.zero_()
    env, args = tr.env, tr._fused_args()[0]
    N, A, bound = env.n, env.act_dim, float(tr.action_bound)
    obs = env.reset()
    nxt = torch.empty_like(obs)
    steps = 64
    acts = torch.empty(steps, N, A, device=g.dev)
    for c in range(steps):
        ops.sac_act_step(args, env, obs, nxt, noise_seed=5, noise_counter=1000 + c, action_out=acts[c])
        obs, nxt = nxt, obs
    ctr = torch.tensor([1000 + steps - 1], dtype=torch.int64, device=g.dev)
    via_dev = torch.empty(N, A, device=g.dev)
    ops.sac_act_step(args, env, obs, nxt, noise_seed=5, noise_counter=0, noise_counter_dev=ctr, action_out=via_dev)
    torch.cuda.synchronize()
    assert torch.equal(via_dev, acts[-1])
    e = np.arctanh(acts.cpu().numpy().astype(np.float64) / bound)
    assert_standard_normal(e, "sac_act_step stream 2")
    assert_uncorrelated(e[:, :-1], e[:, 1:], "sac_act_step, neighbouring envs")
    assert_uncorrelated(e[:-1], e[1:], "sac_act_step, consecutive noise counters")


# ----------------------------------------------------- GPU == oracle, bits ---
@pytest.mark.gpu
def test_keyed_permutation_bit_exact_at_the_construction_switches(oracle):
    """The distribution tests above read most laws off the oracle: the kernels' bits equal the oracle's on both sides
    of each switch of keyed_permute (Fisher-Yates up to 16 — sizes that use the second to fourth Philox word group —,
    12 Feistel rounds up to 512, 6 from 513), for the epoch shuffle and the replay draw (with B < size and B == size)."""
    g = Gpu()
    for M in (5, 6, 9, 13, 16, 17, 100, 511, 512, 513, 1024, 1025):
        for c in (0, 7, (1 << 33) + 3):
            got = g.ops.permutation(11, c, M, g.dev).cpu().numpy()
            assert np.array_equal(got, oracle.permutation(11, c, M)), (M, c)
            for B in sorted({min(M, 8), M}):
                got = g.ops.uniform_indices(11, c, M, B, g.dev).cpu().numpy()
                assert np.array_equal(got, oracle.uniform_indices(11, c, M, B)), (M, B, c)
