"""Plain NumPy float64 restatement of the one-launch GRU / LSTM sequence kernels' contract (include/gymrl.h:
gymrl_gru_seq_fwd/_bwd, gymrl_lstm_seq_fwd/_bwd), written as the explicit time loop, and the input generators of
tests/test_rnn_seq_edges_gpu.py.  PyTorch's gate order (GRU r, z, n; LSTM i, f, g, o); a row with t >= len is frozen:
it writes zeros, keeps its state forward and passes its gradient through backward; a None operand means zeros.
Nothing here goes through torch.nn: tests/test_rnn_seq_ref.py checks the loops against float64 nn.GRU / nn.LSTM and
every generator for the property it states, on the CPU."""
import numpy as np

TILE = 16                                  # rows of a workgroup's tile
FWD = {"gru": ("h_seq", "h_last"), "lstm": ("h_seq", "c_seq", "h_last", "c_last")}
BWD = {"gru": ("dgi", "dgh", "dh0"), "lstm": ("dgates", "dh0", "dc0")}
NAMES = {k: FWD[k] + BWD[k] for k in FWD}
GATES = {"gru": 3, "lstm": 4}


def _sig(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _f64(a, shape):
    return np.zeros(shape) if a is None else np.asarray(a, np.float64).reshape(shape)


def gru_seq(lens, gi, W, b, h0, d_hseq, d_hlast, pre=None):
    """-> h_seq [T,B,H], h_last [B,H], dgi, dgh [T,B,3H], dh0 [B,H], all float64.  pre: a dict that receives "a"
    [T,B,3H], the gate pre-activations (gi_r + gh_r, gi_z + gh_z, gi_n + r * gh_n)."""
    T, B, H3 = gi.shape
    H = H3 // 3
    gi, W, b = np.asarray(gi, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    h0, d_hseq, d_hlast = _f64(h0, (B, H)), _f64(d_hseq, (T, B, H)), _f64(d_hlast, (B, H))
    live = np.asarray(lens).reshape(1, B, 1) > np.arange(T).reshape(T, 1, 1)
    h_seq, a = np.zeros((T, B, H)), np.zeros((T, B, H3))
    kept = []
    h = h0.copy()
    for t in range(T):
        gh = h @ W.T + b
        r, z = _sig(gi[t, :, :H] + gh[:, :H]), _sig(gi[t, :, H:2 * H] + gh[:, H:2 * H])
        a[t] = np.concatenate([gi[t, :, :H] + gh[:, :H], gi[t, :, H:2 * H] + gh[:, H:2 * H], gi[t, :, 2 * H:] + r * gh[:, 2 * H:]], 1)
        n = np.tanh(a[t, :, 2 * H:])
        hn = (1.0 - z) * n + z * h
        kept.append((r, z, n, gh[:, 2 * H:], h))
        h_seq[t] = np.where(live[t], hn, 0.0)
        h = np.where(live[t], hn, h)
    h_last = h
    dgi, dgh = np.zeros((T, B, H3)), np.zeros((T, B, H3))
    dh = d_hlast.copy()
    for t in range(T - 1, -1, -1):
        r, z, n, ghn, hp = kept[t]
        go = dh + d_hseq[t]
        dnp = go * (1.0 - z) * (1.0 - n * n)
        d_r, d_z = dnp * ghn * (r * (1.0 - r)), go * (hp - n) * (z * (1.0 - z))
        gi_t, gh_t = np.concatenate([d_r, d_z, dnp], 1), np.concatenate([d_r, d_z, dnp * r], 1)
        dgi[t], dgh[t] = np.where(live[t], gi_t, 0.0), np.where(live[t], gh_t, 0.0)
        dh = np.where(live[t], go * z + gh_t @ W, dh)
    if pre is not None:
        pre["a"] = a
    return h_seq, h_last, dgi, dgh, dh


def lstm_seq(lens, gi, W, b, h0, c0, d_hseq, d_hlast, d_clast, pre=None):
    """-> h_seq, c_seq [T,B,H], h_last, c_last [B,H], dgates [T,B,4H] (= dgi = dgh), dh0, dc0 [B,H], all float64.
    pre: a dict that receives "a" [T,B,4H], the gate pre-activations gi + gh."""
    T, B, H4 = gi.shape
    H = H4 // 4
    gi, W, b = np.asarray(gi, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    h0, c0 = _f64(h0, (B, H)), _f64(c0, (B, H))
    d_hseq, d_hlast, d_clast = _f64(d_hseq, (T, B, H)), _f64(d_hlast, (B, H)), _f64(d_clast, (B, H))
    live = np.asarray(lens).reshape(1, B, 1) > np.arange(T).reshape(T, 1, 1)
    h_seq, c_seq, a = np.zeros((T, B, H)), np.zeros((T, B, H)), np.zeros((T, B, H4))
    kept = []
    h, c = h0.copy(), c0.copy()
    for t in range(T):
        a[t] = gi[t] + (h @ W.T + b)
        i, f, g, o = _sig(a[t, :, :H]), _sig(a[t, :, H:2 * H]), np.tanh(a[t, :, 2 * H:3 * H]), _sig(a[t, :, 3 * H:])
        cn = f * c + i * g
        hn = o * np.tanh(cn)
        kept.append((i, f, g, o, c, cn))
        h_seq[t], c_seq[t] = np.where(live[t], hn, 0.0), np.where(live[t], cn, 0.0)
        h, c = np.where(live[t], hn, h), np.where(live[t], cn, c)
    h_last, c_last = h, c
    dgates = np.zeros((T, B, H4))
    dh, dc = d_hlast.copy(), d_clast.copy()
    for t in range(T - 1, -1, -1):
        i, f, g, o, cp, cn = kept[t]
        go, tc = dh + d_hseq[t], np.tanh(cn)
        dcn = dc + go * o * (1.0 - tc * tc)
        d_t = np.concatenate([dcn * g * (i * (1.0 - i)), dcn * cp * (f * (1.0 - f)), dcn * i * (1.0 - g * g),
                              go * tc * (o * (1.0 - o))], 1)
        dgates[t] = np.where(live[t], d_t, 0.0)
        dh = np.where(live[t], d_t @ W, dh)
        dc = np.where(live[t], dcn * f, dc)
    if pre is not None:
        pre["a"] = a
    return h_seq, c_seq, h_last, c_last, dgates, dh, dc


def weight_grads(dgh, h_seq, h0):
    """dW_hh = sum_t dgh_t^T h_{t-1}, db_hh = sum_t dgh_t over the flattened rows, in float64 (the caller's GEMMs)."""
    T, B, HG = dgh.shape
    H = h_seq.shape[2]
    h0 = _f64(h0, (B, H))
    hprev = np.concatenate([h0[None], np.asarray(h_seq, np.float64)[:-1]], 0) if T else np.zeros((0, B, H))
    d = np.asarray(dgh, np.float64).reshape(T * B, HG)
    return d.T @ hprev.reshape(T * B, H), d.sum(0)


# ---- inputs ---------------------------------------------------------------------------------------------------------

OPERANDS = {"gru": ("h0", "d_hseq", "d_hlast"), "lstm": ("h0", "c0", "d_hseq", "d_hlast", "d_clast")}
# which optional operands are absent: each alone, all of them, and PPG-RNN's call (no initial state, only d_hseq)
ABSENT = {"h0": ("h0",), "c0": ("c0",), "d_hseq": ("d_hseq",), "d_hlast": ("d_hlast",), "d_clast": ("d_clast",),
          "all": ("h0", "c0", "d_hseq", "d_hlast", "d_clast"), "ppg_rnn": ("h0", "c0", "d_hlast", "d_clast")}


def ragged(rng, B, T):
    """Random lengths in [0, T] that hold a 0, a 1 and a T wherever B leaves room for them."""
    lens = rng.integers(0, T + 1, size=B)
    lens[0] = T
    if B > 1:
        lens[-1] = 1
    if B > 2:
        lens[1] = 0
    return [int(x) for x in lens]


def case(kind, seed, B, T, H, lens=None, scale=0.3):
    """The usual random inputs of the sequence tests (gi ~ 1.5 N, W_hh ~ scale N, b_hh ~ 0.5 N, states ~ 0.5 N, unit
    normal incoming gradients), float32, as a dict with every optional operand present."""
    rng = np.random.default_rng(seed)
    G = GATES[kind]
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    c = {"lens": ragged(rng, B, T) if lens is None else [int(x) for x in lens],
         "gi": f32(rng.normal(size=(T, B, G * H)) * 1.5), "W": f32(rng.normal(size=(G * H, H)) * scale),
         "b": f32(rng.normal(size=G * H) * 0.5), "h0": f32(rng.normal(size=(B, H)) * 0.5),
         "d_hseq": f32(rng.normal(size=(T, B, H))), "d_hlast": f32(rng.normal(size=(B, H)))}
    if kind == "lstm":
        c["c0"], c["d_clast"] = f32(rng.normal(size=(B, H)) * 0.5), f32(rng.normal(size=(B, H)))
    assert len(c["lens"]) == B
    return c


def reference(kind, c, absent=(), pre=None):
    """The float64 loop on case c with the operands named in `absent` left out -> {name: array}."""
    op = {k: (None if k in absent else c[k]) for k in OPERANDS[kind]}
    if kind == "gru":
        out = gru_seq(c["lens"], c["gi"], c["W"], c["b"], op["h0"], op["d_hseq"], op["d_hlast"], pre=pre)
    else:
        out = lstm_seq(c["lens"], c["gi"], c["W"], c["b"], op["h0"], op["c0"], op["d_hseq"], op["d_hlast"], op["d_clast"], pre=pre)
    return dict(zip(NAMES[kind], out))


PATTERNS = ("zeros", "full", "ones", "tile0_zero_tile1_full", "tile0_full_tile1_zero", "one_full_slot0", "one_full_slot15",
            "tmax3", "random")


def length_pattern(name, B, T, seed=0):
    """The length patterns of the every-element-is-written test.  Tiles are rows [16k, 16k + 16)."""
    rng = np.random.default_rng(seed)
    row = np.arange(B)
    if name == "zeros":
        lens = np.zeros(B, int)
    elif name == "full":
        lens = np.full(B, T)
    elif name == "ones":
        lens = np.ones(B, int)
    elif name == "tile0_zero_tile1_full":                   # the other tiles, if any, alternate on
        lens = np.where((row // TILE) % 2 == 0, 0, T)
    elif name == "tile0_full_tile1_zero":
        lens = np.where((row // TILE) % 2 == 0, T, 0)
    elif name == "one_full_slot0":
        lens = np.where(row == 0, T, 0)
    elif name == "one_full_slot15":                         # the tile's last slot, or the batch's last row before it
        lens = np.where(row == min(TILE - 1, B - 1), T, 0)
    elif name == "tmax3":                                   # every tile ends at 3 < T: its tail starts at tmax, not T
        lens = rng.integers(0, 4, size=B)
        lens[::TILE] = 3
    elif name == "random":
        lens = np.asarray(ragged(rng, B, T))
    else:
        raise KeyError(name)
    return [int(x) for x in lens]


SAT = 100.0
PLANTED = (SAT, -SAT, 0.0, -0.0)                           # unit 4k + j of gate k holds PLANTED[j] at every row and step


def saturated_case(kind, seed, B, T, H):
    """case() with saturated gates and signed zeros planted in gi: in gate k's block, unit 4k + j holds PLANTED[j]
    (+100, -100, +0.0, -0.0) for every row and step; the first rows, all of length T, are saturated in whole gates:
      lstm row 0: i = f = +100, g = +100 (c grows by 1 each step);  row 1: i = f = +100, g = -100 (c falls by 1)
      gru  row 0: z = +100 (h never moves);  row 1: r = z = -100, n = +100 (h jumps to 1)
    W_hh keeps the usual 0.3 scale, so |gh| stays far below 50 and a planted +-100 is a pre-activation beyond +-50."""
    c = case(kind, seed, B, T, H)
    G, gi = GATES[kind], c["gi"]
    for k in range(G):
        for j, v in enumerate(PLANTED):
            gi[:, :, k * H + 4 * k + j] = v
    blk = lambda k: slice(k * H, (k + 1) * H)  # noqa: E731
    if kind == "lstm":
        for row, g in ((0, SAT), (1, -SAT)):
            gi[:, row, blk(0)], gi[:, row, blk(1)], gi[:, row, blk(2)] = SAT, SAT, g
    else:
        gi[:, 0, blk(1)] = SAT
        gi[:, 1, blk(0)], gi[:, 1, blk(1)], gi[:, 1, blk(2)] = -SAT, -SAT, SAT
    for row in range(min(2, B)):
        c["lens"][row] = T
    return c


def planted_mask(kind, B, T, H):
    """bool [T,B,G*H]: where saturated_case planted +-100."""
    G = GATES[kind]
    m = np.zeros((T, B, G * H), bool)
    for k in range(G):
        m[:, :, k * H + 4 * k], m[:, :, k * H + 4 * k + 1] = True, True
    if kind == "lstm":
        m[:, :2, :3 * H] = True
    else:
        m[:, 0, H:2 * H] = True
        m[:, 1, :] = True
    return m


PERM_B = 35


def placement_case(kind, seed, H, T=8):
    """B = 35 ragged rows with lengths 0, 1, 3, T, T at rows SOLO, and a fixed permutation (row i of the permuted batch is
    row PERM[i]) that moves rows between tiles and between slots."""
    c = case(kind, seed, PERM_B, T, H)
    for row, n in zip(SOLO, (0, 1, 3, T, T)):
        c["lens"][row] = n
    return c


SOLO = (2, 7, 16, 0, 34)
PERM = tuple(int(x) for x in (np.arange(PERM_B) * 12 + 5) % PERM_B)


def take_rows(kind, c, rows):
    """Case c restricted to / reordered by `rows` (every per-row operand, the lengths included)."""
    rows = list(rows)
    out = {"lens": [c["lens"][i] for i in rows], "W": c["W"], "b": c["b"]}
    for k in ("gi", "d_hseq"):
        out[k] = np.ascontiguousarray(c[k][:, rows])
    for k in ("h0", "c0", "d_hlast", "d_clast"):
        if k in c:
            out[k] = np.ascontiguousarray(c[k][rows])
    return out
