"""CPU helpers for the low-latency Linear layers (gymrl_amd/csrc/lin.hip): the launchers' geometry restated, the
forward and the DUELING epilogue in numpy float32 on top of the oracle's chains, NaN-guarded buffers and the derived
rounding bound.  No GPU; tests/test_lin_ref.py grounds these, tests/test_lin_seams_gpu.py uses them to assert the
kernel, tile width, slice count and last-slice length every case means to reach.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24                         # unit roundoff of float32
ACT = {"none": 0, "tanh": 1, "relu": 2, "clamp": 3, "dueling": 4, "silu": 5}
MAX_ITEMS = 4
SKINNY_N, SKINNY_B = 16, 8192          # lin_bwd_input_skinny_kernel: N <= 16, B > 8192
SKINNY_GRID_CAP = 16384                # its grid: at most this many 256-thread blocks, grid-stride beyond


def cdiv(a, b):
    return (a + b - 1) // b


# ---- gymrl_lin_fwd / gymrl_lin_bwd_input ------------------------------------------------------------------------------
def pick_nt(row_tiles, cols):
    """16 x 64 tiles per wave (NT = 4) once 16 x 16 tiles would be more than 2048 waves."""
    return 4 if cols > 16 and row_tiles * cdiv(cols, 16) > 2048 else 1


def fwd_path(B, K, K1, N, ldx, aligned=True):
    """(NT, VEC) of lin_fwd_kernel: VEC needs one input block, K and ldx multiples of 4 and 16-byte-aligned x and w."""
    return pick_nt(cdiv(B, 16), N), bool(K1 == K and K % 4 == 0 and ldx % 4 == 0 and aligned)


def bwd_input_skinny(B, N, K, K1, lddx=None, sum_items=False, n_items=1, aligned=True):
    lddx = K if lddx is None else lddx
    return bool(N <= SKINNY_N and K1 == K and K % 4 == 0 and lddx % 4 == 0 and B > SKINNY_B
                and not (sum_items and n_items > 1) and aligned)


def bwd_input_path(B, N, K, K1, ldy, lddx=None, sum_items=False, n_items=1, aligned=True, dx_aligned=True):
    """("skinny", None, None) or ("mfma", NT, VEC) of gymrl_lin_bwd_input; VEC: N and ldy multiples of 4, aligned dy / y."""
    if bwd_input_skinny(B, N, K, K1, lddx, sum_items, n_items, dx_aligned):
        return "skinny", None, None
    return "mfma", pick_nt(cdiv(B, 16), K), bool(N % 4 == 0 and ldy % 4 == 0 and aligned)


def skinny_blocks(B, K):
    """(blocks launched, blocks the shape asks for) of the skinny kernel."""
    want = cdiv(B * (K // 4), 256)
    return min(want, SKINNY_GRID_CAP), want


# ---- gymrl_lin_bwd_weight ---------------------------------------------------------------------------------------------
def bwd_weight_big_shape(B, N, K):
    return B >= 16384 and N % 64 == 0 and K % 64 == 0


def bwd_weight_slices(B, N, K):
    if B <= 512:
        return 1
    by_rows = cdiv(B, 256)
    if bwd_weight_big_shape(B, N, K):
        blocks = (N // 64) * (K // 64)
        return min(min(cdiv(2048, blocks), 512), by_rows)
    tiles = cdiv(N, 16) * cdiv(K, 16)
    return min(min(max(cdiv(2048, tiles), 16), 256), by_rows)


def bwd_weight_rows_per_slice(B, slices):
    return cdiv(cdiv(B, slices), 32) * 32


def bwd_weight_lds(N, K):
    return N % 128 == 0 and K % 128 == 0


def bwd_weight_path(B, N, K, K1=None, act=0, ld_ok=True, aligned=True):
    """(kernel, nt, slices, rows_per_slice, rows of the last slice).  kernel: "big_lds" | "big" (64 x 64 blocks, nt None) or
    "tile" (16 x 16 tiles, nt 1 | 4).  ld_ok: ldy and ldx multiples of 4; aligned: dy, x, dw 16-byte aligned.  A big shape
    that fails these, or has an activation or a second input block, falls back to the tile kernel with the big shape's cut."""
    K1 = K if K1 is None else K1
    s = bwd_weight_slices(B, N, K)
    rps = bwd_weight_rows_per_slice(B, s)
    last = B - (s - 1) * rps
    if bwd_weight_big_shape(B, N, K) and K1 == K and ld_ok and aligned and act == 0:
        return ("big_lds" if bwd_weight_lds(N, K) else "big"), None, s, rps, last
    nt = 4 if cdiv(N, 16) * cdiv(K, 16) * s > 4096 else 1
    return "tile", nt, s, rps, last


def slices_from_workspace(nbytes, n_items, N, K):
    """The slice count gymrl_lin_workspace_bytes implies (0 bytes: one slice)."""
    per = 4 * n_items * (N * K + N)
    assert nbytes % per == 0
    return nbytes // per if nbytes else 1


def reduce_groups(slices):
    """Slices per group of lin_slice_reduce_kernel's eight groups."""
    each = cdiv(slices, 8)
    return [max(0, min(slices, (g + 1) * each) - g * each) for g in range(8)]


def slice_batches(rows):
    """16-row batches a 64 x 64-block kernel walks for a slice of `rows` rows, and whether the last one is partial."""
    return cdiv(rows, 16), rows % 16 != 0


def smallest_weight_nt4(max_B=8192):
    """The (B, N, K) with the fewest multiplies B N K for which the tile kernel runs NT = 4 with K no multiple of 64."""
    best = None
    for n_tiles in range(1, 65):
        N = 16 * (n_tiles - 1) + 1
        for k_tiles in range(1, 4200 // n_tiles + 2):
            K = 16 * (k_tiles - 1) + 1
            if K % 64 == 0:
                continue
            lo, hi = 1, max_B                 # slices grow with B: the first B at which tiles x slices > 4096
            if bwd_weight_path(hi, N, K)[1] != 4:
                continue
            while lo < hi:
                mid = (lo + hi) // 2
                if bwd_weight_path(mid, N, K)[1] == 4:
                    hi = mid
                else:
                    lo = mid + 1
            if best is None or lo * N * K < best[0]:
                best = (lo * N * K, lo, N, K)
            break                             # more column tiles only cost more
    return best[1:]


# ---- arithmetic -------------------------------------------------------------------------------------------------------
def act_bwd(y, act, lo=0.0, hi=0.0):
    """lin_device.hpp act_bwd on float32 arrays: the derivative as a function of the saved output."""
    y = np.asarray(y, F32)
    if act == ACT["relu"]:
        return (y > 0).astype(F32)
    if act == ACT["tanh"]:
        return F32(1.0) - y * y
    if act == ACT["clamp"]:
        return ((y > F32(lo)) & (y < F32(hi))).astype(F32)
    return np.ones_like(y)


def dz_f32(dy, y, act, lo=0.0, hi=0.0):
    dy = np.asarray(dy, F32)
    return dy if act == ACT["none"] else dy * act_bwd(y, act, lo, hi)


def fwd(orc, x, W, b, act=0, lo=0.0, hi=0.0, x2=None):
    """lin_fwd for none / relu / clamp, bit for bit: the oracle's chain (orc_linear_act's order is lin_fwd's), clamp as
    fminf(fmaxf(z, lo), hi) of the act-none result."""
    xc = np.asarray(x, F32) if x2 is None else np.concatenate([np.asarray(x, F32), np.asarray(x2, F32)], 1)
    if act == ACT["relu"]:
        return orc.linear_act(xc, W, b, 2)
    z = orc.linear_act(xc, W, b, 0)
    if act == ACT["clamp"]:
        return np.minimum(np.maximum(z, F32(lo)), F32(hi))
    assert act == ACT["none"], "tanh / silu: hardware exp2 / rcp / expf epilogues, held to float64 of the pinned z instead"
    return z


def tanh_bound(z):
    """Per-element bound on |train_tanhf(z) - tanh(z)| for float32 z (train_device.hpp: e = exp2(z * fl(2 / ln 2)),
    y = fma(-2, rcp(e + 1), 1)).  Roundings: the constant and the product (u each, scaled by the exponent's sensitivity
    ln 2 * |t| = 2 |z|: 4 |z| u on e), v_exp_f32 within 1 ulp (2 u), the add (u), v_rcp_f32 within 1 ulp (2 u): the
    relative error of r = 1 / (e + 1) is at most (4 |z| + 5) u, it enters y through 2 r = 1 - tanh(z); the fma rounds once
    (u |y|).  Second-order terms are covered by the factor 1.01."""
    z64 = np.asarray(z, np.float64)
    t = np.tanh(z64)
    return 1.01 * U * (np.abs(t) + (1.0 - t) * (4.0 * np.abs(z64) + 5.0))


def dueling(z, A):
    """The DUELING epilogue on z = acc + bias [B, A + 1] (float32): s = the xor-1, 2, 4, 8 butterfly's balanced pairwise
    tree over the 16 columns (columns >= A count as 0), q = v + (z - s / A), every operation rounded to float32; the
    argmax is the first maximum.  Returns (q [B, A], argmax [B] int32)."""
    z = np.asarray(z, F32)
    B = z.shape[0]
    s = np.zeros((B, 16), F32)
    s[:, :A] = z[:, :A]
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2]
    q = z[:, A:A + 1] + (z[:, :A] - s / F32(A))
    assert q.dtype == F32
    return q, np.argmax(q, axis=1).astype(np.int32)


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): |fl(sum) - sum| <= gamma_n * sum |terms| after n float32 roundings on the path."""
    return n * U / (1.0 - n * U)


# ---- NaN-guarded buffers ----------------------------------------------------------------------------------------------
GUARD = 3


def guarded(torch, rows, cols, device, fill=None, col_guard=True, dtype=None, sentinel=float("nan")):
    """(buffer, view): `view` is the [rows, cols] window of a sentinel-filled buffer with GUARD rows above and below and,
    with col_guard, GUARD columns left and right.  fill: a [rows, cols] tensor the window starts from (accumulate)."""
    dtype = torch.float32 if dtype is None else dtype
    c = GUARD if col_guard else 0
    buf = torch.full((rows + 2 * GUARD, cols + 2 * c), sentinel, dtype=dtype, device=device)
    view = buf[GUARD:GUARD + rows, c:c + cols]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def guarded_vec(torch, n, device, fill=None, dtype=None, sentinel=float("nan")):
    dtype = torch.float32 if dtype is None else dtype
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=device)
    view = buf[GUARD:GUARD + n]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def guards_intact(torch, buf, view_shape, col_guard=True, sentinel=float("nan")):
    """Everything outside the window still holds the sentinel and, for a NaN sentinel, nothing inside does."""
    is_nan = sentinel != sentinel
    hit = torch.isnan(buf) if is_nan else buf == sentinel
    inside = torch.zeros_like(hit)
    if buf.dim() == 1:
        inside[GUARD:GUARD + view_shape[0]] = True
    else:
        c = GUARD if col_guard else 0
        inside[GUARD:GUARD + view_shape[0], c:c + view_shape[1]] = True
    outside_ok = bool(hit[~inside].all())
    inside_ok = (not is_nan) or not bool(hit[inside].any())
    return outside_ok and inside_ok
