"""numpy restatement of gymrl_mlp_pack_stack's contract (include/gymrl.h), for tests/test_pack_stack_abi.py (which grounds it on
a hand-written weight) and tests/test_pack_stack_gpu.py (which holds the kernel to it bit for bit).

A layer is (out_dim, in_dim, w_off, b_off, w_at, b_at): floats into a row of params (the weight [out_dim, in_dim] row-major, the
bias) and into a packed row (the MFMA B-operand image, the bias padded with zeros to a multiple of four)."""
import numpy as np


def packed_floats(out_dim, in_dim):
    """gymrl_mlp_packed_floats: 16-row tiles x K-blocks of 16 (K rounded up to 64) x 64 lanes x 4."""
    return (out_dim + 15) // 16 * ((in_dim + 63) // 64 * 4) * 256


def pack_image(W):
    """P[tile][kblock][lane][c] = W[16 tile + (lane & 15)][16 kblock + 4 (lane >> 4) + c], zeros beyond either dimension."""
    out_dim, in_dim = W.shape
    ntiles, nkb = (out_dim + 15) // 16, (in_dim + 63) // 64 * 4
    padded = np.zeros((16 * ntiles, 16 * nkb), dtype=np.float32)
    padded[:out_dim, :in_dim] = W
    image = np.empty((ntiles, nkb, 64, 4), dtype=np.float32)
    for lane in range(64):
        for c in range(4):
            image[:, :, lane, c] = padded[(lane & 15)::16, (4 * (lane >> 4) + c)::16]
    return image.reshape(-1)


def tight_layout(shapes):
    """(w_at, b_at per layer, tight stride) of ops.LunarPolicyStack's row: every image, then every padded bias."""
    sizes = [packed_floats(o, i) for o, i in shapes] + [(o + 3) // 4 * 4 for o, _ in shapes]
    at = [sum(sizes[:k]) for k in range(len(sizes))]
    L = len(shapes)
    return at[:L], at[L:], sum(sizes)


def written_mask(layers, packed_stride):
    """bool[packed_stride]: the floats of a row the launch writes — the 2 L ranges, nothing else."""
    mask = np.zeros(packed_stride, dtype=bool)
    for out_dim, in_dim, _, _, w_at, b_at in layers:
        for at, n in ((w_at, packed_floats(out_dim, in_dim)), (b_at, (out_dim + 3) // 4 * 4)):
            assert not mask[at:at + n].any() and at + n <= packed_stride, "the ranges of a row overlap or overrun it"
            mask[at:at + n] = True
    return mask


def pack_stack(params, layers, packed):
    """The launch on numpy arrays: params f32[P, >= extent], packed f32[P, packed_stride] (a copy is filled and returned; the
    floats outside the ranges keep what `packed` held)."""
    out = np.array(packed, dtype=np.float32, copy=True)
    for p in range(params.shape[0]):
        for out_dim, in_dim, w_off, b_off, w_at, b_at in layers:
            W = params[p, w_off:w_off + out_dim * in_dim].reshape(out_dim, in_dim)
            out[p, w_at:w_at + packed_floats(out_dim, in_dim)] = pack_image(W)
            pad = (out_dim + 3) // 4 * 4
            out[p, b_at:b_at + pad] = 0.0
            out[p, b_at:b_at + out_dim] = params[p, b_off:b_off + out_dim]
    return out
