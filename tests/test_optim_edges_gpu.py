"""The optimiser kernels of gymrl_amd/csrc/optim.hip past one workgroup, through gymrl_amd.ops, against references
that are not the kernel: the oracle's restatement bit for bit (orc_sqnorm, orc_adam_step, orc_soft_update), adam_f32 of
tests/optim_ref.py bit for bit where the oracle has no such form (lr_dev, bias_dev), an exact sum for the norm and
adam_f64 within the bounds tests/test_hip_parity.py::test_adam_and_soft_update uses.  tests/test_optim_ref.py grounds
those references on the CPU.

Every device buffer is a view of n floats at a 16-byte-aligned offset inside a larger allocation with a sentinel on
both sides, read back after the calls.

Sizes: 1..5 the n & 3 tail alone and behind one float4; 1023..1025 one to two workgroups of Adam (1024 elements each);
4095..4097 the same of the norm (4096 each); 1 048 577 = 257 norm partials, a second round of the fold per thread;
1 050 627 = Adam's cap of 1024 workgroups + 2050 elements of a second grid-stride trip + a tail of 3; 4 198 403 the
same of the norm."""
import ctypes as C

import numpy as np
import pytest

from conftest import bounded, rel_close
from optim_ref import BETAS, F32, adam_f32, adam_f64, clip_scale_f32, host_scalars, mixed_grad, sqnorm_fsum

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5                                   # tests/test_hip_parity.py's
P_ABS = 2e-6                                 # its bound on p against torch.optim.Adam
B1, B2 = BETAS
LR, EPS, TAU = 1e-3, 1e-8, 0.005
THIRD = float(F32(1.0 / 3.0))
PAD, SENT = 8, -7777.25                      # 8 floats = 32 bytes: the view stays 16-byte aligned
WS_SENT = -3.0                               # the reduce workspace's doubles past the partials in use

TAILS = [1, 2, 3, 4, 5]
ADAM_SIZES = TAILS + [1023, 1024, 1025, 4095, 4096, 4097, 1048577, 1050627]
NORM_SIZES = ADAM_SIZES + [4198403]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from gymrl_amd import ops
    assert ops.device_ok(), "libgymrl_hip.so did not find a gfx950 device"
    return torch.device("cuda:0")


class Guarded:
    """n floats inside PAD + n + PAD, the pads holding SENT."""

    def __init__(self, a, dev):
        self.n = a.size
        self.buf = torch.full((2 * PAD + self.n,), SENT, dtype=torch.float32, device=dev)
        self.t = self.buf[PAD:PAD + self.n]
        assert self.t.data_ptr() % 16 == 0
        self.set(a)

    def set(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))

    def get(self):
        return self.t.cpu().numpy()

    def shifted(self):
        """The same length one float further on: 4-byte aligned only (still inside the allocation)."""
        return self.buf[PAD + 1:PAD + 1 + self.n]

    def intact(self):
        return bool((self.buf[:PAD] == SENT).all()) and bool((self.buf[PAD + self.n:] == SENT).all())


def workspace(dev):
    return torch.full((16384,), WS_SENT, dtype=torch.float64, device=dev)       # gymrl_reduce_workspace_bytes() / 8


def norm_parts(n):
    return min(max((n + 4095) // 4096, 1), 1024)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(a, b):
    """Bit for bit, except that a NaN matches any NaN: which sign and payload an operation gives a NaN it creates is
    left to the implementation by IEEE 754 (x86 SSE makes 0 * inf a negative quiet NaN), and is no result of the step."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def state(rng, n):
    p = rng.normal(size=n).astype(np.float32)
    m = (0.01 * rng.normal(size=n)).astype(np.float32)
    v = (0.01 * np.abs(rng.normal(size=n))).astype(np.float32)
    return p, m, v


def run_step(ops, entry, P, G, M, V, sq, ws, step, max_norm, gs, lr=LR, b2=B2, **kw):
    """One optimiser step through gymrl_adam_step (after gymrl_sqnorm when clipping) or gymrl_clip_adam_step."""
    if entry == "fused":
        ops.clip_adam_step(P.t, G.t, M.t, V.t, lr, B1, b2, EPS, step, max_norm, ws, grad_scale=gs, sqnorm_out=sq, **kw)
    else:
        if max_norm > 0:
            ops.sqnorm(G.t, sq, ws, gs)
        ops.adam_step(P.t, G.t, M.t, V.t, lr, B1, b2, EPS, step, grad_scale=gs, max_grad_norm=max_norm,
                      sqnorm_buf=sq if max_norm > 0 else None, **kw)


# --------------------------------------------------------------------------------------------------- gymrl_sqnorm ---
@pytest.mark.parametrize("n", NORM_SIZES)
def test_sqnorm(dev, oracle, n):
    from gymrl_amd import ops
    g = mixed_grad(np.random.default_rng(n), n)
    G = Guarded(g, dev)
    for gs in (1.0, 0.5, THIRD):
        ws, sq = workspace(dev), torch.full((1,), -1.0, dtype=torch.float64, device=dev)
        ops.sqnorm(G.t, sq, ws, gs)
        got, exact = float(sq.item()), sqnorm_fsum(g, gs)
        err = abs(got - exact) / exact
        print(f"sqnorm n={n} gs={gs:.9g}: relative error against fsum {err:.3e}")
        assert got == float(oracle.sqnorm(g, gs)[0])                      # the documented order: bit for bit
        assert err <= 1e-13
        assert bool((ws[norm_parts(n):] == WS_SENT).all())                # no partial past the grid's
    assert G.intact() and np.array_equal(bits(G.get()), bits(g))


# --------------------------------------------------------------- gymrl_adam_step / gymrl_clip_adam_step, 3 steps ---
SETTINGS = {          # max_norm, clamp_abs, grad_scale, zero_grad, Polyak target
    "clip": (0.5, 0.0, 1.0, True, False),
    "clip+clamp+scale+keepgrad+polyak": (10.0, 1.0, THIRD, False, True),
    "neverclips+scale+polyak": (1e9, 0.0, 0.5, True, True),
    "clamp-plain": (0.0, 1.0, 1.0, True, False),
}


@pytest.mark.parametrize("key", list(SETTINGS))
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_three_steps(dev, oracle, n, key):
    from gymrl_amd import ops
    max_norm, clamp, gs, zero_grad, polyak = SETTINGS[key]
    rng = np.random.default_rng(1000 * list(SETTINGS).index(key) + n)
    p0, m0, v0 = state(rng, n)
    t0 = rng.normal(size=n).astype(np.float32)
    grads = [mixed_grad(rng, n, step) for step in (1, 2, 3)]
    # the references, once: the oracle's trajectory (bits) and the float64 one (tolerance)
    ref, (po, mo, vo, to), (pf, mf, vf) = [], (p0, m0, v0, t0), (p0, m0, v0)
    for step, g in enumerate(grads, 1):
        sq_o = float(oracle.sqnorm(g, gs)[0]) if max_norm > 0 else None
        po, go, mo, vo = oracle.adam_step(po, g, mo, vo, LR, B1, B2, EPS, step, grad_scale=gs, max_grad_norm=max_norm,
                                          clamp_abs=clamp, zero_grad=zero_grad)
        to = oracle.soft_update(to, po, TAU) if polyak else to
        pf, _, mf, vf, _ = adam_f64(pf, g, mf, vf, LR, B1, B2, EPS, step, grad_scale=gs, max_norm=max_norm, clamp_abs=clamp)
        ref.append((g, sq_o, po, go, mo, vo, to, pf, mf, vf))
    for entry in (("plain", "fused") if max_norm > 0 else ("plain",)):
        P, M, V, T, G = (Guarded(a, dev) for a in (p0, m0, v0, t0, grads[0]))
        ws, sq = workspace(dev), torch.full((1,), -1.0, dtype=torch.float64, device=dev)
        kw = dict(clamp_abs=clamp, zero_grad=zero_grad)
        if polyak:
            kw.update(polyak_target=T.t, tau=TAU)
        for step, (g, sq_o, po, go, mo, vo, to, pf, mf, vf) in enumerate(ref, 1):
            G.set(g)
            run_step(ops, entry, P, G, M, V, sq, ws, step, max_norm, gs, **kw)
            p, m, v, ga = P.get(), M.get(), V.get(), G.get()
            tag = f"optim_edges/{key}/{entry}/n{n}/step{step}"
            assert np.array_equal(bits(p), bits(po)) and np.array_equal(bits(m), bits(mo)) and np.array_equal(bits(v), bits(vo)), tag
            assert np.array_equal(bits(T.get()), bits(to)), tag             # updated from the new p, or untouched
            if max_norm > 0:
                assert float(sq.item()) == sq_o, tag
                assert bool((ws[norm_parts(n):] == WS_SENT).all()), tag
            assert np.array_equal(bits(ga), bits(go)), tag                   # the oracle's: zeroed or left alone
            assert np.array_equal(bits(ga), np.zeros(n, np.int32) if zero_grad else bits(g)), tag   # +0.0 / unchanged
            assert all(x.intact() for x in (P, G, M, V, T)), tag
            ep, em, ev = float(np.max(np.abs(p - pf))), rel_close(m, mf), rel_close(v, vf)
            print(f"{tag}: p {ep:.3e} m {em:.3e} v {ev:.3e}")
            bounded(tag + "/p", ep, P_ABS)
            bounded(tag + "/m", em, TOL)
            bounded(tag + "/v", ev, TOL)


# ------------------------------------------------------------------------------------------------- device scalars ---
@pytest.mark.parametrize("form", ["lr_dev", "bias_dev", "lr_dev+bias_dev"])
@pytest.mark.parametrize("n", [5, 1025, 1050627])
def test_device_scalars(dev, oracle, n, form):
    """lr_dev: step_size = lr_dev[0] * inv_bc1 as one float32 product (inv_bc1 the host's (float)(1 / bc1), or
    bias_dev[1]) — not the host form's (float)(lr / bc1); bias_dev: step_size and sqrt(bc2) straight from the block.
    The host arguments the device values replace are handed in wrong on purpose."""
    from gymrl_amd import ops
    lr, max_norm, gs = 3e-4, 0.5, 0.5
    rng = np.random.default_rng(n + 17)
    p0, m0, v0 = state(rng, n)
    grads = [mixed_grad(rng, n, step) for step in (1, 2, 3)]
    ref, (p, m, v), (pf, mf, vf) = [], (p0, m0, v0), (p0, m0, v0)
    for step, g in enumerate(grads, 1):
        blk = np.frombuffer(ops.adam_bias(lr, B1, B2, step), np.float32)
        assert np.array_equal(blk[:3], np.array(host_scalars(lr, B1, B2, step)))
        ss = F32(F32(lr) * blk[1]) if "lr_dev" in form else blk[0]
        scale = clip_scale_f32(oracle.sqnorm(g, gs)[0], max_norm)
        p, _, m, v = adam_f32(p, g, m, v, B1, B2, EPS, ss, blk[2], scale, grad_scale=gs)
        pf, _, mf, vf, _ = adam_f64(pf, g, mf, vf, lr, B1, B2, EPS, step, grad_scale=gs, max_norm=max_norm)
        ref.append((g, p, m, v, pf, mf, vf))
    for entry in ("plain", "fused"):
        P, M, V, G = (Guarded(a, dev) for a in (p0, m0, v0, grads[0]))
        ws, sq = workspace(dev), torch.zeros(1, dtype=torch.float64, device=dev)
        lr_dev = torch.tensor([lr], dtype=torch.float32, device=dev)
        bias = torch.zeros(4, dtype=torch.float32, device=dev)
        for step, (g, p, m, v, pf, mf, vf) in enumerate(ref, 1):
            G.set(g)
            kw = {}
            if "lr_dev" in form:
                kw["lr_dev"] = lr_dev
            if "bias_dev" in form:
                ops.store_scalars(bias, ops.adam_bias(lr, B1, B2, step))
                kw["bias_dev"] = bias
            run_step(ops, entry, P, G, M, V, sq, ws, 1 if "bias_dev" in form else step, max_norm, gs, lr=123.0, **kw)
            tag = f"optim_edges/{form}/{entry}/n{n}/step{step}"
            gp, gm, gv = P.get(), M.get(), V.get()
            assert np.array_equal(bits(gp), bits(p)) and np.array_equal(bits(gm), bits(m)) and np.array_equal(bits(gv), bits(v)), tag
            assert all(x.intact() for x in (P, G, M, V)), tag
            ep, em, ev = float(np.max(np.abs(gp - pf))), rel_close(gm, mf), rel_close(gv, vf)
            print(f"{tag}: p {ep:.3e} m {em:.3e} v {ev:.3e}")
            bounded(tag + "/p", ep, P_ABS)
            bounded(tag + "/m", em, TOL)
            bounded(tag + "/v", ev, TOL)


# ----------------------------------------------------------------------------------------------- edges of the clip ---
def one_step(ops, dev, oracle, entry, p0, g, m0, v0, max_norm, clamp=0.0, b2=B2):
    """One step of zero_grad = 0 through `entry`; returns the kernel's and the oracle's (p, m, v) and the kernel's norm."""
    P, G, M, V = (Guarded(a, dev) for a in (p0, g, m0, v0))
    ws, sq = workspace(dev), torch.full((1,), -1.0, dtype=torch.float64, device=dev)
    run_step(ops, entry, P, G, M, V, sq, ws, 1, max_norm, 1.0, b2=b2, clamp_abs=clamp, zero_grad=False)
    got = (P.get(), M.get(), V.get())
    assert all(x.intact() for x in (P, G, M, V)) and same_bits(G.get(), g)
    po, _, mo, vo = oracle.adam_step(p0, g, m0, v0, LR, B1, b2, EPS, 1, max_grad_norm=max_norm, clamp_abs=clamp, zero_grad=False)
    return got, (po, mo, vo), float(sq.item())


@pytest.mark.parametrize("entry", ["plain", "fused"])
def test_zero_gradient_leaves_parameters(dev, oracle, entry):
    from gymrl_amd import ops
    n = 1025
    p0, z = np.random.default_rng(3).normal(size=n).astype(np.float32), np.zeros(n, np.float32)
    (p, m, v), ref, sq = one_step(ops, dev, oracle, entry, p0, z, z, z, 0.5)
    assert sq == 0.0                                                     # coef = 0.5 / 1e-6: no clip, and 0 / eps = 0
    assert np.array_equal(bits(p), bits(p0)) and not v.any() and not m.any()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((p, m, v), ref))


@pytest.mark.parametrize("entry", ["plain", "fused"])
def test_norm_equal_to_max_norm(dev, oracle, entry):
    """A one-hot gradient of exactly max_norm: coef = 0.5 / (0.5 + 1e-6) is just below 1 and is applied."""
    from gymrl_amd import ops
    n, k = 1025, 1024
    p0, m0, v0 = state(np.random.default_rng(4), n)
    g = np.zeros(n, np.float32)
    g[k] = 0.5
    scale = clip_scale_f32(0.25, 0.5)
    assert F32(0.999) < scale < F32(1.0)
    (p, m, v), ref, sq = one_step(ops, dev, oracle, entry, p0, g, m0, v0, 0.5)
    assert sq == 0.25
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((p, m, v), ref))
    ss, _, bc2s = host_scalars(LR, B1, B2, 1)
    want = adam_f32(p0, g, m0, v0, B1, B2, EPS, ss, bc2s, scale)
    assert np.array_equal(bits(p), bits(want[0])) and np.array_equal(bits(m), bits(want[2]))
    assert not np.array_equal(bits(m), bits(adam_f32(p0, g, m0, v0, B1, B2, EPS, ss, bc2s, 1.0)[2]))   # scale 1 differs


@pytest.mark.parametrize("b2", [0.999, 0.9])
def test_huge_element_without_clipping(dev, oracle, b2):
    """One element of 1e20, no clip: with beta2 = 0.9 the second moment 0.1 * 1e20 * 1e20 overflows float32, the
    denominator is inf, m / inf = 0 and p keeps its bits at that slot.  With the default beta2 = 0.999 the product is
    1e37, still finite, and the slot moves like any other; both as the oracle has them."""
    from gymrl_amd import ops
    n, k = 1025, 700
    p0, m0, v0 = state(np.random.default_rng(5), n)
    g = mixed_grad(np.random.default_rng(6), n)
    g[k] = 1e20
    (p, m, v), ref, _ = one_step(ops, dev, oracle, "plain", p0, g, m0, v0, 0.0, b2=b2)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((p, m, v), ref))
    if b2 == 0.9:
        assert np.isposinf(v[k]) and bits(p)[k] == bits(p0)[k] and np.isfinite(m[k])
        assert np.isfinite(np.delete(v, k)).all()
    else:
        assert np.isfinite(v).all() and p[k] < p0[k]


@pytest.mark.parametrize("entry", ["plain", "fused"])
def test_subnormal_second_moment(dev, oracle, entry):
    """One element of 1e-21 on zero moments: v = 1e-3 * 1e-21 * 1e-21 is the smallest float32 subnormal."""
    from gymrl_amd import ops
    n, k = 1025, 700
    p0, m0, v0 = state(np.random.default_rng(7), n)
    g = mixed_grad(np.random.default_rng(8), n)
    g[k], m0[k], v0[k] = 1e-21, 0.0, 0.0
    max_norm = 1e9 if entry == "fused" else 0.0
    (p, m, v), (po, mo, vo), _ = one_step(ops, dev, oracle, entry, p0, g, m0, v0, max_norm)
    assert 0.0 < vo[k] < np.finfo(np.float32).tiny                      # the case is what it says
    print(f"subnormal slot ({entry}): kernel v {v[k]!r} p-p0 {p[k] - p0[k]!r}; oracle v {vo[k]!r} p-p0 {po[k] - p0[k]!r}")
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((p, m, v), (po, mo, vo)))
    pf, _, mf, vf, _ = adam_f64(p0, g, m0, v0, LR, B1, B2, EPS, 1, max_norm=max_norm)
    assert abs(p[k] - pf[k]) <= P_ABS and abs(m[k] - mf[k]) <= TOL and abs(v[k] - vf[k]) <= TOL


# ----------------------------------------------------------------------------------------- non-finite gradients ---
@pytest.mark.parametrize("mode", ["clip-plain", "clip-fused", "clamp"])
@pytest.mark.parametrize("n", [1025, 2053])
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan], ids=["posinf", "neginf", "nan"])
def test_nonfinite_gradient(dev, oracle, bad, n, mode):
    """One bad element.  n = 1025: the tail element, with a second (idle) workgroup in the grid; n = 2053: an element
    of workgroup 1 of 3, so workgroups that never load the bad element have to get the NaN scale from the norm.  The
    entries of p, m, v that stop being finite are adam_f64's (torch's, by tests/test_optim_ref.py); the bits are the
    oracle's."""
    from gymrl_amd import ops
    k = 1024 if n == 1025 else 1500
    p0, m0, v0 = state(np.random.default_rng(9), n)
    g = mixed_grad(np.random.default_rng(10), n)
    g[k] = bad
    max_norm, clamp = (0.0, 1.0) if mode == "clamp" else (0.5, 0.0)
    got, ref, sq = one_step(ops, dev, oracle, "fused" if mode == "clip-fused" else "plain", p0, g, m0, v0, max_norm, clamp)
    f64 = adam_f64(p0, g, m0, v0, LR, B1, B2, EPS, 1, max_norm=max_norm, clamp_abs=clamp)
    for a, o, f in zip(got, ref, (f64[0], f64[2], f64[3])):
        assert np.array_equal(~np.isfinite(a), ~np.isfinite(f))
        assert same_bits(a, o)
    nonfinite = ~np.isfinite(got[0])
    if mode == "clamp":
        assert nonfinite.sum() == (1 if np.isnan(bad) else 0) and nonfinite[k] == np.isnan(bad)
    else:
        assert nonfinite.sum() == (n if np.isnan(bad) else 1) and nonfinite[k]
        assert np.isnan(sq) if np.isnan(bad) else sq == np.inf


# --------------------------------------------------------------------------------------------- gymrl_soft_update ---
@pytest.mark.parametrize("tau", [0.005, 0.0, 1.0])
@pytest.mark.parametrize("n", TAILS + [1023, 1024, 1025, 1050627])
def test_soft_update(dev, oracle, n, tau):
    from gymrl_amd import ops
    rng = np.random.default_rng(n + 31)
    t0, s0 = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    T, S = Guarded(t0, dev), Guarded(s0, dev)
    ops.soft_update(T.t, S.t, tau)
    got = T.get()
    assert np.array_equal(bits(got), bits(oracle.soft_update(t0, s0, tau)))
    if tau == 0.0:
        assert np.array_equal(bits(got), bits(t0))
    if tau == 1.0:
        assert np.array_equal(bits(got), bits(s0))
    assert T.intact() and S.intact() and np.array_equal(bits(S.get()), bits(s0))


# ------------------------------------------------------------------------------------------------------ refusals ---
def test_refusals(dev):
    """-22 through the binding, and nothing written: a buffer that is only 4-byte aligned (each of p, g, m, v and the
    Polyak target in turn), clipping without a norm, the fused form without clipping."""
    from gymrl_amd import ops
    n = 64
    rng = np.random.default_rng(11)
    arrays = [rng.normal(size=n).astype(np.float32) for _ in range(5)]
    bufs = [Guarded(a, dev) for a in arrays]
    ws, sq = workspace(dev), torch.full((1,), 3.5, dtype=torch.float64, device=dev)
    refused = lambda: pytest.raises(RuntimeError, match="-22")   # noqa: E731
    for bad in range(5):
        p, g, m, v, tgt = (b.shifted() if i == bad else b.t for i, b in enumerate(bufs))
        with refused():
            ops.adam_step(p, g, m, v, LR, B1, B2, EPS, 1, polyak_target=tgt, tau=TAU)
        with refused():
            ops.clip_adam_step(p, g, m, v, LR, B1, B2, EPS, 1, 0.5, ws, sqnorm_out=sq, polyak_target=tgt, tau=TAU)
    P, G, M, V, T = bufs
    with refused():
        ops.sqnorm(G.shifted(), sq, ws)
    with refused():
        ops.soft_update(T.shifted(), P.t, TAU)
    with refused():
        ops.soft_update(T.t, P.shifted(), TAU)
    with refused():
        ops.clip_adam_step(P.t, G.t, M.t, V.t, LR, B1, B2, EPS, 1, 0.0, ws, sqnorm_out=sq)
    with refused():
        ops.adam_step(P.t, G.t, M.t, V.t, LR, B1, B2, EPS, 1, max_grad_norm=0.5, sqnorm_buf=None)
    for b, a in zip(bufs, arrays):
        assert b.intact() and np.array_equal(bits(b.get()), bits(a))
    assert float(sq.item()) == 3.5 and bool((ws == WS_SENT).all())


def test_fused_step_without_parameters_zeroes_the_norm(dev):
    """gymrl_clip_adam_step at n = 0 writes 0.0 over sqnorm_out: a reader never sees the previous step's norm.  Through
    the C ABI itself: an empty tensor has no address to hand to gymrl_amd.ops."""
    from gymrl_amd._lib import lib
    arrays = [np.full(4, 1.5 + i, np.float32) for i in range(4)]
    bufs = [Guarded(a, dev) for a in arrays]
    ws, sq = workspace(dev), torch.full((1,), 3.5, dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    rc = lib().gymrl_clip_adam_step(*(ptr(b.t) for b in bufs), 0, LR, None, B1, B2, EPS, 1, None, 1.0, 0.5, ptr(sq), 0.0, 1,
                                    None, 0.0, ptr(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert float(sq.item()) == 0.0 and bool((ws == WS_SENT).all())
    for b, a in zip(bufs, arrays):
        assert b.intact() and np.array_equal(bits(b.get()), bits(a))
