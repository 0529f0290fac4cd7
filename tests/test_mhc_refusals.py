"""What the sixteen launching entry points of the mHC backbone (csrc/mhc.hip, mhc_layers.hip, mhc_norm.hip) refuse with -22 before
anything touches HIP: a missing required pointer, a shape outside the documented limits, operands the shape-chosen kernels
cannot take.  CPU only: every call here carries at least one reason for refusal, or B = 0 where the entry point returns 0
before it launches — a fully valid call would launch on the dummy addresses below."""
import ctypes

import pytest

DUMMY = 0x1000                # a non-null, 16-byte aligned host address: never dereferenced
ODD = DUMMY + 4               # not 16-byte aligned
BAD_ACT = 99                  # neither GYMRL_ACT_NONE nor GYMRL_ACT_SILU

# entry point -> its arguments in order (the stream, always last and null, is left out): "name" a required pointer, "name?" an
# optional one, (name, legal value) a scalar.  zero: B = 0 returns 0 before launching (else B < 1 is refused).
# limits: overrides of a legal call, each of which must be refused.
_NBD = (("n", 3), ("n", 0), ("B", -1))
CASES = {
    "mhc_gates": dict(args=("h", "norm_w", "w", "alpha", "beta", ("B", 5), ("n", 2), ("D", 128), ("sk_it", 10), "pre", "post", "mix",
                            "read", "stats?"), zero=True,
                      limits=_NBD + (("D", 126), ("D", 0), ("sk_it", -1), dict(stats=DUMMY, n=4, D=32), dict(stats=DUMMY, D=64))),
    "mhc_combine": dict(args=("post", "mix", "out", "h", ("B", 5), ("n", 2), ("D", 128), ("act", 0), "h_out"), zero=True,
                        limits=_NBD + (("D", 0), ("act", BAD_ACT))),
    "mhc_read_fwd": dict(args=("pre", "h", ("B", 5), ("n", 2), ("D", 128), "read"), zero=True, limits=_NBD + (("D", 126), ("D", 0))),
    "mhc_read_bwd": dict(args=("g", "pre", "h", ("B", 5), ("n", 2), ("D", 128), "d_pre", "d_h?", ("accumulate", 0)), zero=True,
                         limits=_NBD + (("D", 0),)),
    "mhc_combine_bwd": dict(args=("g", "post", "mix", "out", "h", ("B", 5), ("n", 2), ("D", 128), ("act", 0), "d_post", "d_mix", "d_out",
                                  "d_h?"), zero=True, limits=_NBD + (("D", 0), ("act", BAD_ACT))),
    "mhc_gates_bwd": dict(args=("h", "norm_w", "w", "alpha", "pre", "post", "mix", "stats", "d_pre", "d_post", "d_mix", "d_read?", "g_out?",
                                ("B", 5), ("n", 2), ("D", 128), "d_h", "d_norm_w", "d_w", "d_alpha", "d_beta", "workspace"), zero=False,
                          limits=(("n", 4), ("n", 3), ("D", 64), ("D", 512), ("D", 126), ("B", -1))),
    "sinkhorn": dict(args=("A", ("B", 5), ("n", 2), ("sk_it", 10), "u", "v"), zero=True, limits=_NBD + (("sk_it", -1),)),
    "rmsnorm": dict(args=("x", "w", ("B", 5), ("D", 128), ("n_sum", 1), ("eps", 1e-6), ("act", 0), "y"), zero=True,
                    limits=(("B", -1), ("D", 0), ("n_sum", 0), ("act", BAD_ACT))),
    "rmsnorm_bwd": dict(args=("g", "x", "w", ("B", 5), ("D", 128), ("eps", 1e-6), ("act", 0), "d_x", "d_w", "workspace"), zero=False,
                        limits=(("B", -1), ("D", 0), ("D", 513), ("act", BAD_ACT))),
    "rmsnorm_sum_bwd": dict(args=("g", "x", "w", ("B", 5), ("D", 128), ("n_sum", 2), ("eps", 1e-6), ("act", 0), "d_x", "d_w", "workspace"),
                            zero=False, limits=(("B", -1), ("D", 0), ("D", 513), ("n_sum", 0), ("act", BAD_ACT))),
    # D = 256 takes the four-row kernels by SHAPE and therefore requires 16-byte aligned operands
    "norm_proj_fwd": dict(args=("x", "norm_w", "W2", "b2?", ("B", 5), ("D", 128), ("n_out", 4), ("eps", 1e-6), "out"), zero=True,
                          limits=(("B", -1), ("D", 0), ("D", 257), ("n_out", 0), ("n_out", 9), dict(D=256, x=ODD), dict(D=256, norm_w=ODD),
                                  dict(D=256, W2=ODD))),
    "norm_proj_bwd": dict(args=("d_out", "x", "norm_w", "W2", ("B", 5), ("D", 128), ("n_out", 4), ("eps", 1e-6), "d_x", "d_norm_w", "d_W2",
                                "d_b2", "workspace"), zero=False,
                          limits=(("B", -1), ("D", 0), ("D", 257), ("n_out", 0), ("n_out", 9), dict(D=256, n_out=1, x=ODD),
                                  dict(D=256, n_out=1, norm_w=ODD), dict(D=256, n_out=1, W2=ODD), dict(D=256, n_out=1, d_x=ODD))),
    "mhc_sub_forward": dict(args=("h", ("h_broadcast", 0), "norm_w", "w", "alpha", "beta", "lin_w", "lin_b", ("B", 5), ("n", 2), ("D", 128),
                                  ("sk_it", 10), "pre", "post", "mix", "stats", "read", "z", "h_out"), zero=True,
                            limits=(("B", -1), ("n", 4), ("D", 256), ("D", 64), ("sk_it", -1))),
    "mhc_sub_backward": dict(args=("g", ("g_broadcast", 0), "h", ("h_broadcast", 0), "z", "pre", "post", "mix", "stats", "norm_w", "w", "alpha",
                                   "lin_w", ("B", 5), ("n", 2), ("D", 128), "d_z", "d_h", ("sum_branches", 0), "d_norm_w", "d_w", "d_alpha",
                                   "d_beta", "workspace"), zero=False, limits=(("B", -1), ("n", 4), ("D", 256), ("D", 64))),
}


def _call(name, **over):
    """Entry point `name` on a legal argument list with `over` written over it (an optional pointer is null unless given)."""
    from gymrl_amd import _lib
    assert over, "a fully valid call would launch"
    vals = []
    for a in CASES[name]["args"]:
        key, legal = (a.rstrip("?"), None if a.endswith("?") else DUMMY) if isinstance(a, str) else a
        v = over.pop(key, legal)
        vals.append(ctypes.c_void_p(v) if isinstance(a, str) else v)
    assert not over, over
    return getattr(_lib.lib(), "gymrl_" + name)(*vals, ctypes.c_void_p(None))


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_required_pointer_is_required(name):
    for a in CASES[name]["args"]:
        if isinstance(a, str) and not a.endswith("?"):
            assert _call(name, **{a: None}) == -22, a


@pytest.mark.parametrize("name", sorted(CASES))
def test_documented_limits(name):
    for lim in CASES[name]["limits"]:
        over = dict(lim) if isinstance(lim, dict) else {lim[0]: lim[1]}
        assert _call(name, **over) == -22, lim


@pytest.mark.parametrize("name", sorted(CASES))
def test_an_empty_batch(name):
    """B = 0: nothing to do (0, before anything launches) — or refused, where the entry point asks for B >= 1."""
    assert _call(name, B=0) == (0 if CASES[name]["zero"] else -22)


# ---- the one-launch policy forward and its image: a descriptor struct -------------------------------------------------------
def _policy(n_sub=2):
    from gymrl_amd import _lib
    p = _lib.MhcPolicy()
    p.obs_dim, p.n_sub, p.n_act, p.sk_it = 8, n_sub, 4, 10
    p.in_w = p.in_b = p.final_norm_w = DUMMY
    for s in range(n_sub):
        for f, _ in _lib.MhcSub._fields_:
            setattr(p.sub[s], f, DUMMY)
    for h in range(2):
        for f in ("w1", "b1", "norm_w", "w2", "b2"):
            setattr(p.head[h], f, DUMMY)
    return p


def _policy_refusals():
    """(what, descriptor) pairs, each descriptor refused by policy_fill."""
    from gymrl_amd import _lib
    for f, v in (("obs_dim", 0), ("obs_dim", 17), ("n_sub", -1), ("n_sub", 9), ("n_act", 0), ("n_act", 9), ("sk_it", -1), ("in_w", None),
                 ("in_b", None), ("final_norm_w", None)):
        p = _policy()
        setattr(p, f, v)
        yield (f, v), p
    for s in range(2):
        for f, _ in _lib.MhcSub._fields_:
            p = _policy()
            setattr(p.sub[s], f, None)
            yield ("sub", s, f), p
    for h in range(2):
        for f in ("w1", "b1", "norm_w", "w2", "b2"):
            p = _policy()
            setattr(p.head[h], f, None)
            yield ("head", h, f), p


def test_policy_forward_refusals():
    from gymrl_amd import _lib
    fwd = _lib.lib().gymrl_mhc_policy_forward
    null, ok = ctypes.c_void_p(None), ctypes.c_void_p(DUMMY)
    p = _policy()
    assert fwd(None, ok, 5, ok, ok, null) == -22
    for obs, logits, value in ((null, ok, ok), (ok, null, ok), (ok, ok, null)):
        assert fwd(ctypes.byref(p), obs, 5, logits, value, null) == -22
    assert fwd(ctypes.byref(p), ok, -1, ok, ok, null) == -22
    for what, q in _policy_refusals():
        assert fwd(ctypes.byref(q), ok, 5, ok, ok, null) == -22, what
    p.image = ODD                                           # the packed image is read in 16-byte pieces
    assert fwd(ctypes.byref(p), ok, 5, ok, ok, null) == -22
    p.image = None
    assert fwd(ctypes.byref(p), ok, 0, ok, ok, null) == 0   # an empty batch: 0 before anything launches


def test_policy_pack_refusals():
    from gymrl_amd import _lib
    pack = _lib.lib().gymrl_mhc_policy_pack
    null = ctypes.c_void_p(None)
    p = _policy()
    assert pack(None, ctypes.c_void_p(DUMMY), null) == -22
    assert pack(ctypes.byref(p), null, null) == -22
    assert pack(ctypes.byref(p), ctypes.c_void_p(ODD), null) == -22          # a misaligned image
    for what, q in _policy_refusals():
        assert pack(ctypes.byref(q), ctypes.c_void_p(DUMMY), null) == -22, what
    assert _lib.lib().gymrl_mhc_policy_image_floats(9) == 0 and _lib.lib().gymrl_mhc_policy_image_floats(-1) == 0
