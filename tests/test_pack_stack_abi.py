"""CPU-side checks of the population packing launch's boundary: gymrl_mlp_pack_stack declared, exported and mirrored, its argument
struct the size the library reports, every refusal of include/gymrl.h returned as -22 before anything is launched (no GPU here),
the wrappers' own refusals, the numpy restatement (tests/pack_stack_ref.py) grounded on a hand-written weight, and the surface
es_lunarlander gained (Config.policy, the checkpoint's policy name)."""
import ctypes

import numpy as np
import pytest

import pack_stack_ref as ref
from test_abi import _agrees, _mirrors, _parse_header

FAKE = 256                                             # never dereferenced: validation fails first
NAME, SIZE = "gymrl_mlp_pack_stack", "gymrl_mlp_pack_stack_args_bytes"
FIELDS = ["P", "n_layers", "params", "params_stride", "packed", "packed_stride", "layer"]
LAYER_FIELDS = ["out_dim", "in_dim", "w_off", "b_off", "w_at", "b_at"]


def test_header_declares_and_binding_mirrors_the_entry_point():
    from gymrl_amd import _lib
    functions, structs = _parse_header()
    mirrors = _mirrors()
    L = _lib.lib()
    assert NAME in functions and SIZE in functions and hasattr(L, NAME) and hasattr(L, SIZE)
    _, params = functions[NAME]
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 2
    for ct, htype in zip(argtypes, params):
        assert _agrees(ct, htype, mirrors)
    assert _lib.SIGNATURES[SIZE] == (ctypes.c_size_t, [])
    assert [f for f, _ in structs["gymrl_mlp_pack_stack_args"]] == [f for f, _ in _lib.MlpPackStackArgs._fields_] == FIELDS
    assert [f for f, _ in structs["gymrl_mlp_pack_layer"]] == [f for f, _ in _lib.MlpPackLayer._fields_] == LAYER_FIELDS
    assert _lib.MlpPackStackArgs._c_name_ == "gymrl_mlp_pack_stack_args" and _lib.MlpPackLayer._c_name_ == "gymrl_mlp_pack_layer"
    assert getattr(L, SIZE)() == ctypes.sizeof(_lib.MlpPackStackArgs) == 40 + _lib.MLP_MAX_STAGES * ctypes.sizeof(_lib.MlpPackLayer)
    assert ctypes.sizeof(_lib.MlpPackLayer) == 40
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION           # an addition
    # a section of its own directly behind the forward it packs for, the table in the header's order, not at the header's end
    names, table = list(functions), list(_lib.SIGNATURES)
    for order in (names, table):
        at = order.index("gymrl_mlp_forward")
        assert order[at + 1:at + 4] == [SIZE, NAME, "gymrl_rollout_lunar"]
    assert names[-1] == "gymrl_mountaincar_rule_eval"


def _call(layers=((4, 8, 0, 32, 0, 1024),), **kw):
    """One field away from an argument block that passes every check (it is never sent as it is: its pointers are fakes): a
    (4, 8) layer, weight then bias in a row of 36 floats, image (1024 floats) then bias in a row of 1028."""
    from gymrl_amd import _lib
    a = _lib.MlpPackStackArgs()
    a.P, a.n_layers, a.params, a.params_stride, a.packed, a.packed_stride = 2, len(layers), FAKE, 36, FAKE, 1028
    for e, layer in zip(a.layer, layers):
        e.out_dim, e.in_dim, e.w_off, e.b_off, e.w_at, e.b_at = layer
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return _lib.lib().gymrl_mlp_pack_stack(ctypes.byref(a), None)


def test_every_refusal_is_einval_before_any_launch():
    from gymrl_amd import _lib
    L = _lib.lib()
    assert L.gymrl_mlp_pack_stack(None, None) == -22
    assert _call(params=None) == -22 and _call(packed=None) == -22
    for P in (0, -1, 65536, 1 << 20):
        assert _call(P=P) == -22, P
    for n in (0, -1, _lib.MLP_MAX_STAGES + 1):
        assert _call(n_layers=n) == -22, n
    ok = (4, 8, 0, 32, 0, 1024)
    for field, bad in ((0, 0), (0, -4), (1, 0), (1, -8), (0, _lib.MLP_MAX_WIDTH + 1), (1, _lib.MLP_MAX_WIDTH + 1)):
        layer = list(ok)
        layer[field] = bad
        assert _call(layers=(tuple(layer),)) == -22, (field, bad)
    for field in (2, 3, 4, 5):                                        # a negative offset
        layer = list(ok)
        layer[field] = -4
        assert _call(layers=(tuple(layer),)) == -22, field
    assert _call(layers=((4, 8, 5, 0, 0, 1024),)) == -22              # w_off + 32 = 37 > 36
    assert _call(layers=((4, 8, 0, 33, 0, 1024),)) == -22             # b_off + 4 = 37 > 36
    assert _call(params_stride=35) == -22 and _call(params_stride=-36) == -22
    for field, bad in ((4, 2), (5, 1026), (4, 1), (5, 1025)):           # w_at / b_at % 4
        layer = list(ok)
        layer[field] = bad
        assert _call(layers=(tuple(layer),)) == -22, (field, bad)
    assert _call(packed_stride=1030) == -22 and _call(packed_stride=-1028) == -22
    assert _call(packed_stride=1024) == -22                           # the bias ends at 1028
    assert _call(layers=((4, 8, 0, 32, 0, 1028),)) == -22             # the bias ends beyond the row
    assert _call(layers=((4, 8, 0, 32, 8, 0),)) == -22                # the image ends at 1032
    assert _call(layers=((4, 8, 0, 32, 0, 512),)) == -22              # the bias inside the image
    assert _call(layers=((4, 8, 0, 32, 0, 1020),)) == -22             # the bias on the image's last float4
    assert _call(layers=((1, 8, 0, 8, 0, 2048), (1, 8, 9, 17, 1024, 2048)), params_stride=18, packed_stride=2052) == -22   # two biases, one place
    assert _call(layers=((4, 8, 0, 32, 0, 2048), (4, 8, 0, 32, 512, 2052)), packed_stride=2056) == -22                  # two images overlap
    for addr in (260, 264, 258):                                      # 16-byte stores
        assert _call(packed=addr) == -22, addr
    for addr in (257, 258, 259):                                      # float loads
        assert _call(params=addr) == -22, addr
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_mlp_pack_stack(ctypes.byref(_lib.MlpDesc()), None)   # another struct's pointer


def test_the_numpy_restatement_on_a_hand_written_weight():
    """A 2 x 3 weight, float by float: one tile, K padded 3 -> 64 (four K-blocks), lane l of K-block kb holds row l & 15, columns
    16 kb + 4 (l >> 4) .. + 3."""
    W = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], dtype=np.float32)
    image = ref.pack_image(W)
    assert ref.packed_floats(2, 3) == image.size == 1 * 4 * 64 * 4 == 1024
    expected = np.zeros(1024, dtype=np.float32)
    expected[0:3] = [1.0, 2.0, 3.0]           # K-block 0, lane 0: row 0, columns 0..3 (column 3 is beyond in_dim)
    expected[4:7] = [4.0, 5.0, 6.0]           # K-block 0, lane 1: row 1
    assert np.array_equal(image.view(np.uint32), expected.view(np.uint32))
    assert ref.packed_floats(4, 8) == 1024 and ref.packed_floats(5, 72) == 2048 and ref.packed_floats(17, 64) == 2048
    assert ref.packed_floats(256, 256) == 16 * 16 * 256
    # a column past the first float4 lands in lane 16 (l >> 4 == 1), a row past the first tile in tile 1
    W = np.zeros((17, 20), dtype=np.float32)
    W[3, 6], W[16, 19] = 7.0, 9.0
    image = ref.pack_image(W).reshape(2, 4, 64, 4)
    assert image[0, 0, 16 + 3, 2] == 7.0 and image[1, 1, 0, 3] == 9.0 and np.count_nonzero(image) == 2
    # the stack: the bias padded with zeros, everything else untouched
    params = np.arange(2 * 10, dtype=np.float32).reshape(2, 10) + 1.0
    layers = [(2, 3, 1, 7, 8, 0)]                                     # bias in front of the image, a gap of 4 between them
    sentinel = np.full((2, 8 + 1024 + 4), -7.0, dtype=np.float32)
    out = ref.pack_stack(params, layers, sentinel)
    mask = ref.written_mask(layers, sentinel.shape[1])
    assert mask.sum() == 4 + 1024 and not mask[4:8].any() and not mask[-4:].any()
    assert np.all(out[:, ~mask] == -7.0)
    assert out[1, 0:4].tolist() == [18.0, 19.0, 0.0, 0.0]
    assert out[1, 8:12].tolist() == [12.0, 13.0, 14.0, 0.0] and out[1, 12:16].tolist() == [15.0, 16.0, 17.0, 0.0]
    assert ref.tight_layout([(4, 8), (1, 8)]) == ([0, 1024], [2048, 2052], 2056)


def test_the_wrappers_refuse_cpu_tensors_wrong_dtypes_and_other_shapes():
    import torch
    from gymrl_amd import ops
    from gymrl_amd.ppo_lunarlander import ActorCritic
    params, packed, layers = torch.zeros(2, 36), torch.zeros(2, 1028), [(4, 8, 0, 32, 0, 1024)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mlp_pack_stack(params, layers, packed)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mlp_pack_stack(params.to("meta"), layers, packed)         # one of the two elsewhere is no better
    with pytest.raises(ValueError):
        ops.mlp_pack_stack(params[0], layers, packed)                 # not [P, n]
    fused = ActorCritic(8, 4, 64)._act_net()
    flat = torch.zeros(16)
    with pytest.raises(ValueError, match="stack"):
        ops.LunarPolicyStack(fused, flat, torch.zeros(2, 16))         # not on the device
    with pytest.raises(ValueError, match="stack"):
        ops.LunarPolicyStack(fused, flat, torch.zeros(2, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match="out is a LunarPolicyStack"):
        ops.LunarPolicyStack(fused, flat, torch.zeros(2, 16), out=torch.zeros(2, 16))
    earlier = object.__new__(ops.LunarPolicyStack)                    # a stack of three policies, as an earlier call left it
    earlier.P, earlier.stride, earlier.buffer = 3, 16, torch.zeros(3, 16)
    with pytest.raises(ValueError, match="another shape"):
        ops.LunarPolicyStack(fused, flat, torch.zeros(2, 16), out=earlier)
    with pytest.raises(ValueError, match="stack"):
        ops.LunarPolicyStack(fused, flat, torch.zeros(3, 16), out=earlier)       # the right count, still not on the device
    with pytest.raises(ValueError, match="in place"):
        ops.MlprnnPolicyStack(None, flat, torch.zeros(2, 16), copy=False)        # not on the device
    with pytest.raises(ValueError, match="in place"):
        ops.MlprnnPolicyStack(None, flat, torch.zeros(2, 12), copy=False)        # rows shorter than the network


def test_dtype_refusals_need_no_device():
    """A wrong dtype is refused as such wherever the tensor lives: the device check comes first, so this is stated on the
    wrapper's helper."""
    import torch
    from gymrl_amd import ops

    class OnDevice:                        # what the helper reads of a tensor, claiming to be on the device
        def __init__(self, t):
            self.t = t
        is_cuda = True
        dtype = property(lambda self: self.t.dtype)
        shape = property(lambda self: self.t.shape)
        dim = lambda self: self.t.dim()
        stride = lambda self, i: self.t.stride(i)
        data_ptr = lambda self: 256

    with pytest.raises(TypeError, match="float32"):
        ops._dense_rows(OnDevice(torch.zeros(2, 8, dtype=torch.float64)), "mlp_pack_stack", "params")
    with pytest.raises(TypeError, match="float32"):
        ops._dense_rows(OnDevice(torch.zeros(2, 8, dtype=torch.int32)), "mlp_pack_stack", "packed")
    with pytest.raises(ValueError, match="dense"):
        ops._dense_rows(OnDevice(torch.zeros(8, 2).t()), "mlp_pack_stack", "params")
    assert ops._dense_rows(OnDevice(torch.zeros(4, 16)[:, :8]), "mlp_pack_stack", "params") == (256, 16)
    assert ops._dense_rows(OnDevice(torch.zeros(1, 8)), "mlp_pack_stack", "params") == (256, 8)


def test_es_lunarlander_states_its_new_surface():
    from gymrl_amd import es_lunarlander
    cfg = es_lunarlander.Config()
    assert cfg.policy == "mlp" and es_lunarlander.POLICIES == ("mlp", "mlprnn")
    with pytest.raises(ValueError, match="policy"):
        es_lunarlander.check_policy({"policy": "mlprnn"}, "mlp")
    with pytest.raises(ValueError, match="policy"):
        es_lunarlander.check_policy({"policy": "mlp"}, "mlprnn")
    with pytest.raises(ValueError, match="policy"):
        es_lunarlander.check_policy({}, "mlprnn")                     # a checkpoint from before there was a choice
    es_lunarlander.check_policy({}, "mlp")
    es_lunarlander.check_policy({"policy": "mlprnn"}, "mlprnn")
    from gymrl_amd.utils.cli import apply_overrides
    assert apply_overrides(es_lunarlander.Config(), ["--policy", "mlprnn"]).policy == "mlprnn"
