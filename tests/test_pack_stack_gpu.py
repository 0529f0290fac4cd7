"""gymrl_mlp_pack_stack on the GPU: every float of every packed row against tests/pack_stack_ref.py AND against the launch per
layer and policy it replaces (ops.mlp_pack plus a bias copy, restated below as the constructor of ops.LunarPolicyStack had it), bit
for bit, at the smallest shapes where the layout can go wrong; then the two stacks built on it."""
import numpy as np
import pytest

import pack_stack_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
# layers as (out_dim, in_dim)
CASES = {
    "a": [(4, 8), (1, 8)],                  # one tile, K padded 8 -> 64, a bias of 4 and of 1
    "b": [(5, 72)],                         # K rounds to 128, a partial tile, bias padding of 3
    "c": [(17, 64), (16, 16)],              # a second tile holding one row, no padding in K
    "d": None,                              # PPO's hidden-64 network: the stages of a real FusedMLP (ppo_net.LAYOUT's offsets)
}
VARIANTS = ("tight", "wide", "slice", "shuffled")


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def ppo_net64():
    """(ActorCritic(8, 4, 64) on the device, its flat buffer, its FusedMLP)."""
    from gymrl_amd import ppo_net
    from gymrl_amd.flat import flatten_module
    from gymrl_amd.ppo_lunarlander import ActorCritic
    g = torch.random.get_rng_state()
    torch.manual_seed(11)
    model = ActorCritic(8, 4, 64)
    torch.random.set_rng_state(g)
    flat, _ = flatten_module(model, dev(), order=ppo_net.LAYOUT)
    return model, flat, model._act_net()


def case_layout(case, variant):
    """-> (layers with offsets, floats a params row must hold, packed stride).  "shuffled" lays the parameters out last layer
    first with the biases in front, and the packed ranges in yet another order with gaps; the others ascend."""
    if CASES[case] is None:
        _, flat, fused = ppo_net64()
        mods = [m for m, _, _, _ in fused.stages]
        shapes = [tuple(m.weight.shape) for m in mods]
        assert shapes[0] == (64, 8) and shapes[1] == (64, 64) and sorted(o for o, _ in shapes)[:2] == [1, 4] and len(shapes) == 6
        own = [((m.weight.data_ptr() - flat.data_ptr()) // 4, (m.bias.data_ptr() - flat.data_ptr()) // 4) for m in mods]
        extent = flat.numel()
    else:
        shapes, own = CASES[case], None
    L = len(shapes)
    if variant == "shuffled" or own is None:
        order = list(range(L))
        pieces = [("b", k) for k in reversed(order)] + [("w", k) for k in reversed(order)] if variant == "shuffled" else \
                 [(kind, k) for k in order for kind in ("w", "b")]
        at, off = 3 if variant == "shuffled" else 0, {}
        for kind, k in pieces:
            off[kind, k] = at
            at += shapes[k][0] * (shapes[k][1] if kind == "w" else 1) + (2 if variant == "shuffled" else 0)
        own, extent = [(off["w", k], off["b", k]) for k in range(L)], at
    if variant == "shuffled":
        sizes = {("w", k): ref.packed_floats(*shapes[k]) for k in range(L)}
        sizes.update({("b", k): (shapes[k][0] + 3) // 4 * 4 for k in range(L)})
        at, where = 8, {}
        for key in [("b", k) for k in range(L)][::-1] + [("w", k) for k in range(1, L)] + [("w", 0)]:
            where[key] = at
            at += sizes[key] + 4                                     # a float4 of padding behind every range
        w_at, b_at, stride = [where["w", k] for k in range(L)], [where["b", k] for k in range(L)], at + 12
    else:
        w_at, b_at, stride = ref.tight_layout(shapes)
        if variant == "wide":
            stride += 20
    layers = [(o, i, own[k][0], own[k][1], w_at[k], b_at[k]) for k, (o, i) in enumerate(shapes)]
    return layers, extent, stride


def make_params(P, extent, variant, seed):
    """f32[P, extent] of distinct values on the device: contiguous, rows further apart than their extent, or a slice of a wider
    tensor that starts 4-byte aligned only."""
    rng = np.random.default_rng(seed)
    values = torch.from_numpy(rng.standard_normal((P, extent)).astype(np.float32)).to(dev())
    if variant == "tight":
        return values
    wide = torch.full((P, extent + 13), 777.0, dtype=torch.float32, device=dev())
    lo = 5 if variant in ("slice", "shuffled") else 0
    wide[:, lo:lo + extent] = values
    view = wide[:, lo:lo + extent]
    assert P == 1 or not view.is_contiguous()
    return view


def loop_pack(params, layers, packed):
    """The launches this replaces: gymrl_mlp_pack into the row's range and a bias copy, per layer and policy.  (The constructor
    wrote into a zeroed buffer; here the padding of a bias is zeroed by hand, the buffer holds a sentinel.)"""
    from gymrl_amd import ops
    for p in range(params.shape[0]):
        for o, i, w_off, b_off, w_at, b_at in layers:
            W = params[p, w_off:w_off + o * i].view(o, i)
            ops.mlp_pack(W, packed[p, w_at:w_at + ref.packed_floats(o, i)])
            packed[p, b_at:b_at + (o + 3) // 4 * 4] = 0.0
            packed[p, b_at:b_at + o] = params[p, b_off:b_off + o]
    return packed


def bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def check(params, layers, stride):
    from gymrl_amd import ops
    P = params.shape[0]
    packed = torch.full((P, stride), SENTINEL, dtype=torch.float32, device=dev())
    assert ops.mlp_pack_stack(params, layers, packed) is packed
    got = packed.cpu().numpy()
    mask = ref.written_mask(layers, stride)
    assert np.all(got[:, ~mask] == np.float32(SENTINEL)), "a float outside the 2 L ranges was written"
    want = ref.pack_stack(params.cpu().numpy(), layers, np.full((P, stride), SENTINEL, dtype=np.float32))
    assert np.array_equal(bits(got), bits(want)), "not the restated contract's bits"
    by_loop = loop_pack(params, layers, torch.full((P, stride), SENTINEL, dtype=torch.float32, device=dev()))
    assert np.array_equal(bits(got), bits(by_loop)), "not the bits of the launch per layer and policy"
    assert not np.any(got[:, mask] == np.float32(SENTINEL))          # the ranges are written whole (no value is the sentinel)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("case", sorted(CASES))
def test_pack_stack_is_the_contract_and_the_loop_bit_for_bit(case, P, variant):
    layers, extent, stride = case_layout(case, variant)
    if variant == "shuffled":
        offs, ats = [v for l in layers for v in l[2:4]], [v for l in layers for v in l[4:6]]
        assert offs != sorted(offs) and ats != sorted(ats)            # neither side ascends: the bias lies in front of its weight
        assert stride > ref.tight_layout([l[:2] for l in layers])[2]
    check(make_params(P, extent, variant, seed=P), layers, stride)


def test_pack_stack_past_a_wave_of_policies():
    """gridDim.y = 300: every row its own policy's."""
    layers, extent, stride = case_layout("a", "wide")
    check(make_params(300, extent, "wide", seed=5), layers, stride)


def loop_stack_buffer(fused, flat, params, stride=None):
    """ops.LunarPolicyStack's buffer as its constructor's double loop filled it: zeros, then a launch and a copy per layer and
    policy."""
    mods = [m for m, _, _, _ in fused.stages]
    shapes = [tuple(m.weight.shape) for m in mods]
    w_at, b_at, tight = ref.tight_layout(shapes)
    own = [((m.weight.data_ptr() - flat.data_ptr()) // 4, (m.bias.data_ptr() - flat.data_ptr()) // 4) for m in mods]
    layers = [(o, i, own[k][0], own[k][1], w_at[k], b_at[k]) for k, (o, i) in enumerate(shapes)]
    buffer = torch.zeros(params.shape[0], tight if stride is None else stride, dtype=torch.float32, device=params.device)
    return loop_pack(params.contiguous(), layers, buffer)


def perturbed(flat, P, seed, pad=0):
    rng = np.random.default_rng(seed)
    noise = torch.from_numpy(rng.standard_normal((P, flat.numel() + pad)).astype(np.float32)).to(flat.device)
    noise[:, :flat.numel()] = flat + 0.1 * noise[:, :flat.numel()]
    return noise


def test_lunar_policy_stack_is_the_loops_buffer_and_refills_in_place():
    from gymrl_amd import ops
    _, flat, fused = ppo_net64()
    first, second = perturbed(flat, 3, 1), perturbed(flat, 3, 2, pad=8)[:, :flat.numel() + 4]      # the second: strided rows
    assert not second.is_contiguous()
    stack = ops.LunarPolicyStack(fused, flat, first)
    assert np.array_equal(bits(stack.buffer), bits(loop_stack_buffer(fused, flat, first)))
    padded = ops.LunarPolicyStack(fused, flat, first, stride=stack.stride + 20)
    assert np.array_equal(bits(padded.buffer), bits(loop_stack_buffer(fused, flat, first, stack.stride + 20)))
    address, desc_w = stack.buffer.data_ptr(), [stack.desc.stage[k].W for k in range(6)]
    again = ops.LunarPolicyStack(fused, flat, second, out=stack)
    assert again is stack and stack.buffer.data_ptr() == address and [stack.desc.stage[k].W for k in range(6)] == desc_w
    assert np.array_equal(bits(stack.buffer), bits(loop_stack_buffer(fused, flat, second)))
    assert not np.array_equal(bits(stack.buffer), bits(padded.buffer[:, :stack.stride]))
    with pytest.raises(ValueError, match="another shape"):
        ops.LunarPolicyStack(fused, flat, first[:2], out=stack)
    with pytest.raises(ValueError, match="another shape"):
        ops.LunarPolicyStack(fused, flat, first, stride=stack.stride + 4, out=stack)
    with pytest.raises(ValueError, match="out is a LunarPolicyStack"):
        ops.LunarPolicyStack(fused, flat, first, out=stack.buffer)


def test_lunar_policy_eval_on_the_stack_is_three_single_launches():
    from gymrl_amd import ops
    _, flat, fused = ppo_net64()
    params = perturbed(flat, 3, 7)
    stack = ops.LunarPolicyStack(fused, flat, params)
    seed, id0 = 42 + 1_000_003, 1 << 40
    together = ops.lunar_policy_eval(stack, 2, seed, id0, cap=60)
    for p in range(3):
        flat.copy_(params[p])
        fused.refresh()
        alone = ops.lunar_policy_eval(fused, 2, seed, id0, cap=60)
        assert len(alone) == len(together) == 4
        for t, a in zip(together, alone):
            assert torch.equal(t[p:p + 1].contiguous().view(torch.uint8), a.contiguous().view(torch.uint8)), p
    assert len(torch.unique(together[0])) > 1


def test_mlprnn_stack_in_place_is_the_copying_stack():
    from gymrl_amd import ops
    from gymrl_amd.flat import flatten_module
    from gymrl_amd.ppg_rnn_lunarlander import ActorCriticPPG
    g = torch.random.get_rng_state()
    torch.manual_seed(5)
    net = ActorCriticPPG(8, 4, hidden_size=64)
    torch.random.set_rng_state(g)
    named = [n for n, _ in net.named_parameters()]
    critic = [n for n in named if n.startswith("critic_fc.")]
    aux = [n for n in named if n.startswith("aux_critic_fc.")]
    flat, _ = flatten_module(net, dev(), order=critic + [n for n in named if n not in critic and n not in aux] + aux)
    n = flat.numel()
    rows = perturbed(flat, 3, 9, pad=(-n) % 4 + 8)                   # f32[3, stride]: a learner's population buffer
    assert rows.shape[1] % 4 == 0 and rows.shape[1] > n
    copying = ops.MlprnnPolicyStack(net, flat, rows[:, :n])
    in_place = ops.MlprnnPolicyStack(net, flat, rows, copy=False)
    assert in_place.buffer is rows and in_place.stride == rows.shape[1] and in_place.P == 3
    assert copying.buffer.data_ptr() != rows.data_ptr()
    assert in_place.desc.lin_w - rows.data_ptr() == copying.desc.lin_w - copying.buffer.data_ptr()
    seed, id0 = 42 + 1_000_003, 1 << 40
    a = ops.lunar_mlprnn_eval(copying, 2, seed, id0, cap=60, want_h_final=True)
    b = ops.lunar_mlprnn_eval(in_place, 2, seed, id0, cap=60, want_h_final=True)
    for x, y in zip(a, b):
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
    assert len(torch.unique(a[0])) > 1
    with pytest.raises(ValueError, match="in place"):
        ops.MlprnnPolicyStack(net, flat, rows[:, 1:], copy=False)    # rows 4-byte aligned only
    with pytest.raises(ValueError, match="in place"):
        ops.MlprnnPolicyStack(net, flat, rows, stride=rows.shape[1] + 4, copy=False)
