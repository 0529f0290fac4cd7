"""What the four classic-control episode evaluators refuse alike, on the smallest block each of them takes (P = 1, E = 1, H = 4):
the TimeLimit of the env as the largest `cap`, and the shared rules on sizes, streams, the stride, `images` and the outputs.
Every refusal is -22 before the first HIP call, so nothing here is launched.

The one call per case that PASSES the argument checks (cap == TimeLimit) cannot hide behind fake pointers where a device is
present: there it is a real launch on real, zeroed tensors (one workgroup, one episode) and returns 0; without a device the
same block on fake pointers gets as far as the first HIP call and returns that call's error, -1000 - hipErrorNoDevice."""
import ctypes

import pytest

CARTPOLE, PENDULUM, MOUNTAINCAR, ACROBOT = 0, 1, 3, 5
FAKE = 256                                             # never dereferenced: validation fails first
NO_DEVICE = -1000 - 100                                # the C ABI's -1000 - hipError, hipErrorNoDevice
LIMITS = {CARTPOLE: 500, PENDULUM: 200, MOUNTAINCAR: 200, ACROBOT: 500}     # gymnasium's max_episode_steps
CASES = [("gymrl_classic_policy_eval", CARTPOLE), ("gymrl_classic_policy_eval", PENDULUM), ("gymrl_classic_duel_eval", CARTPOLE),
         ("gymrl_mountaincar_net_eval", MOUNTAINCAR), ("gymrl_acrobot_net_eval", ACROBOT)]


def _block(entry, kind, ptr=FAKE, out=(FAKE, FAKE, FAKE), **kw):
    """The smallest valid block of an entry point: a three-layer MLP (the dueling entry point: two hidden layers and two heads)."""
    from gymrl_amd import _lib, ops
    _, D, A, _, cap = ops.EPISODE_ENVS[kind]
    if entry == "gymrl_classic_policy_eval":
        a = _lib.ClassicEvalArgs()
        a.env_kind, a.head, a.D, a.A, a.bound = kind, ops.CLASSIC_EVAL_HEADS[kind], D, A, 2.0
        for k in range(3):
            a.w[k] = a.b[k] = ptr
    elif entry == "gymrl_classic_duel_eval":
        a = _lib.ClassicDuelEvalArgs()
        a.env_kind, a.n_hidden, a.D, a.A = kind, 2, D, A
        a.w[0] = a.b[0] = a.w[1] = a.b[1] = a.value_w = a.value_b = a.adv_w = a.adv_b = ptr
    else:
        a = (_lib.MountainCarNetEvalArgs if kind == MOUNTAINCAR else _lib.AcrobotNetEvalArgs)()
        a.net, a.n_hidden = 0, 2
        a.w[0] = a.b[0] = a.w[1] = a.b[1] = a.head_w = a.head_b = ptr
    a.P, a.E, a.H, a.cap = 1, 1, 4, cap
    a.policy_stride, a.images, a.seed, a.stream_id0, a.start, a.final_obs = 0, None, 42, 1 << 40, None, None
    a.returns, a.lengths, a.terminated = out
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def _call(entry, kind, **kw):
    from gymrl_amd import _lib
    return getattr(_lib.lib(), entry)(ctypes.byref(_block(entry, kind, **kw)), None)


def test_the_table_of_the_binding_is_the_librarys():
    from gymrl_amd import ops
    assert sorted(ops.EPISODE_ENVS) == sorted(LIMITS)
    for kind, (name, D, A, nst, cap) in ops.EPISODE_ENVS.items():
        assert ops.ENV_KINDS[name] == kind
        assert ops.env_dims(kind) == (D, A, kind != PENDULUM, cap) and cap == LIMITS[kind]
        assert nst == (4 if kind in (CARTPOLE, ACROBOT) else 2)
    assert ops.ACROBOT_MAX_STEPS == 500 and ops.MOUNTAINCAR_MAX_STEPS == 200
    assert ops.CLASSIC_PPO_EVAL_CAPS == {CARTPOLE: 500, MOUNTAINCAR: 200, ACROBOT: 500}
    assert ops.ROLLOUT_CLASSIC_DIMS == {CARTPOLE: (4, 2), MOUNTAINCAR: (2, 3), ACROBOT: (6, 3)}


@pytest.mark.parametrize("entry,kind", CASES)
def test_the_time_limit_is_the_largest_cap(entry, kind):
    from gymrl_amd import ops
    limit = LIMITS[kind]
    assert _call(entry, kind, cap=limit + 1) == -22 and _call(entry, kind, cap=2 * limit) == -22
    if not ops.device_ok():
        assert _call(entry, kind, cap=limit) == NO_DEVICE              # past every argument check, at the first HIP call
        return
    import torch
    zeros = torch.zeros(1024, device="cuda")                           # every layer of the policy: H * H = 16 floats at the most
    out = (torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.uint8, device="cuda"))
    rc = _call(entry, kind, cap=limit, ptr=zeros.data_ptr(), out=tuple(t.data_ptr() for t in out))
    torch.cuda.synchronize()
    assert rc == 0 and 1 <= int(out[1][0]) <= limit


@pytest.mark.parametrize("entry,kind", CASES)
def test_the_shared_rules_refuse_alike_before_any_launch(entry, kind):
    c = lambda **kw: _call(entry, kind, **kw)     # noqa: E731
    assert c(P=0) == -22 and c(P=-1) == -22
    assert c(E=0) == -22 and c(E=-1) == -22
    assert c(cap=0) == -22 and c(cap=-1) == -22
    assert c(stream_id0=-1) == -22
    assert c(policy_stride=6) == -22 and c(P=2, policy_stride=4098) == -22                        # % 4
    assert c(P=2) == -22                                                                           # stride 0 is ONE policy
    assert c(P=2, policy_stride=4096, images=FAKE) == -22                                          # an image is of ONE policy
    assert c(P=2, policy_stride=4096, images=FAKE, H=16) == -22                                    # ... at a width that has one, too
    for name in ("returns", "lengths", "terminated"):
        assert c(**{name: None}) == -22, f"NULL {name}"
    assert c(returns=FAKE + 2) == -22                                                              # off by 2 bytes
