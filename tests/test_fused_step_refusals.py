"""What the nine entry points of the fused off-policy vector steps (gymrl_{sac,td3,dsac}_{act_step,update,pack_images}) refuse
with -22 before anything touches HIP: a missing required pointer, a shape one past its bound.  CPU only: every struct passed
here carries at least one reason for refusal — a fully valid one would launch on the dummy addresses below.

The three algorithms' checks differ in a few places on purpose; the tables name each difference (CASES: `neg_cursor`,
`idx_dev_rescues`, `max_batch`, `n_critics`), so a change of the shared validation that moves one of them fails here."""
import ctypes

import pytest

DUMMY = 0x1000                # a non-null host address: never dereferenced, the checks only compare against NULL
RING = ("r_state", "r_action", "r_reward", "r_next", "r_flag")
PENDULUM_DA, CARTPOLE_DA = (3, 1), (4, 2)


def _net(n):
    return tuple((kind, k) for k in range(n) for kind in ("w", "b"))


# entry point -> what a legal argument struct of it looks like and where its check differs from its siblings'
#   nets: member -> the (w | b, k) slots the check requires            scalars: plain required pointers
#   neg_cursor: the act step refuses cursor < 0 (SAC's does not: its check stops at cap >= N)
#   idx_dev_rescues: a device-side draw record stands in for idx / idx_size (SAC's update takes no idx_dev in that condition)
CASES = {
    "sac_act_step": dict(struct="SacActArgs", env="PENDULUM", da=PENDULUM_DA, nets={"actor": _net(4)},
                         scalars=("env_state", "obs", "obs_out") + RING, neg_cursor=False),
    "td3_act_step": dict(struct="Td3ActArgs", env="PENDULUM", da=PENDULUM_DA, nets={"actor": _net(3)},
                         scalars=("env_state", "obs", "obs_out") + RING, neg_cursor=True),
    "dsac_act_step": dict(struct="DsacActArgs", env="CARTPOLE", da=CARTPOLE_DA, nets={"actor": _net(3)},
                          scalars=("env_state", "obs", "obs_out") + RING, neg_cursor=True),
    "sac_update": dict(struct="SacUpdateArgs", max_batch=8192, idx_dev_rescues=False,
                       nets={"actor": _net(4), "critic": _net(6), "target": _net(6)},
                       scalars=RING + ("workspace", "sums", "log_alpha", "alpha_m", "alpha_v", "actor_p", "actor_m", "actor_v",
                                       "critic_p", "critic_m", "critic_v")),
    "td3_update": dict(struct="Td3UpdateArgs", max_batch=256, idx_dev_rescues=True, n_critics=2,
                       nets={"actor": _net(3), "actor_target": _net(3), "critic": _net(6), "critic_target": _net(6)},
                       scalars=RING + ("workspace", "sums", "actor_p", "actor_m", "actor_v", "critic_p", "critic_m", "critic_v")),
    "dsac_update": dict(struct="DsacUpdateArgs", max_batch=256, idx_dev_rescues=True,
                        nets={n: _net(3) for n in ("actor", "critic1", "critic2", "critic1_target", "critic2_target")},
                        scalars=RING + ("workspace", "sums", "log_alpha", "alpha_m", "alpha_v", "actor_p", "actor_m", "actor_v",
                                        "critic1_p", "critic1_m", "critic1_v", "critic2_p", "critic2_m", "critic2_v")),
    # the pack calls read the H x H layers only: w[1] of every network (w[4]: the twin module's second fc2)
    "sac_pack_images": dict(struct="SacUpdateArgs", scalars=("images",),
                            nets={"actor": (("w", 1),), "critic": (("w", 1), ("w", 4)), "target": (("w", 1), ("w", 4))}),
    "td3_pack_images": dict(struct="Td3UpdateArgs", scalars=("images",), n_critics=2,
                            nets={"actor": (("w", 1),), "actor_target": (("w", 1),), "critic": (("w", 1), ("w", 4)),
                                  "critic_target": (("w", 1), ("w", 4))}),
    "dsac_pack_images": dict(struct="DsacUpdateArgs", scalars=("images",),
                             nets={n: (("w", 1),) for n in ("actor", "critic1", "critic2", "critic1_target", "critic2_target")}),
}
ACT, UPDATE, PACK = ([n for n in CASES if n.endswith(s)] for s in ("act_step", "update", "pack_images"))


def _legal(name):
    """A struct of entry point `name` that its check would accept: NEVER passed as it is."""
    from gymrl_amd import _lib, ops
    case = CASES[name]
    a = getattr(_lib, case["struct"])()
    for f in case["scalars"]:
        setattr(a, f, DUMMY)
    for member, slots in case["nets"].items():
        for kind, k in slots:
            getattr(getattr(a, member), kind)[k] = DUMMY
    a.H = 64
    if name in ACT:
        a.N, (a.D, a.A), a.cap, a.cursor, a.env_kind = 20, case["da"], 20, 0, getattr(ops, case["env"])
    elif name in UPDATE:
        a.B, a.D, a.A, a.idx, a.idx_size = 24, 3, 1, DUMMY, 0
    if "n_critics" in case:
        a.n_critics = case["n_critics"]
    if name == "dsac_update":
        a.alpha_t = 1
    return a


def _refused(name, **fields):
    """-22 from entry point `name` for a legal struct with `fields` overwritten (at least one: see the module docstring)."""
    from gymrl_amd import _lib
    assert fields, "a fully valid struct would launch"
    a = _legal(name)
    for f, v in fields.items():
        setattr(a, f, v)
    return getattr(_lib.lib(), "gymrl_" + name)(ctypes.byref(a), ctypes.c_void_p(None)) == -22


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_required_pointer_is_required(name):
    from gymrl_amd import _lib
    case = CASES[name]
    call = getattr(_lib.lib(), "gymrl_" + name)
    assert call(None, ctypes.c_void_p(None)) == -22
    for f in case["scalars"]:
        assert _refused(name, **{f: None}), f
    for member, slots in case["nets"].items():
        for kind, k in slots:
            a = _legal(name)
            getattr(getattr(a, member), kind)[k] = None
            assert call(ctypes.byref(a), ctypes.c_void_p(None)) == -22, (member, kind, k)


@pytest.mark.parametrize("name", ACT)
def test_act_step_limits(name):
    case = CASES[name]
    D, A = case["da"]
    for fields in (dict(N=0), dict(D=D + 1), dict(D=0), dict(A=A + 1), dict(A=0), dict(H=0), dict(H=260), dict(H=62), dict(cap=19),
                   dict(env_kind=2), dict(D=9), dict(A=5)):
        assert _refused(name, **fields), fields
    if case["neg_cursor"]:
        assert _refused(name, cursor=-1)


@pytest.mark.parametrize("name", UPDATE)
def test_update_limits(name):
    case = CASES[name]
    for fields in (dict(B=0), dict(B=case["max_batch"] + 1), dict(D=0), dict(D=9), dict(A=0), dict(A=5), dict(H=0), dict(H=260),
                   dict(H=62), dict(idx=None, idx_size=23)):
        assert _refused(name, **fields), fields
    if not case["idx_dev_rescues"]:
        assert _refused(name, idx=None, idx_dev=DUMMY, idx_size=0)
    if "n_critics" in case:
        assert _refused(name, n_critics=0) and _refused(name, n_critics=3)
    if name == "dsac_update":                    # the temperature's bias corrections: a step count or a device record
        assert _refused(name, alpha_t=0) and _refused(name, alpha_t=-1)


@pytest.mark.parametrize("name", PACK)
def test_pack_images_limits(name):
    for fields in (dict(H=0), dict(H=-16), dict(H=24), dict(H=272)):
        assert _refused(name, **fields), fields
    if "n_critics" in CASES[name]:
        assert _refused(name, n_critics=0) and _refused(name, n_critics=3)
