"""CPU-side checks of the acting entry point gymrl_mlprnn_act and the masked normalisation entries: declared and loaded,
the parameter descriptor mirrors include/gymrl.h, and every bad argument is -EINVAL (-22) before any HIP call (no GPU
here)."""
import ctypes


def _params(fake=256, **override):
    from gymrl_amd import _lib
    P = _lib.MlprnnParams()
    for i in range(4):
        P.pscn_w[i], P.pscn_b[i], P.pscn_a[i] = fake, fake, fake
    for name, _ in _lib.MlprnnParams._fields_[3:]:
        setattr(P, name, fake)
    for k, v in override.items():
        if k.startswith("pscn_w"):
            P.pscn_w[int(k[-1])] = v
        else:
            setattr(P, k, v)
    return P


def test_symbols_and_descriptor():
    from gymrl_amd import _lib
    L = _lib.lib()
    for name in ("gymrl_mlprnn_params_bytes", "gymrl_mlprnn_act", "gymrl_running_norm_masked", "gymrl_reward_scaling_masked"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.gymrl_mlprnn_params_bytes() == ctypes.sizeof(_lib.MlprnnParams) == 28 * 8
    assert L.gymrl_abi_version() == 4


def test_mlprnn_act_validates_arguments_without_gpu():
    from gymrl_amd import _lib
    L = _lib.lib()
    null, fake = None, 256           # `fake` is 16-byte aligned and never dereferenced: validation fails first

    def act(P=None, N=4, D=8, A=4, x=fake, h=fake, h_out=fake, a=fake, lp=fake, v=fake):
        P = _params() if P is None else P
        return L.gymrl_mlprnn_act(x, h, ctypes.byref(P), N, D, A, null, null, 0, 0, 0, 0, h_out, a, lp, v, null, null)

    for A in (0, 1, 9, 16):
        assert act(A=A) == -22, A
    for D in (0, -1, 17):
        assert act(D=D) == -22, D
    assert act(N=-1) == -22 and act(N=(1 << 24) + 1) == -22
    for kw in ("x", "h", "h_out", "a", "lp", "v"):
        assert act(**{kw: null}) == -22, kw
    assert L.gymrl_mlprnn_act(fake, fake, None, 4, 8, 4, null, null, 0, 0, 0, 0, fake, fake, fake, fake, null, null) == -22
    for name, _ in _lib.MlprnnParams._fields_[3:]:
        assert act(P=_params(**{name: None})) == -22, name                   # NULL parameter
    for i in range(4):
        P = _params()
        P.pscn_b[i] = None
        assert act(P=P) == -22
    for name in ("pscn_w1", "pscn_w2", "pscn_w3", "lin_w", "w_ih", "w_hh", "actor_w1", "critic_w1"):
        assert act(P=_params(**{name: 260})) == -22, name                    # float4-read weight not 16-byte aligned
    assert act(N=0) == 0                                                     # nothing to launch


def test_masked_normalisation_validates_arguments_without_gpu():
    from gymrl_amd import _lib
    L = _lib.lib()
    null, fake = None, 256
    assert L.gymrl_running_norm_masked(null, fake, 4, 8, fake, 1, fake, null) == -22
    assert L.gymrl_running_norm_masked(fake, fake, 4, 0, fake, 1, fake, null) == -22
    assert L.gymrl_running_norm_masked(fake, fake, -1, 8, fake, 1, fake, null) == -22
    assert L.gymrl_running_norm_masked(fake, fake, 0, 8, fake, 1, fake, null) == 0
    assert L.gymrl_reward_scaling_masked(fake, null, fake, 4, 0.99, null, fake, fake, null) == -22
    assert L.gymrl_reward_scaling_masked(fake, null, fake, -2, 0.99, fake, fake, fake, null) == -22
    assert L.gymrl_reward_scaling_masked(fake, null, fake, 0, 0.99, fake, fake, fake, null) == 0


def test_networks_have_the_reference_state_dict_keys():
    """ActorCriticPPG(8, 4) / ActorCritic(8, 4) on the CPU: exactly the reference modules' state_dict keys and shapes
    (tests/golden/ppg_rnn_state_dict_keys.json, recorded from the reference's classes)."""
    import json
    import os
    from conftest import ROOT
    from gymrl_amd.ppg_rnn_lunarlander import ActorCriticPPG
    from gymrl_amd.ppo_rnn_lunarlander import ActorCritic
    with open(os.path.join(ROOT, "tests", "golden", "ppg_rnn_state_dict_keys.json")) as f:
        want = json.load(f)
    for key, cls in (("ppg", ActorCriticPPG), ("ppo", ActorCritic)):
        got = [[k, list(v.shape)] for k, v in cls(8, 4).state_dict().items()]
        assert got == want[key], key
