"""CPU-side checks of gymrl_tabular_train's boundary (SARSA, Expected SARSA, Double Q-learning): declared, exported and mirrored,
the argument struct the size the library reports, every refusal of include/gymrl.h returned as -22 before anything is launched
(fake pointers, no GPU here), and the Q-learning entry points' own refusals where they were."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

FAKE = 256                                             # never dereferenced: validation fails first
ENTRY_POINTS = ["gymrl_tabular_state_bytes", "gymrl_tabular_args_bytes", "gymrl_tabular_train"]
FIELDS = ["rule", "env_kind", "is_slippery", "shaped", "Q", "state", "n_runs", "restart", "seed", "run_id0", "eps_table", "max_episodes",
          "max_steps", "max_iters", "lr", "gamma", "episode_rewards", "episode_lengths", "k_out", "episodes_out", "Q2", "eps_len"]
QLEARNING, SARSA, EXPECTED_SARSA, DOUBLE_Q = 0, 1, 2, 3
POINTERS = ("Q", "state", "eps_table", "episode_rewards", "episode_lengths", "k_out", "episodes_out")


def test_header_declares_library_exports_and_binding_mirrors():
    from gymrl_amd import _lib, ops
    functions, structs = _parse_header()
    mirrors = _mirrors()
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in functions and hasattr(L, name) and name in _lib.SIGNATURES
        _, params = functions[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(params)
        for ct, htype in zip(argtypes, params):
            assert _agrees(ct, htype, mirrors)
    assert _lib.SIGNATURES["gymrl_tabular_state_bytes"] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
    assert _lib.SIGNATURES["gymrl_tabular_args_bytes"] == (ctypes.c_size_t, [])
    assert _lib.SIGNATURES["gymrl_tabular_train"] == (ctypes.c_int, [ctypes.POINTER(_lib.TabularTrainArgs), ctypes.c_void_p])
    cls = _lib.TabularTrainArgs
    assert cls._c_name_ == "gymrl_tabular_train_args" and mirrors["gymrl_tabular_train_args"] is cls
    assert [f for f, _ in structs["gymrl_tabular_train_args"]] == [f for f, _ in cls._fields_] == FIELDS
    assert L.gymrl_tabular_args_bytes() == ctypes.sizeof(cls)
    # rule in front, then gymrl_qlearn_train's arguments in its order, then the two additions
    assert len(FIELDS) == 1 + (len(_lib.SIGNATURES["gymrl_qlearn_train"][1]) - 1) + 2
    # one section behind the Q-learning entry points, the table in the header's order; an addition: same version, same end
    names, table = list(functions), list(_lib.SIGNATURES)
    for order in (names, table):
        at = order.index("gymrl_qlearn_eval")
        assert order[at + 1:at + 4] == ENTRY_POINTS
    assert names[-1] == "gymrl_mountaincar_rule_eval"
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION
    assert ops.TABULAR_RULES == {"qlearning": QLEARNING, "sarsa": SARSA, "expected_sarsa": EXPECTED_SARSA, "double_q": DOUBLE_Q}


def test_state_bytes():
    from gymrl_amd import _lib
    L = _lib.lib()
    for rule in (QLEARNING, SARSA, EXPECTED_SARSA, DOUBLE_Q):
        assert L.gymrl_tabular_state_bytes(rule, 0) == 0 and L.gymrl_tabular_state_bytes(rule, -3) == 0
        # gymrl_qlearn_train's record and one more i32 field (the pending action), padded to 256 bytes like the others
        assert L.gymrl_tabular_state_bytes(rule, 1) == L.gymrl_qlearn_state_bytes(1) + 256 == 6 * 256
        assert L.gymrl_tabular_state_bytes(rule, 65) == L.gymrl_qlearn_state_bytes(65) + 512
        assert L.gymrl_tabular_state_bytes(rule, 65536) == 65536 * (8 + 5 * 4)
    assert L.gymrl_tabular_state_bytes(4, 8) == 0 and L.gymrl_tabular_state_bytes(-1, 8) == 0


def _args(rule=SARSA, **kw):
    from gymrl_amd import _lib
    a = _lib.TabularTrainArgs()
    a.rule, a.env_kind, a.is_slippery, a.shaped, a.n_runs, a.restart, a.seed, a.run_id0 = rule, 0, 1, 1, 3, 1, 42, 0
    a.max_episodes, a.max_steps, a.max_iters, a.lr, a.gamma = 30, 100, 3030, 0.1, 0.9
    for name in POINTERS:
        setattr(a, name, FAKE)
    a.Q2 = FAKE if rule == DOUBLE_Q else None
    a.eps_len = 30 * (101 if rule == SARSA else 100)
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def _train(rule=SARSA, **kw):
    from gymrl_amd import _lib
    return _lib.lib().gymrl_tabular_train(ctypes.byref(_args(rule, **kw)), None)


ALL_RULES = (QLEARNING, SARSA, EXPECTED_SARSA, DOUBLE_Q)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_train_refuses_bad_arguments_before_any_launch(rule):
    from gymrl_amd import _lib
    assert _lib.lib().gymrl_tabular_train(None, None) == -22
    for name in POINTERS:
        assert _train(rule, **{name: None}) == -22, f"NULL {name}"
    for name, bad in (("Q", 260), ("state", 264), ("eps_table", 260), ("episode_rewards", 260), ("episode_lengths", 258), ("k_out", 257),
                      ("episodes_out", 258)):
        assert _train(rule, **{name: bad}) == -22, f"misaligned {name}"
    assert _train(rule, n_runs=0) == -22 and _train(rule, n_runs=-1) == -22
    assert _train(rule, env_kind=2) == -22 and _train(rule, env_kind=-1) == -22
    assert _train(rule, max_episodes=0) == -22 and _train(rule, max_steps=0) == -22 and _train(rule, max_iters=-1) == -22
    assert _train(rule, run_id0=-1) == -22
    # nothing to do: no launch, no error — and only for arguments that would have been accepted
    assert _train(rule, max_iters=0, restart=0) == 0
    assert _train(rule, max_iters=0, restart=0, Q=None) == -22


def test_unknown_rule():
    from gymrl_amd import _lib
    for rule in (-1, 4, 99):
        a = _args(SARSA)
        a.rule = rule
        assert _lib.lib().gymrl_tabular_train(ctypes.byref(a), None) == -22


def test_second_table_against_the_rule():
    for rule in (QLEARNING, SARSA, EXPECTED_SARSA):
        assert _train(rule, Q2=FAKE) == -22, f"rule {rule} with a second table"
    assert _train(DOUBLE_Q, Q2=None) == -22
    assert _train(DOUBLE_Q, Q2=260) == -22                                     # misaligned
    assert _train(DOUBLE_Q, max_iters=0, restart=0) == 0


def test_epsilon_table_length():
    """max_episodes * max_steps entries; SARSA: max_episodes * (max_steps + 1)."""
    for rule in (QLEARNING, EXPECTED_SARSA, DOUBLE_Q):
        assert _train(rule, eps_len=2999, max_iters=0, restart=0) == -22
        assert _train(rule, eps_len=3000, max_iters=0, restart=0) == 0
        assert _train(rule, eps_len=0) == -22 and _train(rule, eps_len=-5) == -22
    assert _train(SARSA, eps_len=3000) == -22 and _train(SARSA, eps_len=3029) == -22
    assert _train(SARSA, eps_len=3030, max_iters=0, restart=0) == 0 and _train(SARSA, eps_len=4000, max_iters=0, restart=0) == 0


def test_int32_range_of_the_draw_count():
    big = 1 << 40
    # 2^16 * 2^15 = 2^31: refused under every rule, as gymrl_qlearn_train refuses it
    for rule in ALL_RULES:
        assert _train(rule, max_episodes=1 << 16, max_steps=1 << 15, eps_len=big) == -22
    # 2^16 * (2^15 - 1) fits; SARSA's 2^16 * 2^15 draws do not
    fits = dict(max_episodes=1 << 16, max_steps=(1 << 15) - 1, eps_len=big, max_iters=0, restart=0)
    for rule in (QLEARNING, EXPECTED_SARSA, DOUBLE_Q):
        assert _train(rule, **fits) == 0
    assert _train(SARSA, **fits) == -22
    assert _train(SARSA, **dict(fits, max_steps=(1 << 15) - 2)) == 0


def test_qlearn_entry_points_refuse_what_they_refused():
    from gymrl_amd import _lib
    L = _lib.lib()
    train = [0, 1, 1, FAKE, FAKE, 3, 1, 42, 0, FAKE, 30, 100, 3000, 0.1, 0.9, FAKE, FAKE, FAKE, FAKE, None]
    for pos in (3, 4, 9, 15, 16, 17, 18):
        args = list(train)
        args[pos] = None
        assert L.gymrl_qlearn_train(*args) == -22
    args = list(train)
    args[10], args[11] = 1 << 16, 1 << 15
    assert L.gymrl_qlearn_train(*args) == -22
    args = list(train)
    args[12], args[6] = 0, 0
    assert L.gymrl_qlearn_train(*args) == 0
    assert L.gymrl_qlearn_eval(7, 0, FAKE, 3, 5, 42, 1 << 40, 200, FAKE, FAKE, FAKE, None) == -22
    assert L.gymrl_qlearn_eval(1, 0, None, 3, 5, 42, 1 << 40, 200, FAKE, FAKE, FAKE, None) == -22
    assert L.gymrl_qlearn_state_bytes(1) == 5 * 256 and L.gymrl_qlearn_state_bytes(0) == 0


def test_ops_wrapper_refusals():
    import torch
    from gymrl_amd import ops
    R, E, T = 2, 3, 4
    Q = torch.zeros(R, 16, 4, dtype=torch.float64)

    def call(rule, eps_len, Q2=None, Q=Q):
        state = torch.zeros(ops.tabular_state_bytes(rule, R), dtype=torch.uint8)
        ops.tabular_train(rule, ops.FROZENLAKE, Q, state, torch.zeros(eps_len, dtype=torch.float64), 42, 0, E, T, 5, 0.1, 0.9,
                          torch.zeros(R, E, dtype=torch.float64), torch.zeros(R, E, dtype=torch.int32), torch.zeros(R, dtype=torch.int32),
                          torch.zeros(R, dtype=torch.int32), Q2=Q2, restart=True)

    assert ops.tabular_draws(SARSA, E, T) == E * (T + 1) and ops.tabular_draws(DOUBLE_Q, E, T) == E * T
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(SARSA, E * (T + 1))
    with pytest.raises(ValueError):
        call(SARSA, E * T)                                  # Q-learning's table length
    with pytest.raises(ValueError):
        call(DOUBLE_Q, E * T)                               # no second table
    with pytest.raises(ValueError):
        call(EXPECTED_SARSA, E * T, Q2=Q.clone())
    with pytest.raises(ValueError):
        call(7, E * T)
    with pytest.raises(ValueError):
        call(DOUBLE_Q, E * T, Q2=torch.zeros(R, 48, 4, dtype=torch.float64))


def test_trainer_refuses_an_unknown_rule():
    from gymrl_amd import sarsa_cliffwalking, sarsa_frozenlake
    for mod in (sarsa_cliffwalking, sarsa_frozenlake):
        cfg = mod.Config()
        assert cfg.rule == "sarsa"
        cfg.rule = "watkins"
        with pytest.raises(ValueError, match="rule"):
            mod.TDTrainer(cfg)
    # the siblings' defaults, plus the rule
    from gymrl_amd import qlearning_cliffwalking, qlearning_frozenlake
    for mod, sib in ((sarsa_cliffwalking, qlearning_cliffwalking), (sarsa_frozenlake, qlearning_frozenlake)):
        assert dict(vars(sib.Config()), rule="sarsa") == vars(mod.Config())
