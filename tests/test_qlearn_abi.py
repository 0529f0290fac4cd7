"""CPU-side checks of the tabular Q-learning boundary: include/gymrl.h declares the entry points, the library exports them,
the ctypes binding says what the header says, and every pointer or size error is refused with -22 before anything is
launched (no GPU here)."""
import ctypes

import pytest

from test_abi import _agrees, _mirrors, _parse_header

ENTRY_POINTS = ("gymrl_qlearn_state_bytes", "gymrl_qlearn_train", "gymrl_qlearn_eval")
FROZENLAKE, CLIFFWALKING = 0, 1


def test_header_declares_and_library_exports_the_entry_points():
    from gymrl_amd import _lib
    functions, _ = _parse_header()
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in functions, f"{name} is not declared in include/gymrl.h"
        assert hasattr(L, name), f"{name} is not exported"
    order = list(functions)
    assert order.index("gymrl_softmax_rows_bwd") < order.index("gymrl_qlearn_state_bytes")          # additions only, at the end
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION


def test_signatures_match_the_header():
    from gymrl_amd import _lib
    functions, _ = _parse_header()
    mirrors = _mirrors()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        ret, params = functions[name]
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters in the header, {len(argtypes)} in the table"
        for i, (ct, htype) in enumerate(zip(argtypes, params)):
            assert _agrees(ct, htype, mirrors), f"{name}: parameter {i}"
    assert _lib.SIGNATURES["gymrl_qlearn_state_bytes"][0] is ctypes.c_size_t
    assert _lib.SIGNATURES["gymrl_qlearn_train"][0] is ctypes.c_int and _lib.SIGNATURES["gymrl_qlearn_eval"][0] is ctypes.c_int
    assert [n for n in _lib.SIGNATURES if n.startswith("gymrl_qlearn_")] == [n for n in functions if n.startswith("gymrl_qlearn_")]


def test_state_bytes():
    from gymrl_amd import _lib
    L = _lib.lib()
    assert L.gymrl_qlearn_state_bytes(0) == 0 and L.gymrl_qlearn_state_bytes(-3) == 0
    # five SoA fields (one f64, four i32), each padded to 256 bytes
    assert L.gymrl_qlearn_state_bytes(1) == 5 * 256
    assert L.gymrl_qlearn_state_bytes(65) == 768 + 4 * 512
    assert L.gymrl_qlearn_state_bytes(65536) == 65536 * (8 + 4 * 4)


# argument positions of the pointers each entry point requires
TRAIN_POINTERS = {"Q": 3, "state": 4, "eps_table": 9, "episode_rewards": 15, "episode_lengths": 16, "k_out": 17, "episodes_out": 18}
EVAL_POINTERS = {"Q": 2, "returns": 8, "lengths": 9, "flags": 10}


def _train_args(kind=FROZENLAKE, R=3):
    fake = 256                                         # never dereferenced: validation fails first
    return [kind, 1, 1, fake, fake, R, 1, 42, 0, fake, 30, 100, 3000, 0.1, 0.9, fake, fake, fake, fake, None]


def _eval_args(kind=CLIFFWALKING, R=3):
    fake = 256
    return [kind, 0, fake, R, 5, 42, 1 << 40, 200, fake, fake, fake, None]


def test_train_refuses_bad_arguments_before_any_launch():
    from gymrl_amd import _lib
    L = _lib.lib()
    for name, pos in TRAIN_POINTERS.items():
        args = _train_args()
        args[pos] = None
        assert L.gymrl_qlearn_train(*args) == -22, f"NULL {name}"
    assert L.gymrl_qlearn_train(*_train_args(R=0)) == -22 and L.gymrl_qlearn_train(*_train_args(R=-1)) == -22
    assert L.gymrl_qlearn_train(*_train_args(kind=2)) == -22 and L.gymrl_qlearn_train(*_train_args(kind=-1)) == -22
    for name, pos, bad in (("Q", 3, 260), ("state", 4, 264), ("eps_table", 9, 260), ("episode_rewards", 15, 260),
                           ("episode_lengths", 16, 258), ("k_out", 17, 257), ("episodes_out", 18, 258)):
        args = _train_args()
        args[pos] = bad
        assert L.gymrl_qlearn_train(*args) == -22, f"misaligned {name}"
    args = _train_args()
    args[10], args[11] = 1 << 16, 1 << 15                                    # max_episodes * max_steps = 2^31
    assert L.gymrl_qlearn_train(*args) == -22
    for pos in (10, 11):                                                      # an empty episode budget
        args = _train_args()
        args[pos] = 0
        assert L.gymrl_qlearn_train(*args) == -22
    args = _train_args()
    args[12] = -1                                                             # max_iters
    assert L.gymrl_qlearn_train(*args) == -22
    args = _train_args()
    args[12], args[6] = 0, 0                                                  # nothing to do: no launch, no error
    assert L.gymrl_qlearn_train(*args) == 0
    args = _train_args()
    args[5] = 3.0                                                             # a float for the run count
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_qlearn_train(*args)


def test_eval_refuses_bad_arguments_before_any_launch():
    from gymrl_amd import _lib
    L = _lib.lib()
    for name, pos in EVAL_POINTERS.items():
        args = _eval_args()
        args[pos] = None
        assert L.gymrl_qlearn_eval(*args) == -22, f"NULL {name}"
    assert L.gymrl_qlearn_eval(*_eval_args(R=0)) == -22
    assert L.gymrl_qlearn_eval(*_eval_args(kind=7)) == -22
    for name, pos, bad in (("Q", 2, 260), ("returns", 8, 260), ("lengths", 9, 258)):
        args = _eval_args()
        args[pos] = bad
        assert L.gymrl_qlearn_eval(*args) == -22, f"misaligned {name}"
    for pos in (4, 7):                                                        # no episodes / no steps
        args = _eval_args()
        args[pos] = 0
        assert L.gymrl_qlearn_eval(*args) == -22


def test_ops_wrappers_refuse_cpu_tensors():
    import torch
    from gymrl_amd import ops
    R, E, T = 2, 3, 4
    Q = torch.zeros(R, 16, 4, dtype=torch.float64)
    state = torch.zeros(ops.qlearn_state_bytes(R), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.qlearn_train(ops.FROZENLAKE, Q, state, torch.zeros(E * T, dtype=torch.float64), 42, 0, E, T, 5, 0.1, 0.9,
                         torch.zeros(R, E, dtype=torch.float64), torch.zeros(R, E, dtype=torch.int32),
                         torch.zeros(R, dtype=torch.int32), torch.zeros(R, dtype=torch.int32), restart=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.qlearn_eval(ops.FROZENLAKE, Q, 5, 42, 1 << 40, 100)
    with pytest.raises(ValueError):
        ops.qlearn_eval(ops.CLIFFWALKING, Q, 5, 42, 1 << 40, 100)            # a FrozenLake-shaped table for CliffWalking
