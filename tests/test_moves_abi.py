"""Argument errors of the legal-move / afterstate entry points (r48_moves.hip) without a GPU:
NULL pointers and n < 0 come back as R48_EINVAL with a message before any HIP call."""
import ctypes as C

import pytest

from rein48_amd import _lib

P = C.c_void_p(0x1000)     # a non-NULL, 16-byte aligned stand-in: never dereferenced on these paths
ODD = C.c_void_p(0x1008)   # not 16-byte aligned

# name -> (good argument tuple, indices of the pointer arguments that must not be NULL, index of n)
CASES = {
    "r48_boards_legal": ((P, 4, P, None), (0, 2), 1),
    "r48_boards_afterstates": ((P, 4, P, None, None, None), (0, 2), 1),
    "r48_sample_actions_masked": ((P, P, 4, 1, 0, 0, P, None, None, None), (0, 1, 6), 2),
    "r48_egreedy_actions_masked": ((P, P, 4, 0.1, 1, 0, 0, P, None), (0, 1, 7), 2),
    "r48_td_target_masked": ((P, None, P, None, P, 4, 0.99, 0, P, None), (0, 2, 4, 8), 5),
}


def _einval(lib, name, args):
    assert getattr(lib, name)(*args) == _lib.R48_EINVAL, (name, args)
    msg = lib.r48_last_error()
    assert name.encode() in msg and len(msg) > len(name) + 10, msg


@pytest.mark.parametrize("name", sorted(CASES))
def test_null_and_negative_arguments(name):
    lib = _lib.load()
    good, required, n_at = CASES[name]
    for k in required:
        _einval(lib, name, good[:k] + (None,) + good[k + 1:])
    _einval(lib, name, good[:n_at] + (-1,) + good[n_at + 1:])
    with pytest.raises(_lib.Rein48Error):
        _lib.check(getattr(lib, name)(*(good[:n_at] + (-5,) + good[n_at + 1:])))


def test_misaligned_boards_and_negative_gid0():
    lib = _lib.load()
    _einval(lib, "r48_boards_legal", (ODD, 4, P, None))
    _einval(lib, "r48_boards_afterstates", (P, 4, ODD, None, None, None))
    _einval(lib, "r48_sample_actions_masked", (P, P, 4, 1, -1, 0, P, None, None, None))
    _einval(lib, "r48_egreedy_actions_masked", (ODD, P, 4, 0.1, 1, 0, 0, P, None))
    _einval(lib, "r48_td_target_masked", (P, None, P, ODD, P, 4, 0.99, 0, P, None))


@pytest.mark.parametrize("name", sorted(CASES))
def test_zero_boards_is_a_noop(name):
    """n == 0 returns R48_OK without touching a pointer or the GPU."""
    good, _, n_at = CASES[name]
    assert getattr(_lib.load(), name)(*(good[:n_at] + (0,) + good[n_at + 1:])) == _lib.R48_OK
