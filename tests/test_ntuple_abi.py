"""Argument errors of the n-tuple entry points (r48_ntuple.hip) without a GPU: NULL or misaligned
pointers, n < 0 and bad layouts come back as R48_EINVAL with a message before any HIP call, and
n == 0 is a no-op."""
import ctypes as C

import pytest

from rein48_amd import _lib

P = C.c_void_p(0x1000)     # a non-NULL, 16-byte aligned stand-in: never dereferenced on these paths
ODD = C.c_void_p(0x1008)   # not 16-byte aligned


def cells(*tuples):
    flat = [c for t in tuples for c in t]
    return (C.c_uint8 * len(flat))(*flat)


GOOD = cells((0, 1, 2, 3), (4, 5, 6, 7))      # m = 2, L = 4

# name -> (good argument tuple, indices of the pointer arguments that must not be NULL, index of n,
#          index of cells -- m and L follow it)
CASES = {
    "r48_ntuple_value": ((P, 4, GOOD, 2, 4, P, P, None), (0, 2, 5, 6), 1, 2),
    "r48_ntuple_act": ((P, 4, GOOD, 2, 4, P, P, None, None, None, None, None), (0, 2, 5, 6), 1, 2),
    "r48_ntuple_accumulate": ((P, 4, P, None, GOOD, 2, 4, P, P, None), (0, 2, 4, 7, 8), 1, 4),
    "r48_ntuple_apply": ((P, 4, None, GOOD, 2, 4, 0.1, P, P, P, None), (0, 3, 7, 8, 9), 1, 3),
}


def _einval(lib, name, args):
    assert getattr(lib, name)(*args) == _lib.R48_EINVAL, (name, args)
    msg = lib.r48_last_error()
    assert name.encode() in msg and len(msg) > len(name) + 10, msg


def _with(args, k, v):
    return args[:k] + (v,) + args[k + 1:]


@pytest.mark.parametrize("name", sorted(CASES))
def test_null_and_negative_arguments(name):
    lib = _lib.load()
    good, required, n_at, _ = CASES[name]
    for k in required:
        _einval(lib, name, _with(good, k, None))
    _einval(lib, name, _with(good, n_at, -1))
    _einval(lib, name, _with(good, 0, ODD))                     # boards not 16-byte aligned
    with pytest.raises(_lib.Rein48Error):
        _lib.check(getattr(lib, name)(*_with(good, n_at, -5)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_bad_layouts(name):
    """m outside 1..8, L outside 2..6, a cell >= 16, a cell repeated within a tuple -- also with
    n == 0: the layout is checked before the no-op return."""
    lib = _lib.load()
    good, _, n_at, c_at = CASES[name]
    for n in (4, 0):
        base = _with(good, n_at, n)
        for m, L in ((0, 4), (9, 4), (-1, 4), (2, 1), (2, 7), (2, 0)):
            _einval(lib, name, _with(_with(base, c_at + 1, m), c_at + 2, L))
        _einval(lib, name, _with(base, c_at, cells((0, 1, 2, 16), (4, 5, 6, 7))))
        _einval(lib, name, _with(base, c_at, cells((0, 1, 2, 255), (4, 5, 6, 7))))
        _einval(lib, name, _with(base, c_at, cells((0, 1, 2, 3), (4, 5, 6, 4))))
    # a cell may repeat across tuples, and the limits themselves are fine
    assert getattr(lib, name)(*_with(_with(good, n_at, 0), c_at, cells((0, 1, 2, 3), (3, 2, 1, 0)))) == _lib.R48_OK
    eight = cells(*[(k, k + 1) for k in range(8)])
    assert getattr(lib, name)(*_with(_with(_with(_with(good, n_at, 0), c_at, eight), c_at + 1, 8), c_at + 2, 2)) == _lib.R48_OK
    six = cells((0, 1, 2, 3, 4, 5))
    assert getattr(lib, name)(*_with(_with(_with(_with(good, n_at, 0), c_at, six), c_at + 1, 1), c_at + 2, 6)) == _lib.R48_OK


def test_misaligned_outputs():
    lib = _lib.load()
    _einval(lib, "r48_ntuple_act", (P, 4, GOOD, 2, 4, P, P, ODD, None, None, None, None))         # after
    _einval(lib, "r48_ntuple_accumulate", (P, 4, P, None, GOOD, 2, 4, C.c_void_p(0x1004), P, None))  # acc: 8 bytes
    _einval(lib, "r48_ntuple_apply", (P, 4, None, GOOD, 2, 4, 0.1, P, C.c_void_p(0x1004), P, None))


@pytest.mark.parametrize("name", sorted(CASES))
def test_zero_boards_is_a_noop(name):
    """n == 0 returns R48_OK without touching a pointer or the GPU."""
    good, _, n_at, _ = CASES[name]
    assert getattr(_lib.load(), name)(*_with(good, n_at, 0)) == _lib.R48_OK
