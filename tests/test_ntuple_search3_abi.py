"""Argument errors of r48_ntuple_search3 (r48_ntuple.hip) without a GPU: NULL tables or actions, a
misaligned q or tables, a bad layout, n < 0 and an n beyond the grid come back as R48_EINVAL with a
message naming the function before any HIP call; n == 0 is a no-op; q and legal may be NULL."""
import ctypes as C

import pytest

from rein48_amd import _lib

P = C.c_void_p(0x1000)     # a non-NULL, 16-byte aligned stand-in: never dereferenced on these paths
ODD = C.c_void_p(0x1008)   # not 16-byte aligned
ODD4 = C.c_void_p(0x1002)  # not 4-byte aligned
NAME = "r48_ntuple_search3"


def cells(*tuples):
    flat = [c for t in tuples for c in t]
    return (C.c_uint8 * len(flat))(*flat)


GOOD_CELLS = cells((0, 1, 2, 3), (4, 5, 6, 7))      # m = 2, L = 4
# boards, n, cells, m, L, tables, actions, q, legal, stream
GOOD = (P, 4, GOOD_CELLS, 2, 4, P, P, P, P, None)
BOARDS, N, CELLS, M, LEN, TABLES, ACTIONS, Q, LEGAL = range(9)


def _with(args, k, v):
    return args[:k] + (v,) + args[k + 1:]


def _einval(args):
    lib = _lib.load()
    assert lib.r48_ntuple_search3(*args) == _lib.R48_EINVAL, args
    msg = lib.r48_last_error()
    assert NAME.encode() in msg and len(msg) > len(NAME) + 10, msg
    return msg


def test_the_binding_mirrors_the_header():
    assert len(_lib.SIGNATURES[NAME][1]) == len(GOOD)


def test_null_misaligned_and_negative_arguments():
    for k in (BOARDS, CELLS, TABLES, ACTIONS):
        _einval(_with(GOOD, k, None))
        _einval(_with(_with(GOOD, k, None), N, 0))              # checked before the no-op return
    _einval(_with(GOOD, N, -1))
    _einval(_with(GOOD, BOARDS, ODD))                           # boards not 16-byte aligned
    _einval(_with(GOOD, Q, ODD4))                               # q not 4-byte aligned
    _einval(_with(GOOD, TABLES, ODD4))
    _einval(_with(_with(GOOD, Q, ODD4), N, 0))
    with pytest.raises(_lib.Rein48Error):
        _lib.check(_lib.load().r48_ntuple_search3(*_with(GOOD, N, -5)))


def test_bad_layouts():
    for n in (4, 0):
        base = _with(GOOD, N, n)
        for m, L in ((0, 4), (9, 4), (-1, 4), (2, 1), (2, 7), (2, 0)):
            _einval(_with(_with(base, M, m), LEN, L))
        _einval(_with(base, CELLS, cells((0, 1, 2, 16), (4, 5, 6, 7))))
        _einval(_with(base, CELLS, cells((0, 1, 2, 3), (4, 5, 6, 4))))


def test_board_count_beyond_the_grid():
    """One board per workgroup, at most 2^31 - 1 workgroups."""
    assert b"grid" in _einval(_with(GOOD, N, 2 ** 31))
    _einval(_with(GOOD, N, 2 ** 62))


def test_zero_boards_is_a_noop():
    """n == 0 returns R48_OK without touching a pointer or the GPU, with or without q and legal."""
    lib = _lib.load()
    zero = _with(GOOD, N, 0)
    assert lib.r48_ntuple_search3(*zero) == _lib.R48_OK
    assert lib.r48_ntuple_search3(*_with(_with(zero, Q, None), LEGAL, None)) == _lib.R48_OK
