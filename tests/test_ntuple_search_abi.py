"""Argument errors of r48_ntuple_search (r48_ntuple.hip) without a GPU: a depth other than 1 or 2,
NULL tables or actions, a misaligned q or tables, a bad layout, n < 0 and an n beyond the grid come
back as R48_EINVAL with a message before any HIP call; n == 0 is a no-op; q and legal may be NULL."""
import ctypes as C

import pytest

from rein48_amd import _lib

P = C.c_void_p(0x1000)     # a non-NULL, 16-byte aligned stand-in: never dereferenced on these paths
ODD = C.c_void_p(0x1008)   # not 16-byte aligned
ODD4 = C.c_void_p(0x1002)  # not 4-byte aligned
NAME = "r48_ntuple_search"


def cells(*tuples):
    flat = [c for t in tuples for c in t]
    return (C.c_uint8 * len(flat))(*flat)


GOOD_CELLS = cells((0, 1, 2, 3), (4, 5, 6, 7))      # m = 2, L = 4
# boards, n, cells, m, L, tables, depth, actions, q, legal, stream
GOOD = (P, 4, GOOD_CELLS, 2, 4, P, 2, P, P, P, None)
BOARDS, N, CELLS, M, LEN, TABLES, DEPTH, ACTIONS, Q, LEGAL = range(10)


def _with(args, k, v):
    return args[:k] + (v,) + args[k + 1:]


def _einval(args):
    lib = _lib.load()
    assert lib.r48_ntuple_search(*args) == _lib.R48_EINVAL, args
    msg = lib.r48_last_error()
    assert NAME.encode() in msg and len(msg) > len(NAME) + 10, msg
    return msg


@pytest.mark.parametrize("depth", [0, 3, -1])
def test_depth_must_be_one_or_two(depth):
    assert b"depth" in _einval(_with(GOOD, DEPTH, depth))
    _einval(_with(_with(GOOD, DEPTH, depth), N, 0))             # checked before the no-op return


def test_null_misaligned_and_negative_arguments():
    for k in (BOARDS, CELLS, TABLES, ACTIONS):
        _einval(_with(GOOD, k, None))
    _einval(_with(GOOD, N, -1))
    _einval(_with(GOOD, BOARDS, ODD))                           # boards not 16-byte aligned
    _einval(_with(GOOD, Q, ODD4))                               # q not 4-byte aligned
    _einval(_with(GOOD, TABLES, ODD4))
    with pytest.raises(_lib.Rein48Error):
        _lib.check(_lib.load().r48_ntuple_search(*_with(GOOD, N, -5)))


def test_bad_layouts():
    for n in (4, 0):
        base = _with(GOOD, N, n)
        for m, L in ((0, 4), (9, 4), (-1, 4), (2, 1), (2, 7), (2, 0)):
            _einval(_with(_with(base, M, m), LEN, L))
        _einval(_with(base, CELLS, cells((0, 1, 2, 16), (4, 5, 6, 7))))
        _einval(_with(base, CELLS, cells((0, 1, 2, 3), (4, 5, 6, 4))))


def test_board_count_beyond_the_grid():
    """One board per wave, 4 waves per workgroup, at most 2^31 - 1 workgroups."""
    assert b"grid" in _einval(_with(GOOD, N, 4 * (2 ** 31 - 1) + 1))
    _einval(_with(GOOD, N, 2 ** 62))


@pytest.mark.parametrize("depth", [1, 2])
def test_zero_boards_is_a_noop(depth):
    """n == 0 returns R48_OK without touching a pointer or the GPU, with or without q and legal."""
    lib = _lib.load()
    zero = _with(_with(GOOD, N, 0), DEPTH, depth)
    assert lib.r48_ntuple_search(*zero) == _lib.R48_OK
    assert lib.r48_ntuple_search(*_with(_with(zero, Q, None), LEGAL, None)) == _lib.R48_OK
