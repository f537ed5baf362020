"""Argument errors of r48_ntuple_carousel without a GPU: every refusal the header lists comes back
as R48_EINVAL with a message that names the function and what is wrong, before any HIP call (the
pointers are host stand-ins that are never dereferenced on these paths); n == 0 is a no-op after the
checks."""
import ctypes as C

import pytest

from rein48_amd import _lib
from test_ntuple_abi import ODD, P, _einval, _with

NAME = "r48_ntuple_carousel"


def cuts(*c):
    return (C.c_uint8 * max(1, len(c)))(*c)


# boards, n, done, cuts, n_cuts, pool, pool_has, seen, turn, starts, seed, gid0, ctr, stream
GOOD = (P, 4, P, cuts(9), 1, P, P, P, P, P, 7, 0, 0, None)
BOARDS, N, DONE, CUTS, N_CUTS, POOL, POOL_HAS, SEEN, TURN, STARTS = range(10)


def _refused(args, what):
    lib = _lib.load()
    _einval(lib, NAME, args)
    assert what in lib.r48_last_error(), lib.r48_last_error()


def test_the_signature_is_registered():
    assert len(_lib.SIGNATURES[NAME][1]) == len(GOOD)
    assert _lib.SIGNATURES[NAME][1][10] is C.c_uint64 and _lib.SIGNATURES[NAME][1][12] is C.c_uint32


@pytest.mark.parametrize("n", [4, 0])
def test_null_pointers_are_refused(n):
    base = _with(GOOD, N, n)   # also with n == 0: the checks come before the no-op return
    for k, name in ((BOARDS, b"boards"), (DONE, b"done"), (CUTS, b"cuts"), (POOL, b"pool"), (POOL_HAS, b"pool_has"),
                    (SEEN, b"seen"), (TURN, b"turn")):
        _refused(_with(base, k, None), name + b" is NULL")


@pytest.mark.parametrize("n", [4, 0])
def test_misaligned_pointers_are_refused(n):
    base = _with(GOOD, N, n)
    _refused(_with(base, BOARDS, ODD), b"boards is not 16-byte aligned")
    _refused(_with(base, POOL, ODD), b"pool is not 16-byte aligned")
    _refused(_with(base, STARTS, C.c_void_p(0x1004)), b"starts is not 8-byte aligned")
    # the byte buffers need no alignment, and 8 bytes are enough for starts
    zero = _with(GOOD, N, 0)
    for k in (DONE, POOL_HAS, SEEN, TURN):
        assert getattr(_lib.load(), NAME)(*_with(zero, k, C.c_void_p(0x1001))) == _lib.R48_OK
    assert getattr(_lib.load(), NAME)(*_with(zero, STARTS, ODD)) == _lib.R48_OK


def test_n_out_of_range_is_refused():
    for n in (-1, -5, 2 ** 31, 2 ** 40):
        _refused(_with(GOOD, N, n), b"boards")
    with pytest.raises(_lib.Rein48Error):
        _lib.check(getattr(_lib.load(), NAME)(*_with(GOOD, N, -5)))


@pytest.mark.parametrize("n", [4, 0])
def test_bad_cuts_are_refused_with_their_message(n):
    base = _with(GOOD, N, n)
    for n_cuts in (0, -1, 4, 100):   # a carousel has at least one cut
        _refused(_with(base, N_CUTS, n_cuts), b"n_cuts must be 1..3")
    for bad in (cuts(0), cuts(16), cuts(255)):
        _refused(_with(base, CUTS, bad), b"a cut is not in 1..15")
    _refused(_with(_with(base, CUTS, cuts(3, 16)), N_CUTS, 2), b"a cut is not in 1..15")
    for bad in (cuts(4, 4), cuts(5, 4)):
        _refused(_with(_with(base, CUTS, bad), N_CUTS, 2), b"cuts are not strictly ascending")
    _refused(_with(_with(base, CUTS, cuts(1, 2, 2)), N_CUTS, 3), b"cuts are not strictly ascending")


def test_zero_boards_is_a_noop():
    """n == 0 returns R48_OK without touching a pointer or the GPU, with 1 to 3 cuts, with and
    without starts."""
    lib = _lib.load()
    zero = _with(GOOD, N, 0)
    assert getattr(lib, NAME)(*zero) == _lib.R48_OK
    assert getattr(lib, NAME)(*_with(zero, STARTS, None)) == _lib.R48_OK
    assert getattr(lib, NAME)(*_with(_with(zero, CUTS, cuts(1, 15)), N_CUTS, 2)) == _lib.R48_OK
    assert getattr(lib, NAME)(*_with(_with(zero, CUTS, cuts(1, 8, 15)), N_CUTS, 3)) == _lib.R48_OK
