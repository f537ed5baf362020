"""Argument errors of r48_ntuple_search_ruled (r48_ntuple.hip) without a GPU: everything
r48_ntuple_search3 refuses (NULL tables or actions, a misaligned q or tables, a bad layout, n < 0, an
n beyond the grid), a NULL rule and a rule entry outside 1..4 come back as R48_EINVAL with a message
naming the function before any HIP call; n == 0 is a no-op after the checks; q, legal and depth_out
may be NULL. The symbol is declared in _lib.py and include/rein48.h."""
import ctypes as C
import os
import re

import pytest

from rein48_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(0x1000)     # a non-NULL, 16-byte aligned stand-in: never dereferenced on these paths
ODD = C.c_void_p(0x1008)   # not 16-byte aligned
ODD4 = C.c_void_p(0x1002)  # not 4-byte aligned
NAME = "r48_ntuple_search_ruled"


def cells(*tuples):
    flat = [c for t in tuples for c in t]
    return (C.c_uint8 * len(flat))(*flat)


def rule(*depths):
    return (C.c_uint8 * 17)(*depths)


GOOD_CELLS = cells((0, 1, 2, 3), (4, 5, 6, 7))      # m = 2, L = 4
GOOD_RULE = rule(4, 4, 3, 3, 3, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1)
# boards, n, cells, m, L, tables, rule, actions, q, legal, depth_out, stream
GOOD = (P, 4, GOOD_CELLS, 2, 4, P, GOOD_RULE, P, P, P, P, None)
BOARDS, N, CELLS, M, LEN, TABLES, RULE, ACTIONS, Q, LEGAL, DEPTH = range(11)


def _with(args, k, v):
    return args[:k] + (v,) + args[k + 1:]


def _einval(args):
    lib = _lib.load()
    assert lib.r48_ntuple_search_ruled(*args) == _lib.R48_EINVAL, args
    msg = lib.r48_last_error()
    assert NAME.encode() in msg and len(msg) > len(NAME) + 10, msg
    return msg


def test_the_binding_mirrors_the_header():
    assert len(_lib.SIGNATURES[NAME][1]) == len(GOOD)
    with open(os.path.join(ROOT, "include", "rein48.h")) as f:
        decl = re.search(r"int %s\(([^;]*)\);" % NAME, f.read())
    assert decl, "include/rein48.h does not declare " + NAME
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    assert len(params) == len(GOOD)
    assert params[RULE] == "const uint8_t *rule" and params[DEPTH] == "uint8_t *depth_out"


def test_null_misaligned_and_negative_arguments():
    for k in (BOARDS, CELLS, TABLES, ACTIONS, RULE):
        _einval(_with(GOOD, k, None))
        _einval(_with(_with(GOOD, k, None), N, 0))              # checked before the no-op return
    _einval(_with(GOOD, N, -1))
    _einval(_with(GOOD, BOARDS, ODD))                           # boards not 16-byte aligned
    _einval(_with(GOOD, Q, ODD4))                               # q not 4-byte aligned
    _einval(_with(GOOD, TABLES, ODD4))
    _einval(_with(_with(GOOD, Q, ODD4), N, 0))
    with pytest.raises(_lib.Rein48Error):
        _lib.check(_lib.load().r48_ntuple_search_ruled(*_with(GOOD, N, -5)))


def test_bad_layouts():
    for n in (4, 0):
        base = _with(GOOD, N, n)
        for m, L in ((0, 4), (9, 4), (-1, 4), (2, 1), (2, 7), (2, 0)):
            _einval(_with(_with(base, M, m), LEN, L))
        _einval(_with(base, CELLS, cells((0, 1, 2, 16), (4, 5, 6, 7))))
        _einval(_with(base, CELLS, cells((0, 1, 2, 3), (4, 5, 6, 4))))


def test_bad_rules():
    """Every entry is a depth 1..4, whichever number of blanks it is for."""
    assert b"rule" in _einval(_with(GOOD, RULE, None))
    for n in (4, 0):
        base = _with(GOOD, N, n)
        for k in (0, 1, 8, 15, 16):
            for bad in (0, 5, 255):
                depths = [2] * 17
                depths[k] = bad
                assert b"rule" in _einval(_with(base, RULE, rule(*depths)))
    for d in (1, 2, 3, 4):                                      # the whole range is accepted
        assert _lib.load().r48_ntuple_search_ruled(*_with(_with(GOOD, N, 0), RULE, rule(*[d] * 17))) == _lib.R48_OK


def test_board_count_beyond_the_grid():
    """One board per workgroup, at most 2^31 - 1 workgroups."""
    assert b"grid" in _einval(_with(GOOD, N, 2 ** 31))
    _einval(_with(GOOD, N, 2 ** 62))


def test_zero_boards_is_a_noop():
    """n == 0 returns R48_OK without touching a pointer or the GPU, with or without the nullable outputs."""
    lib = _lib.load()
    zero = _with(GOOD, N, 0)
    assert lib.r48_ntuple_search_ruled(*zero) == _lib.R48_OK
    assert lib.r48_ntuple_search_ruled(*_with(_with(_with(zero, Q, None), LEGAL, None), DEPTH, None)) == _lib.R48_OK


def test_depth_rule():
    """NTupleNet.depth_rule: 4 where blanks <= d4, else 3 where blanks <= d3, else base."""
    from rein48_amd.ntuple import NTupleNet
    assert NTupleNet.depth_rule(16) == (3,) * 17 and NTupleNet.depth_rule(-1) == (2,) * 17
    assert NTupleNet.depth_rule(6, 2) == (4, 4, 4, 3, 3, 3, 3) + (2,) * 10
    assert NTupleNet.depth_rule(3, 5) == (4,) * 6 + (2,) * 11                   # d4 wins where both hold
    assert NTupleNet.depth_rule(0, base=1) == (3,) + (1,) * 16
    assert NTupleNet.depth_rule(16, 16) == (4,) * 17
    for base in (0, 5):
        with pytest.raises(ValueError):
            NTupleNet.depth_rule(4, base=base)
