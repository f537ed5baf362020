"""Argument errors of r48_ntuple_td_act (r48_ntuple.hip) without a GPU: NULL or misaligned pointers,
outputs that alias the previous step's buffers, n < 0 and bad layouts come back as R48_EINVAL with a
message naming the function before any HIP call; n == 0 is a no-op after the layout check; reward
and delta_out may be NULL."""
import ctypes as C
import os
import re

import pytest

from rein48_amd import _lib
from test_ntuple_abi import ODD, _with, cells

NAME = "r48_ntuple_td_act"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF4 = C.c_void_p(0x1004)   # 4-byte aligned, not 8
OFF2 = C.c_void_p(0x1002)   # not 4-byte aligned


def at(k):
    """Distinct 16-byte aligned stand-ins, never dereferenced on these paths."""
    return C.c_void_p(0x1000 + 0x100 * k)


GOOD_CELLS = cells((0, 1, 2, 3), (4, 5, 6, 7))      # m = 2, L = 4
(BOARDS, N, CELLS, M, LEN, TABLES, PREV_AFTER, PREV_VALUE, PREV_DONE, PREV_VALID, ACTIONS, AFTER, VALUE, REWARD, LEGAL,
 VALID_OUT, DELTA_OUT, ACC, CNT, STREAM) = range(20)
GOOD = tuple(4 if k == N else GOOD_CELLS if k == CELLS else 2 if k == M else 4 if k == LEN else None if k == STREAM else at(k)
             for k in range(20))
REQUIRED = (BOARDS, CELLS, TABLES, PREV_AFTER, PREV_VALUE, PREV_DONE, PREV_VALID, ACTIONS, AFTER, VALUE, LEGAL, VALID_OUT,
            ACC, CNT)
# argument -> the least misalignment that must be refused
MISALIGNED = {BOARDS: ODD, PREV_AFTER: ODD, AFTER: ODD, ACC: OFF4, TABLES: OFF2, PREV_VALUE: OFF2, VALUE: OFF2,
              REWARD: OFF2, DELTA_OUT: OFF2, CNT: OFF2}


def _einval(args):
    lib = _lib.load()
    assert getattr(lib, NAME)(*args) == _lib.R48_EINVAL, args
    msg = lib.r48_last_error()
    assert NAME.encode() in msg and len(msg) > len(NAME) + 10, msg
    return msg


def test_the_symbol_is_exported_and_the_binding_mirrors_the_header():
    assert hasattr(_lib.load(), NAME)
    assert len(_lib.SIGNATURES[NAME][1]) == len(GOOD)
    with open(os.path.join(ROOT, "include", "rein48.h")) as f:
        decl = re.search(r"\bint %s\(([^)]*)\);" % NAME, f.read())
    assert decl is not None
    names = [p.split()[-1].lstrip("*") for p in decl.group(1).split(",")]
    assert names == ["boards", "n", "cells", "m", "L", "tables", "prev_after", "prev_value", "prev_done", "prev_valid",
                     "actions", "after", "value", "reward", "legal", "valid_out", "delta_out", "acc", "cnt", "stream"]


def test_null_and_negative_arguments():
    for k in REQUIRED:
        _einval(_with(GOOD, k, None))
        _einval(_with(_with(GOOD, k, None), N, 0))              # checked before the no-op return
    _einval(_with(GOOD, N, -1))
    with pytest.raises(_lib.Rein48Error):
        _lib.check(getattr(_lib.load(), NAME)(*_with(GOOD, N, -5)))


def test_misaligned_arguments():
    """Boards and afterstates 16 bytes, acc 8 bytes, floats, reward and cnt 4 bytes -- also with n == 0."""
    for k, bad in MISALIGNED.items():
        _einval(_with(GOOD, k, bad))
        _einval(_with(_with(GOOD, k, bad), N, 0))
    ok = _with(GOOD, N, 0)                                      # 4 bytes are enough for the floats, reward and cnt
    for j, k in enumerate((TABLES, PREV_VALUE, VALUE, REWARD, DELTA_OUT, CNT)):
        ok = _with(ok, k, C.c_void_p(0x2004 + 0x100 * j))
    assert getattr(_lib.load(), NAME)(*ok) == _lib.R48_OK


def test_outputs_must_not_alias_the_previous_buffers():
    """apply reads prev_after and prev_valid after this call, and prev_value is read by every lane
    while others write value."""
    for out, prev in ((AFTER, PREV_AFTER), (VALUE, PREV_VALUE), (VALID_OUT, PREV_VALID)):
        _einval(_with(GOOD, out, GOOD[prev]))
        _einval(_with(_with(GOOD, out, GOOD[prev]), N, 0))
        _einval(_with(GOOD, prev, GOOD[out]))


def test_bad_layouts():
    """m outside 1..8, L outside 2..6, a cell >= 16, a cell repeated within a tuple -- also with
    n == 0: the layout is checked before the no-op return."""
    lib = _lib.load()
    for n in (4, 0):
        base = _with(GOOD, N, n)
        for m, L in ((0, 4), (9, 4), (-1, 4), (2, 1), (2, 7), (2, 0)):
            _einval(_with(_with(base, M, m), LEN, L))
        _einval(_with(base, CELLS, cells((0, 1, 2, 16), (4, 5, 6, 7))))
        _einval(_with(base, CELLS, cells((0, 1, 2, 255), (4, 5, 6, 7))))
        _einval(_with(base, CELLS, cells((0, 1, 2, 3), (4, 5, 6, 4))))
    zero = _with(GOOD, N, 0)
    eight = cells(*[(k, k + 1) for k in range(8)])
    assert getattr(lib, NAME)(*_with(_with(_with(zero, CELLS, eight), M, 8), LEN, 2)) == _lib.R48_OK
    six = cells((0, 1, 2, 3, 4, 5))
    assert getattr(lib, NAME)(*_with(_with(_with(zero, CELLS, six), M, 1), LEN, 6)) == _lib.R48_OK


def test_zero_boards_is_a_noop():
    """n == 0 returns R48_OK without touching a pointer or the GPU, with or without reward and delta_out."""
    lib = _lib.load()
    zero = _with(GOOD, N, 0)
    assert getattr(lib, NAME)(*zero) == _lib.R48_OK
    assert getattr(lib, NAME)(*_with(_with(zero, REWARD, None), DELTA_OUT, None)) == _lib.R48_OK
