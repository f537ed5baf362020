"""Argument errors of r48_ntuple_play_ruled (r48_ntuple.hip) without a GPU: what r48_ntuple_play
refuses (n_steps < 0, NULL tables, misaligned boards (16 bytes), tables, length or gain (4 bytes), a
bad layout, n < 0) and what r48_ntuple_search_ruled refuses (a NULL rule, a rule entry outside 1..4,
n beyond 2^31 - 1 boards) come back as R48_EINVAL before any HIP call, with r48_last_error naming the
function and the argument; n == 0 or n_steps == 0 is a no-op after these checks; length, gain and
done may be NULL. r48_ntuple_play keeps refusing depth 3."""
import ctypes as C
import os
import re

import pytest

from rein48_amd import _lib
from test_ntuple_abi import ODD, _with, cells

NAME = "r48_ntuple_play_ruled"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF2 = C.c_void_p(0x1002)   # not 4-byte aligned


def at(k):
    """Distinct 16-byte aligned stand-ins, never dereferenced on these paths."""
    return C.c_void_p(0x1000 + 0x100 * k)


def rule(*depths):
    return (C.c_uint8 * 17)(*depths)


GOOD_CELLS = cells((0, 1, 2, 3), (4, 5, 6, 7))      # m = 2, L = 4
GOOD_RULE = rule(4, 4, 3, 3, 3, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1)
(BOARDS, N, CELLS, M, LEN, TABLES, RULE, N_STEPS, ENV_SEED, GID0, ENV_STEP, LENGTH, GAIN, DONE, STREAM) = range(15)
GOOD = (at(BOARDS), 4, GOOD_CELLS, 2, 4, at(TABLES), GOOD_RULE, 3, 0x2048, 1, 150, at(LENGTH), at(GAIN), at(DONE), None)
NO_WORK = ((N, 0), (N_STEPS, 0))                    # either makes the call a no-op, after the checks


def _einval(args, word=None):
    lib = _lib.load()
    assert getattr(lib, NAME)(*args) == _lib.R48_EINVAL, args
    msg = lib.r48_last_error()
    assert NAME.encode() in msg and len(msg) > len(NAME) + 10, msg
    if word is not None:
        assert word in msg, msg
    return msg


def _einval_also_without_work(args, word):
    _einval(args, word)
    for k, v in NO_WORK:
        _einval(_with(args, k, v), word)            # checked before the no-op return


def test_the_symbol_is_exported_and_the_binding_mirrors_the_header():
    assert hasattr(_lib.load(), NAME)
    assert len(_lib.SIGNATURES[NAME][1]) == len(GOOD)
    assert _lib.SIGNATURES[NAME][1][RULE] is C.c_void_p and _lib.SIGNATURES[NAME][1][N_STEPS] is C.c_int32
    with open(os.path.join(ROOT, "include", "rein48.h")) as f:
        decl = re.search(r"\bint %s\(([^)]*)\);" % NAME, f.read())
    assert decl is not None
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "boards", "n", "cells", "m", "L", "tables", "rule", "n_steps", "env_seed", "gid0", "env_step", "length", "gain",
        "done", "stream"]
    assert params[RULE] == "const uint8_t *rule" and params[BOARDS] == "int8_t *boards"


def test_bad_rules():
    """A NULL rule, and every entry a depth 1..4, whichever number of blanks it is for."""
    _einval_also_without_work(_with(GOOD, RULE, None), b"rule")
    for k in (0, 1, 8, 15, 16):
        for bad in (0, 5, 255):
            depths = [2] * 17
            depths[k] = bad
            _einval_also_without_work(_with(GOOD, RULE, rule(*depths)), b"rule")
    for d in (1, 2, 3, 4):                                      # the whole range is accepted
        assert getattr(_lib.load(), NAME)(*_with(_with(GOOD, N, 0), RULE, rule(*[d] * 17))) == _lib.R48_OK


@pytest.mark.parametrize("n_steps", [-1, -(2 ** 31)])
def test_n_steps_must_not_be_negative(n_steps):
    _einval(_with(GOOD, N_STEPS, n_steps), b"n_steps")
    _einval(_with(_with(GOOD, N_STEPS, n_steps), N, 0), b"n_steps")


def test_null_and_negative_arguments():
    _einval_also_without_work(_with(GOOD, TABLES, None), b"tables")
    _einval_also_without_work(_with(GOOD, BOARDS, None), b"boards")
    _einval_also_without_work(_with(GOOD, CELLS, None), b"cells")
    _einval(_with(GOOD, N, -1), b"n < 0")
    with pytest.raises(_lib.Rein48Error):
        _lib.check(getattr(_lib.load(), NAME)(*_with(GOOD, N, -5)))


def test_misaligned_arguments():
    """Boards 16 bytes; tables, length and gain 4 bytes -- also where the call has no work to do."""
    for k, bad, word in ((BOARDS, ODD, b"boards"), (TABLES, OFF2, b"tables"), (LENGTH, OFF2, b"length"),
                         (GAIN, OFF2, b"gain")):
        _einval_also_without_work(_with(GOOD, k, bad), word)
    ok = _with(GOOD, N, 0)                                      # 4 bytes are enough for them, 1 for done
    for j, k in enumerate((TABLES, LENGTH, GAIN)):
        ok = _with(ok, k, C.c_void_p(0x2004 + 0x100 * j))
    ok = _with(ok, DONE, C.c_void_p(0x3001))
    assert getattr(_lib.load(), NAME)(*ok) == _lib.R48_OK


def test_bad_layouts():
    for k, v in NO_WORK + ((N, 4),):
        base = _with(GOOD, k, v)
        for m, L in ((0, 4), (9, 4), (-1, 4), (2, 1), (2, 7), (2, 0)):
            _einval(_with(_with(base, M, m), LEN, L), b"layout")
        _einval(_with(base, CELLS, cells((0, 1, 2, 16), (4, 5, 6, 7))), b"layout")
        _einval(_with(base, CELLS, cells((0, 1, 2, 3), (4, 5, 6, 4))), b"layout")


def test_board_count_beyond_the_grid():
    """r48_ntuple_search_ruled's limit: one board per workgroup, at most 2^31 - 1 workgroups."""
    _einval(_with(GOOD, N, 2 ** 31), b"grid")
    _einval(_with(_with(GOOD, N, 2 ** 31), N_STEPS, 0), b"grid")
    _einval(_with(GOOD, N, 2 ** 62), b"grid")


def test_no_boards_or_no_steps_is_a_noop():
    """R48_OK without touching a pointer or the GPU, with or without length, gain and done."""
    lib = _lib.load()
    for k, v in NO_WORK:
        args = _with(GOOD, k, v)
        assert getattr(lib, NAME)(*args) == _lib.R48_OK
        assert getattr(lib, NAME)(*_with(_with(_with(args, LENGTH, None), GAIN, None), DONE, None)) == _lib.R48_OK


def test_the_plain_play_keeps_refusing_depth_three():
    lib = _lib.load()
    args = (at(0), 4, GOOD_CELLS, 2, 4, at(5), 3, 3, 0x2048, 1, 150, at(11), at(12), at(13), None)
    assert lib.r48_ntuple_play(*args) == _lib.R48_EINVAL and b"depth" in lib.r48_last_error()
