"""Argument errors of r48_ntuple_play (r48_ntuple.hip) without a GPU: a depth other than 1 or 2,
n_steps < 0, NULL tables, misaligned boards (16 bytes), tables, length or gain (4 bytes), a bad
layout, n < 0 and an n beyond depth 2's grid come back as R48_EINVAL with a message naming the
function and the argument before any HIP call; n == 0 or n_steps == 0 is a no-op after these checks;
length, gain and done may be NULL."""
import ctypes as C
import os
import re

import pytest

from rein48_amd import _lib
from test_ntuple_abi import ODD, _with, cells

NAME = "r48_ntuple_play"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF2 = C.c_void_p(0x1002)   # not 4-byte aligned


def at(k):
    """Distinct 16-byte aligned stand-ins, never dereferenced on these paths."""
    return C.c_void_p(0x1000 + 0x100 * k)


GOOD_CELLS = cells((0, 1, 2, 3), (4, 5, 6, 7))      # m = 2, L = 4
(BOARDS, N, CELLS, M, LEN, TABLES, DEPTH, N_STEPS, ENV_SEED, GID0, ENV_STEP, LENGTH, GAIN, DONE, STREAM) = range(15)
GOOD = (at(BOARDS), 4, GOOD_CELLS, 2, 4, at(TABLES), 1, 3, 0x2048, 1, 150, at(LENGTH), at(GAIN), at(DONE), None)
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
    with open(os.path.join(ROOT, "include", "rein48.h")) as f:
        decl = re.search(r"\bint %s\(([^)]*)\);" % NAME, f.read())
    assert decl is not None
    names = [p.split()[-1].lstrip("*") for p in decl.group(1).split(",")]
    assert names == ["boards", "n", "cells", "m", "L", "tables", "depth", "n_steps", "env_seed", "gid0", "env_step",
                     "length", "gain", "done", "stream"]


@pytest.mark.parametrize("depth", [0, 3, -1])
def test_depth_must_be_one_or_two(depth):
    _einval_also_without_work(_with(GOOD, DEPTH, depth), b"depth")


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


def test_board_count_beyond_the_grid_at_depth_two():
    """r48_ntuple_search's limit: one board per wave, 4 waves per workgroup, at most 2^31 - 1 workgroups."""
    two = _with(GOOD, DEPTH, 2)
    _einval(_with(two, N, 4 * (2 ** 31 - 1) + 1), b"grid")
    _einval(_with(_with(two, N, 4 * (2 ** 31 - 1) + 1), N_STEPS, 0), b"grid")
    _einval(_with(two, N, 2 ** 62), b"grid")


@pytest.mark.parametrize("depth", [1, 2])
def test_no_boards_or_no_steps_is_a_noop(depth):
    """R48_OK without touching a pointer or the GPU, with or without length, gain and done."""
    lib = _lib.load()
    for k, v in NO_WORK:
        args = _with(_with(GOOD, DEPTH, depth), k, v)
        assert getattr(lib, NAME)(*args) == _lib.R48_OK
        assert getattr(lib, NAME)(*_with(_with(_with(args, LENGTH, None), GAIN, None), DONE, None)) == _lib.R48_OK
