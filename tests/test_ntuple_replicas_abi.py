"""Argument errors of the replica entry points (r48_ntuple_td_act_replicas, r48_ntuple_apply_replicas,
r48_ntuple_apply_tc_replicas; r48_ntuple.hip) without a GPU: everything the unstaged parents refuse,
replicas outside 1..64, n not a multiple of replicas, a NULL or misaligned steps and more than 2^32
entries come back as R48_EINVAL with a message naming the function before any HIP call; n == 0 is a
no-op after the checks; reward and delta_out may be NULL."""
import ctypes as C
import os
import re

import pytest

from rein48_amd import _lib
from test_ntuple_abi import ODD, _with, cells

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF4 = C.c_void_p(0x1004)   # 4-byte aligned, not 8
OFF2 = C.c_void_p(0x1002)   # not 4-byte aligned
GOOD_CELLS = cells((0, 1, 2, 3), (4, 5, 6, 7))      # m = 2, L = 4

PARAMS = {
    "r48_ntuple_td_act_replicas": ["boards", "n", "replicas", "cells", "m", "L", "tables", "prev_after", "prev_value",
                                   "prev_done", "prev_valid", "actions", "after", "value", "reward", "legal", "valid_out",
                                   "delta_out", "acc", "cnt", "stream"],
    "r48_ntuple_apply_replicas": ["boards", "n", "replicas", "valid", "cells", "m", "L", "steps", "tables", "acc", "cnt",
                                  "stream"],
    "r48_ntuple_apply_tc_replicas": ["boards", "n", "replicas", "valid", "cells", "m", "L", "steps", "tables", "tc_e",
                                     "tc_a", "acc", "cnt", "stream"],
}
NULLABLE = {"reward", "delta_out", "valid", "stream"}
# pointer argument -> the least misalignment that must be refused
MISALIGNED = {"boards": ODD, "prev_after": ODD, "after": ODD, "acc": OFF4, "tables": OFF2, "prev_value": OFF2,
              "value": OFF2, "reward": OFF2, "delta_out": OFF2, "cnt": OFF2, "steps": OFF2, "tc_e": OFF2, "tc_a": OFF2}
NAMES = sorted(PARAMS)


def at(k):
    """Distinct 16-byte aligned stand-ins, never dereferenced on these paths."""
    return C.c_void_p(0x1000 + 0x100 * k)


def good(name, n=6, replicas=3):
    """A good argument tuple of `name`: n = 6 boards in 3 replicas of the m = 2, L = 4 layout."""
    fixed = {"n": n, "replicas": replicas, "cells": GOOD_CELLS, "m": 2, "L": 4, "stream": None, "valid": None}
    return tuple(fixed[p] if p in fixed else at(k) for k, p in enumerate(PARAMS[name]))


def put(name, args, **kw):
    for p, v in kw.items():
        args = _with(args, PARAMS[name].index(p), v)
    return args


def _einval(name, args):
    lib = _lib.load()
    assert getattr(lib, name)(*args) == _lib.R48_EINVAL, (name, args)
    msg = lib.r48_last_error()
    assert name.encode() in msg and len(msg) > len(name) + 10, msg
    return msg


def _ok(name, args):
    lib = _lib.load()
    assert getattr(lib, name)(*args) == _lib.R48_OK, (name, args, lib.r48_last_error())


@pytest.mark.parametrize("name", NAMES)
def test_the_symbol_is_exported_and_the_binding_mirrors_the_header(name):
    assert hasattr(_lib.load(), name)
    assert len(_lib.SIGNATURES[name][1]) == len(PARAMS[name])
    with open(os.path.join(ROOT, "include", "rein48.h")) as f:
        decl = re.search(r"\bint %s\(([^)]*)\);" % name, f.read())
    assert decl is not None
    assert [p.split()[-1].lstrip("*") for p in decl.group(1).split(",")] == PARAMS[name]


@pytest.mark.parametrize("name", NAMES)
def test_null_and_negative_arguments(name):
    for p in PARAMS[name]:
        if p in NULLABLE or p in ("n", "replicas", "m", "L"):
            continue
        _einval(name, put(name, good(name), **{p: None}))
        _einval(name, put(name, good(name, n=0), **{p: None}))     # checked before the no-op return
    _einval(name, put(name, good(name), n=-3))
    with pytest.raises(_lib.Rein48Error):
        _lib.check(getattr(_lib.load(), name)(*put(name, good(name), n=-6)))


@pytest.mark.parametrize("name", NAMES)
def test_misaligned_arguments(name):
    """Boards and afterstates 16 bytes, acc 8 bytes, floats (steps among them), reward and cnt 4 bytes --
    also with n == 0; 4 bytes are enough for the latter."""
    ok = good(name, n=0)
    for j, p in enumerate(PARAMS[name]):
        if p not in MISALIGNED:
            continue
        _einval(name, put(name, good(name), **{p: MISALIGNED[p]}))
        _einval(name, put(name, good(name, n=0), **{p: MISALIGNED[p]}))
        if MISALIGNED[p] is OFF2:
            ok = put(name, ok, **{p: C.c_void_p(0x2004 + 0x100 * j)})
    _ok(name, ok)


def test_outputs_must_not_alias_the_previous_buffers():
    name = "r48_ntuple_td_act_replicas"
    for out, prev in (("after", "prev_after"), ("value", "prev_value"), ("valid_out", "prev_valid")):
        for n in (6, 0):
            g = good(name, n=n)
            _einval(name, put(name, g, **{out: g[PARAMS[name].index(prev)]}))
            _einval(name, put(name, g, **{prev: g[PARAMS[name].index(out)]}))


@pytest.mark.parametrize("name", NAMES)
def test_bad_layouts(name):
    """m outside 1..8, L outside 2..6, a cell >= 16, a cell repeated within a tuple -- also with n == 0."""
    for n in (6, 0):
        base = good(name, n=n)
        for m, L in ((0, 4), (9, 4), (-1, 4), (2, 1), (2, 7), (2, 0)):
            _einval(name, put(name, base, m=m, L=L))
        _einval(name, put(name, base, cells=cells((0, 1, 2, 16), (4, 5, 6, 7))))
        _einval(name, put(name, base, cells=cells((0, 1, 2, 3), (4, 5, 6, 4))))


@pytest.mark.parametrize("name", NAMES)
def test_replicas_and_n(name):
    """replicas is 1..64 and divides n -- also with n == 0, where every count in range divides."""
    for n in (6, 0):
        for replicas in (0, -1, 65, 1 << 20):
            _einval(name, good(name, n=n, replicas=replicas))
    for n, replicas in ((7, 3), (6, 4), (1, 2), (63, 64)):
        _einval(name, good(name, n=n, replicas=replicas))
    for replicas in (1, 3, 64):
        _ok(name, good(name, n=0, replicas=replicas))


@pytest.mark.parametrize("name", NAMES)
def test_the_entry_count_is_bounded_by_2_to_the_32(name):
    """L = 6, m = 8 is 2^27 entries a replica: 32 replicas are exactly 2^32 and accepted, 33 are refused."""
    eight = cells(*[(k, k + 1, k + 2, k + 3, k + 4, k + 5) for k in range(8)])
    big = put(name, good(name, n=0), cells=eight, m=8, L=6)
    _ok(name, put(name, big, replicas=32))
    _einval(name, put(name, big, replicas=33))
    _einval(name, put(name, big, replicas=64))
    _einval(name, put(name, big, replicas=33, n=33))
    _ok(name, put(name, good(name, n=0), cells=cells((0, 1, 2, 3, 4, 5)), m=1, L=6, replicas=64))


@pytest.mark.parametrize("name", NAMES)
def test_zero_boards_is_a_noop(name):
    """n == 0 returns R48_OK without touching a pointer or the GPU; reward and delta_out may be NULL."""
    _ok(name, good(name, n=0))
    if name == "r48_ntuple_td_act_replicas":
        _ok(name, put(name, good(name, n=0), reward=None, delta_out=None))
