"""Argument errors of the temporal-coherence entry points (r48_ntuple_apply_tc, r48_ntuple_tc_rate)
without a GPU: NULL or misaligned pointers, n < 0 and bad layouts come back as R48_EINVAL with a
message naming the function before any HIP call, and n == 0 is a no-op after the layout check."""
import ctypes as C

import pytest

from rein48_amd import _lib
from test_ntuple_abi import GOOD, ODD, P, _einval, _with, cells

OFF4 = C.c_void_p(0x1004)   # 4-byte aligned, not 8
OFF2 = C.c_void_p(0x1002)   # not 4-byte aligned

# name -> (good argument tuple, indices of the pointer arguments that must not be NULL, index of n,
#          index of cells -- m and L follow it)
CASES = {
    # boards, n, valid, cells, m, L, step, tables, tc_e, tc_a, acc, cnt, stream
    "r48_ntuple_apply_tc": ((P, 4, None, GOOD, 2, 4, 0.1, P, P, P, P, P, None), (0, 3, 7, 8, 9, 10, 11), 1, 3),
    # boards, n, cells, m, L, tc_e, tc_a, rate_out, stream
    "r48_ntuple_tc_rate": ((P, 4, GOOD, 2, 4, P, P, P, None), (0, 2, 5, 6, 7), 1, 2),
}
# argument index -> the least misalignment that must be refused
MISALIGNED = {
    "r48_ntuple_apply_tc": {7: OFF2, 8: OFF2, 9: OFF2, 10: OFF4, 11: OFF2},
    "r48_ntuple_tc_rate": {5: OFF2, 6: OFF2, 7: OFF2},
}


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
        _einval(lib, name, _with(base, c_at, cells((0, 1, 2, 3), (4, 5, 6, 4))))
    eight = cells(*[(k, k + 1) for k in range(8)])
    assert getattr(lib, name)(*_with(_with(_with(_with(good, n_at, 0), c_at, eight), c_at + 1, 8), c_at + 2, 2)) == _lib.R48_OK


@pytest.mark.parametrize("name", sorted(CASES))
def test_misaligned_tables_and_scratch(name):
    """acc must be 8-byte aligned, every float table and cnt 4-byte aligned -- also with n == 0."""
    lib = _lib.load()
    good, _, n_at, _ = CASES[name]
    for k, bad in MISALIGNED[name].items():
        _einval(lib, name, _with(good, k, bad))
        _einval(lib, name, _with(_with(good, n_at, 0), k, bad))
    if name == "r48_ntuple_apply_tc":      # 4-byte alignment is enough for the float tables and cnt
        ok = _with(good, n_at, 0)
        for k in (7, 8, 9, 11):
            ok = _with(ok, k, OFF4)
        assert getattr(lib, name)(*ok) == _lib.R48_OK


@pytest.mark.parametrize("name", sorted(CASES))
def test_zero_boards_is_a_noop(name):
    """n == 0 returns R48_OK without touching a pointer or the GPU."""
    good, _, n_at, _ = CASES[name]
    assert getattr(_lib.load(), name)(*_with(good, n_at, 0)) == _lib.R48_OK
