"""Argument errors of the twelve _staged n-tuple entry points without a GPU: bad cuts and a missing
own come back as R48_EINVAL with a message that names the function and what is wrong, before any HIP
call; the plain entry point's own refusals still hold under the twin's name; n == 0 is a no-op, and
n_cuts == 0 needs neither cuts nor own."""
import ctypes as C

import pytest

from rein48_amd import _lib
from test_ntuple_abi import GOOD, ODD, P, _einval, _with

RULE = (C.c_uint8 * 17)(*([2] * 17))


def cuts(*c):
    return (C.c_uint8 * max(1, len(c)))(*c)


ONE = cuts(9)

# name -> (good argument tuple with cuts = (9,), index of cuts -- n_cuts follows it, index of own or None)
CASES = {
    # boards, n, cells, m, L, cuts, n_cuts, tables, value, stream
    "r48_ntuple_value_staged": ((P, 4, GOOD, 2, 4, ONE, 1, P, P, None), 5, None),
    # ..., tables, actions, after, value, reward, legal, stream
    "r48_ntuple_act_staged": ((P, 4, GOOD, 2, 4, ONE, 1, P, P, None, None, None, None, None), 5, None),
    # ..., tables, prev_after, prev_value, prev_done, prev_valid, actions, after, value, reward, legal, valid_out,
    # delta_out, acc, cnt, own, stream (distinct stand-ins for the buffers that must differ)
    "r48_ntuple_td_act_staged": ((P, 4, GOOD, 2, 4, ONE, 1, P, C.c_void_p(0x2000), C.c_void_p(0x3000), P,
                                  C.c_void_p(0x4000), P, P, P, None, P, P, None, P, P, P, None), 5, 21),
    # ..., tables, depth, actions, q, legal, stream
    "r48_ntuple_search_staged": ((P, 4, GOOD, 2, 4, ONE, 1, P, 2, P, None, None, None), 5, None),
    "r48_ntuple_search3_staged": ((P, 4, GOOD, 2, 4, ONE, 1, P, P, None, None, None), 5, None),
    # ..., tables, rule, actions, q, legal, depth_out, stream
    "r48_ntuple_search_ruled_staged": ((P, 4, GOOD, 2, 4, ONE, 1, P, RULE, P, None, None, None, None), 5, None),
    # ..., tables, depth, n_steps, env_seed, gid0, env_step, length, gain, done, stream
    "r48_ntuple_play_staged": ((P, 4, GOOD, 2, 4, ONE, 1, P, 1, 3, 7, 0, 0, None, None, None, None), 5, None),
    # ..., tables, rule, n_steps, env_seed, gid0, env_step, length, gain, done, stream
    "r48_ntuple_play_ruled_staged": ((P, 4, GOOD, 2, 4, ONE, 1, P, RULE, 3, 7, 0, 0, None, None, None, None), 5, None),
    # boards, n, delta, valid, cells, m, L, cuts, n_cuts, acc, cnt, own, stream
    "r48_ntuple_accumulate_staged": ((P, 4, P, None, GOOD, 2, 4, ONE, 1, P, P, P, None), 7, 11),
    # boards, n, valid, cells, m, L, cuts, n_cuts, step, tables, acc, cnt, own, stream
    "r48_ntuple_apply_staged": ((P, 4, None, GOOD, 2, 4, ONE, 1, 0.1, P, P, P, P, None), 6, 12),
    # ..., step, tables, tc_e, tc_a, acc, cnt, own, stream
    "r48_ntuple_apply_tc_staged": ((P, 4, None, GOOD, 2, 4, ONE, 1, 0.1, P, P, P, P, P, P, None), 6, 14),
    # boards, n, cells, m, L, cuts, n_cuts, tc_e, tc_a, rate_out, stream
    "r48_ntuple_tc_rate_staged": ((P, 4, GOOD, 2, 4, ONE, 1, P, P, P, None), 5, None),
}


def _refused(lib, name, args, what):
    _einval(lib, name, args)
    assert what in lib.r48_last_error(), lib.r48_last_error()


def test_every_twin_is_covered():
    assert sorted(CASES) == sorted(n for n in _lib.SIGNATURES if n.endswith("_staged"))
    assert len(CASES) == 12


@pytest.mark.parametrize("name", sorted(CASES))
def test_bad_cuts_are_refused_with_their_message(name):
    lib = _lib.load()
    good, c_at, _ = CASES[name]
    for n in (4, 0):   # also with n == 0: the cuts are checked before the no-op return
        base = _with(good, 1, n)
        for n_cuts in (-1, 4, 100):
            _refused(lib, name, _with(base, c_at + 1, n_cuts), b"n_cuts must be 0..3")
        _refused(lib, name, _with(base, c_at, None), b"cuts is NULL")
        for bad in (cuts(0), cuts(16), cuts(255)):
            _refused(lib, name, _with(base, c_at, bad), b"a cut is not in 1..15")
        _refused(lib, name, _with(_with(base, c_at, cuts(3, 16)), c_at + 1, 2), b"a cut is not in 1..15")
        for bad in (cuts(4, 4), cuts(5, 4)):
            _refused(lib, name, _with(_with(base, c_at, bad), c_at + 1, 2), b"cuts are not strictly ascending")
        _refused(lib, name, _with(_with(base, c_at, cuts(1, 2, 2)), c_at + 1, 3), b"cuts are not strictly ascending")


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c[2] is not None))
def test_a_staged_update_needs_own(name):
    lib = _lib.load()
    good, c_at, own_at = CASES[name]
    _refused(lib, name, _with(good, own_at, None), b"own is NULL")
    _refused(lib, name, _with(_with(good, 1, 0), own_at, None), b"own is NULL")


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_plain_refusals_hold_under_the_twins_name(name):
    lib = _lib.load()
    good, c_at, _ = CASES[name]
    _einval(lib, name, _with(good, 0, None))
    _einval(lib, name, _with(good, 0, ODD))
    _einval(lib, name, _with(good, 1, -1))
    m_at = good.index(GOOD) + 1
    _refused(lib, name, _with(good, m_at, 9), b"bad layout")
    assert name.encode() + b":" in lib.r48_last_error()


@pytest.mark.parametrize("name", sorted(CASES))
def test_zero_boards_is_a_noop(name):
    """n == 0 returns R48_OK without touching a pointer or the GPU, with 1 to 3 cuts and with none;
    n_cuts == 0 needs neither cuts nor own."""
    lib = _lib.load()
    good, c_at, own_at = CASES[name]
    zero = _with(good, 1, 0)
    assert getattr(lib, name)(*zero) == _lib.R48_OK
    assert getattr(lib, name)(*_with(_with(zero, c_at, cuts(1, 8, 15)), c_at + 1, 3)) == _lib.R48_OK
    none = _with(_with(zero, c_at, None), c_at + 1, 0)
    if own_at is not None:
        none = _with(none, own_at, None)
    assert getattr(lib, name)(*none) == _lib.R48_OK
