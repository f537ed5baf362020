"""The fused TD step's kernel (k_nt_td_act in r48_ntuple.hip, NTupleNet.td_act) on the GPU against the
three steps it replaces, bit for bit: NTupleNet.act, the trainer's torch expression for delta, and
NTupleNet.accumulate on a twin net with the same tables.

Board counts 1, 63, 257 and 1,000: a single lane, a partial wave, one workgroup plus one lane and a
ragged last workgroup. Layouts: lines-squares and one custom layout each of tuple length 2, 3 and 5
and a single 6-tuple, so every instantiation of the kernel runs. Boards are those of running games
(150 greedy-merge steps from reset with auto-reset, made once and shared) with one board that has no
legal move at row 3. The previous step's state is random: boards with exponents up to 17, values,
about a quarter of the rows done and about a quarter not valid. Tables are random floats; a second
case scales them to ~2^21, so that most deltas lie beyond the +-2^20 clamp.
"""
import functools

import numpy as np
import pytest
import torch

from test_moves_gpu import NO_MOVES, T
from test_ntuple_gpu import guard_ok, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTS = [1, 63, 257, 1000]
NMAX = max(COUNTS)
I_NO_MOVES = 3
LAYOUTS = {
    "lines-squares": "lines-squares",
    "3x2": ((0, 1), (5, 6), (3, 7)),
    "3x3": ((0, 1, 2), (5, 9, 10), (15, 3, 12)),
    "2x5": ((0, 1, 2, 3, 4), (5, 6, 9, 10, 13)),
    "1x6": ((0, 1, 2, 4, 5, 6),),
}
SCALES = {"float": 37.0, "clamp": 2.0 ** 21}
CASES = [(lay, n, kind) for lay in LAYOUTS for n in COUNTS for kind in SCALES]


@functools.lru_cache(maxsize=None)
def pool():
    """int8 [NMAX, 16] on the host, read-only: boards of running games, row 3 with no legal move."""
    from rein48_amd import VecGame
    from rein48_amd.evaluate import afterstate_policy
    env = VecGame(NMAX, device=DEV, seed=7)
    env.reset()
    greedy = afterstate_policy(None)
    for t in range(150):
        env.step(greedy(env.boards, t), auto_reset=True)
    boards = env.boards.cpu().numpy().copy()
    boards[I_NO_MOVES] = NO_MOVES
    boards.setflags(write=False)
    return boards


@functools.lru_cache(maxsize=None)
def nets(lay):
    """The net under test and its twin for the unfused steps (scratch zero between tests)."""
    from rein48_amd.ntuple import NTupleNet
    return NTupleNet(LAYOUTS[lay], device=DEV), NTupleNet(LAYOUTS[lay], device=DEV)


def fill(net, twin, seed, scale):
    g = torch.Generator(device=DEV).manual_seed(seed)
    net.tables.copy_(torch.randn(net.tables.shape, generator=g, device=DEV) * scale)
    twin.tables.copy_(net.tables)
    for x in (net, twin):                                       # whatever an earlier, failed test left behind
        x.acc.zero_()
        x.cnt.zero_()


def previous(n, seed, scale):
    """(prev_after int8 [n, 16], prev_value float32 [n], prev_done uint8 [n], prev_valid uint8 [n])."""
    rng = np.random.default_rng(seed)
    after = np.where(rng.random((n, 16)) < 0.6, rng.integers(1, 18, (n, 16)), 0).astype(np.int8)
    after[n // 2:] = after[rng.integers(0, max(1, n // 8), n - n // 2)]       # copies: entries hit many times
    value = (rng.normal(size=n) * 3 * scale).astype(np.float32)
    done = (rng.random(n) < 0.25).astype(np.uint8)
    valid = (rng.random(n) >= 0.25).astype(np.uint8)
    return after, value, done, valid


def torch_delta(prev_done, reward, value, prev_value):
    """NTupleTrainer.train_step's expression."""
    target = torch.where(prev_done != 0, torch.zeros_like(value), reward.float() + value)
    return torch.sub(target, prev_value)


def i32(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("lay,n,kind", CASES)
def test_td_act_equals_act_the_torch_delta_and_accumulate(lay, n, kind):
    net, twin = nets(lay)
    scale = SCALES[kind]
    fill(net, twin, 5, scale)
    boards = pool()[:n]
    p_after, p_value, p_done, p_valid = previous(n, 100 + n, scale)
    bt, pa, pv, pd, pk = T(boards), T(p_after), T(p_value), T(p_done), T(p_valid)
    # the unfused steps on the twin
    wa, wf, wv, wr, wl = twin.act(bt)
    wd = torch_delta(pd, wr, wv, pv)
    twin.accumulate(pa, wd, pk)
    # the fused kernel, every output a slice of a poisoned buffer
    ra, a = guarded(n, torch.int8, 0x55)
    rf, f = guarded(n, torch.int8, 0x55, row=16)
    rv, v = guarded(n, torch.float32, 7.5)
    rr, r = guarded(n, torch.int32, 0x55555555)
    rl, lg = guarded(n, torch.uint8, 0x55)
    rk, ok = guarded(n, torch.uint8, 0x55)
    rd, d = guarded(n, torch.float32, 7.5)
    out = net.td_act(bt, pa, pv, pd, pk, a, f, v, r, lg, ok, d)
    assert all(x is y for x, y in zip(out, (a, f, v, r, lg, ok, d)))
    assert torch.equal(a, wa) and torch.equal(f, wf) and torch.equal(i32(v), i32(wv))
    assert torch.equal(r, wr) and torch.equal(lg, wl)
    assert torch.equal(ok, (wl != 0).to(torch.uint8))
    assert torch.equal(i32(d), i32(wd))
    assert guard_ok(ra, n, 0x55) and guard_ok(rf, 16 * n, 0x55) and guard_ok(rv, n, 7.5) and guard_ok(rr, n, 0x55555555)
    assert guard_ok(rl, n, 0x55) and guard_ok(rk, n, 0x55) and guard_ok(rd, n, 7.5)
    assert torch.equal(net.acc, twin.acc) and torch.equal(net.cnt, twin.cnt)
    # rows that are not valid add nothing; the valid ones add 8m hits each
    assert int(net.cnt.sum()) == 8 * net.m * int(p_valid.sum())
    if n > I_NO_MOVES:
        assert int(lg[I_NO_MOVES]) == 0 and int(ok[I_NO_MOVES]) == 0 and float(v[I_NO_MOVES]) == 0.0
        assert torch.equal(f[I_NO_MOVES], bt[I_NO_MOVES])
        assert int(ok.sum()) == n - 1                           # every other game is running
    clamped = int((wd.abs() > 2.0 ** 20).sum())
    print("%s n=%d %s: %d of %d deltas beyond the clamp, %d rows done, %d not valid"
          % (lay, n, kind, clamped, n, int(p_done.sum()), n - int(p_valid.sum())))
    if n >= 63:
        assert (clamped > n // 2) if kind == "clamp" else (clamped == 0)
        assert 0 < int(p_done.sum()) < n and 0 < int(p_valid.sum()) < n
    # the update's second half leaves equal tables and zero scratch
    step = 0.25 / (8 * net.m)
    net.apply(pa, step, pk)
    twin.apply(pa, step, pk)
    assert torch.equal(i32(net.tables), i32(twin.tables))
    assert not bool(net.acc.any()) and not bool(net.cnt.any()) and not bool(twin.acc.any()) and not bool(twin.cnt.any())
    # inputs unchanged
    assert torch.equal(bt, T(boards)) and torch.equal(pa, T(p_after)) and torch.equal(i32(pv), i32(T(p_value)))
    assert torch.equal(pd, T(p_done)) and torch.equal(pk, T(p_valid))


@pytest.mark.parametrize("lay", ["lines-squares", "3x2"])
def test_no_valid_row_leaves_the_scratch_untouched_and_delta_is_still_written(lay):
    net, twin = nets(lay)
    fill(net, twin, 6, 37.0)
    n = 257
    p_after, p_value, p_done, _ = previous(n, 9, 37.0)
    bt, pa, pv, pd = T(pool()[:n]), T(p_after), T(p_value), T(p_done)
    none = torch.zeros(n, dtype=torch.uint8, device=DEV)
    before = net.tables.clone()
    _, _, v, r, _, _, d = net.td_act(bt, pa, pv, pd, none)
    assert not bool(net.acc.any()) and not bool(net.cnt.any())
    assert torch.equal(i32(d), i32(torch_delta(pd, r, v, pv)))
    assert torch.equal(i32(net.tables), i32(before))            # the kernel only reads the tables


def test_reward_and_delta_out_are_optional_and_aliasing_is_refused():
    from rein48_amd import _lib
    net, twin = nets("lines-squares")
    fill(net, twin, 7, 37.0)
    n = 63
    p_after, p_value, p_done, p_valid = previous(n, 11, 37.0)
    bt, pa, pv, pd, pk = T(pool()[:n]), T(p_after), T(p_value), T(p_done), T(p_valid)
    a, f, v, r, lg, ok, d = twin.td_act(bt, pa, pv, pd, pk)
    a2, f2, v2, lg2, ok2 = (torch.empty_like(x) for x in (a, f, v, lg, ok))
    _lib.check(_lib.load().r48_ntuple_td_act(_lib.ptr(bt), n, *net._lay(), _lib.ptr(net.tables), _lib.ptr(pa), _lib.ptr(pv),
                                             _lib.ptr(pd), _lib.ptr(pk), _lib.ptr(a2), _lib.ptr(f2), _lib.ptr(v2), None,
                                             _lib.ptr(lg2), _lib.ptr(ok2), None, _lib.ptr(net.acc), _lib.ptr(net.cnt), None))
    torch.cuda.synchronize()
    assert torch.equal(a2, a) and torch.equal(f2, f) and torch.equal(i32(v2), i32(v)) and torch.equal(lg2, lg)
    assert torch.equal(ok2, ok) and torch.equal(net.acc, twin.acc) and torch.equal(net.cnt, twin.cnt)
    for x in (net, twin):
        x.apply(pa, 0.0, pk)
        assert not bool(x.acc.any()) and not bool(x.cnt.any())
    # the wrapper passes the refusals on, and checks shapes itself
    for kw in (dict(after=pa), dict(value=pv), dict(valid=pk)):
        with pytest.raises(_lib.Rein48Error):
            net.td_act(bt, pa, pv, pd, pk, **kw)
    with pytest.raises(ValueError):
        net.td_act(bt, pa[:-1], pv, pd, pk)
    with pytest.raises(ValueError):
        net.td_act(bt, pa, pv[:-1], pd, pk)
    with pytest.raises(TypeError):
        net.td_act(bt, pa, pv, pd.float(), pk)
    assert not bool(net.acc.any()) and not bool(net.cnt.any())
