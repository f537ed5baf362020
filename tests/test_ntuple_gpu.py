"""The n-tuple network's kernels (r48_ntuple.hip) on the GPU against numpy restatements: value, the
fused one-ply search (act) against an argmax over the C oracle's four moves, and the two halves of
the per-entry-mean TD update.

Boards are test_moves_gpu.py's (crafted + random, exponents 0..17, many illegal moves, NO_MOVES,
EMPTY) with that module's cached oracle moves, shared and unchanged. Board counts 1, 63, 64, 65, 257
and 4099: a single lane, both sides of a wave boundary and a ragged tail across workgroups. The
restatement here transforms the board (np.rot90 / mirror) and indexes it cell by cell; the kernels
never transform a board, they read it through 8m placed tuples.
"""
import functools

import numpy as np
import pytest
import torch

from test_moves_gpu import NMAX, SIZES, T, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256

THREE = ((0, 1, 2), (5, 9, 10), (15, 3, 12))               # 3 x 3-tuple: whole tables are 3 * 4096 entries
LAYOUTS = {"lines-squares": "lines-squares", "3x3": THREE, "4x6": "4x6"}
CASES = [(lay, n) for lay in ("lines-squares", "3x3") for n in SIZES] + [("4x6", 257)]


@functools.lru_cache(maxsize=None)
def net_of(name):
    from rein48_amd.ntuple import NTupleNet
    return NTupleNet(LAYOUTS[name], device=DEV)


def entries(boards, cells):
    """int64 [n, m, 8]: the flat index into tables[m][16^L] of every hit, from eight explicit board
    transforms and a cell-by-cell index."""
    n, m, L = len(boards), len(cells), len(cells[0])
    g = np.minimum(np.asarray(boards).astype(np.int64), 15).reshape(n, 4, 4)
    out = np.empty((n, m, 8), np.int64)
    s = 0
    for k in range(4):
        r = np.rot90(g, k, axes=(1, 2))
        for f in (r, r[:, :, ::-1]):
            fb = f.reshape(n, 16)
            for t, tup in enumerate(cells):
                out[:, t, s] = t * 16 ** L + sum(fb[:, c] << (4 * j) for j, c in enumerate(tup))
            s += 1
    return out


def hit_values(net, boards):
    """float64 [n, 8m]: the table entries the boards hit (a torch gather, copied to the host)."""
    e = torch.from_numpy(entries(boards, net.cells).reshape(len(boards), -1)).to(DEV)
    return net.tables.flatten()[e].double().cpu().numpy()


def fill_int(net, seed, lo=-1024, hi=1024):
    g = torch.Generator(device=DEV).manual_seed(seed)
    net.tables.copy_(torch.randint(lo, hi + 1, net.tables.shape, generator=g, device=DEV).float())


def fill_float(net, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    net.tables.copy_(torch.randn(net.tables.shape, generator=g, device=DEV) * 37.0)


def guarded(n, dtype, fill, row=1):
    raw = torch.full((n * row + GUARD,), fill, dtype=dtype, device=DEV)
    return raw, (raw[:n * row].view(n, row) if row > 1 else raw[:n])


def guard_ok(raw, used, fill):
    return bool((raw[used:] == fill).all())


@pytest.mark.parametrize("lay,n", CASES)
def test_value_integer_tables_bit_equal_and_float_tables_within_bound(lay, n):
    net = net_of(lay)
    boards = reference()[0][:n]
    bt = T(boards)
    fill_int(net, 1)
    raw, out = guarded(n, torch.float32, 7.5)
    got = net.value(bt, out=out).cpu().numpy()
    want = hit_values(net, boards).sum(1)                    # integers <= 64 * 1024: exact in any order
    np.testing.assert_array_equal(got, want.astype(np.float32))
    assert guard_ok(raw, n, 7.5) and torch.equal(bt, T(boards))
    fill_float(net, 2)
    got = net.value(bt).double().cpu().numpy()
    h = hit_values(net, boards)
    bound = 8 * net.m * 2.0 ** -24 * np.abs(h).sum(1)
    err = np.abs(got - h.sum(1))
    print("value float: max err %.3g, min slack %.3g" % (err.max(), (bound - err).min()))
    assert (err <= bound).all()


def act_reference(net, n):
    """numpy argmax over the oracle's four moves with V from the hit entries (integer tables: exact)."""
    boards, after, reward, legal = reference()
    boards, after, reward, legal = boards[:n], after[:, :n], reward[:, :n], legal[:n]
    v4 = np.stack([hit_values(net, after[a]).sum(1) for a in range(4)])
    ok = ((legal[None, :] >> np.arange(4)[:, None]) & 1).astype(bool)
    score = np.where(ok, reward + v4, -np.inf)
    act = np.argmax(score, axis=0)                            # first maximiser = lowest code
    none = legal == 0
    act[none] = 0
    rows = np.arange(n)
    want_after = np.where(none[:, None], boards, after[act, rows])
    want_v = np.where(none, 0.0, v4[act, rows]).astype(np.float32)
    want_r = np.where(none, 0, reward[act, rows]).astype(np.int32)
    best = score.max(0)
    ties = int((((score == best) & ok).sum(0) > 1).sum())
    return act.astype(np.int8), want_after, want_v, want_r, legal, ties


@pytest.mark.parametrize("lay,n", CASES)
@pytest.mark.parametrize("spread", [1024, 1])
def test_act_integer_tables_equal_numpy_argmax(lay, n, spread):
    """Every output bit for bit, guard bytes intact. Tables in [-1, 1] plant ties between moves (the
    scores are small integers), and board 1 (ONE_TILE) ties all four moves under any tables: its
    afterstates are images of one another under the square's symmetries. Boards 0 and 2 (EMPTY,
    NO_MOVES) have no move."""
    net = net_of(lay)
    fill_int(net, 3 + spread, -spread, spread)
    bt = T(reference()[0][:n])
    ra, a = guarded(n, torch.int8, 0x55)
    rf, f = guarded(n, torch.int8, 0x55, row=16)
    rv, v = guarded(n, torch.float32, 7.5)
    rr, r = guarded(n, torch.int32, 0x55555555)
    rl, lg = guarded(n, torch.uint8, 0x55)
    net.act(bt, a, f, v, r, lg)
    wa, wf, wv, wr, wl, ties = act_reference(net, n)
    np.testing.assert_array_equal(a.cpu().numpy(), wa)
    np.testing.assert_array_equal(f.cpu().numpy(), wf)
    np.testing.assert_array_equal(v.cpu().numpy(), wv)
    np.testing.assert_array_equal(r.cpu().numpy(), wr)
    np.testing.assert_array_equal(lg.cpu().numpy(), wl)
    assert guard_ok(ra, n, 0x55) and guard_ok(rf, 16 * n, 0x55) and guard_ok(rv, n, 7.5)
    assert guard_ok(rr, n, 0x55555555) and guard_ok(rl, n, 0x55)
    print("boards with tied best moves: %d of %d" % (ties, n))
    if n >= 8:
        assert ties >= 1 and wa[1] == 0 and wl[1] == 15
        assert list(wa[[0, 2]]) == [0, 0] and list(wl[[0, 2]]) == [0, 0] and list(wv[[0, 2]]) == [0.0, 0.0]
    # nullable outputs: actions alone
    from rein48_amd import _lib
    only = torch.full((n,), 0x55, dtype=torch.int8, device=DEV)
    _lib.check(_lib.load().r48_ntuple_act(_lib.ptr(bt), n, *net._lay(), _lib.ptr(net.tables), _lib.ptr(only), None,
                                          None, None, None, None))
    assert torch.equal(only, a)


@pytest.mark.parametrize("lay,n", CASES)
def test_act_policies_and_value_consistency(lay, n):
    from rein48_amd.evaluate import afterstate_policy
    net = net_of(lay)
    bt = T(reference()[0][:n])
    # all-zero tables: the greedy-merge policy
    net.tables.zero_()
    assert torch.equal(net.act(bt)[0], afterstate_policy(None)(bt, 0))
    assert torch.equal(net.policy()(bt, 0), afterstate_policy(None)(bt, 0))
    # integer tables: the unfused path (afterstates -> value on 4n boards -> torch argmax) agrees
    fill_int(net, 11)
    assert torch.equal(net.act(bt)[0], afterstate_policy(net.value)(bt, 0))
    # float tables: the value act returns is value(after) bit for bit, and the action is legal
    fill_float(net, 12)
    a, after, v, r, lg = net.act(bt)
    has = lg != 0
    assert torch.equal(v.view(torch.int32)[has], net.value(after).view(torch.int32)[has])
    assert bool((v[~has] == 0).all())
    assert bool((((lg.int() >> a.int()) & 1) == 1)[has].all())


def guarded_net(name):
    """A fresh net whose tables / acc / cnt are slices of poisoned buffers (guard bytes behind each)."""
    from rein48_amd.ntuple import NTupleNet
    net = NTupleNet(LAYOUTS[name], device=DEV)
    k = net.tables.numel()
    raws = {}
    for attr, dtype, fill in (("tables", torch.float32, 7.5), ("acc", torch.int64, 0x5555), ("cnt", torch.int32, 0x5555)):
        raw = torch.full((k + GUARD,), fill, dtype=dtype, device=DEV)
        raw[:k] = 0
        raws[attr] = (raw, fill)
        setattr(net, attr, raw[:k].view(net.m, -1))
    net.guards_ok = lambda: all(guard_ok(raw, k, fill) for raw, fill in raws.values())
    return net


def update_inputs(n, seed):
    """boards with duplicates, deltas (some beyond the +-2^20 clamp), valid with zeros."""
    rng = np.random.default_rng(seed)
    boards = np.array(reference()[0][:n], copy=True)
    if n > 8:
        boards[n // 2:] = boards[rng.integers(0, max(1, n // 8), n - n // 2)]     # many copies of few boards
    delta = (rng.normal(size=n) * 300).astype(np.float32)
    delta[::7] = np.float32(3e6) * np.where(rng.random(len(delta[::7])) < 0.5, -1, 1)
    valid = (rng.random(n) < 0.8).astype(np.uint8)
    return boards, delta, valid


def sums_numpy(boards, delta, valid, cells):
    """(acc int64, cnt int64) over the flat tables, exactly as the contract states them."""
    size = len(cells) * 16 ** len(cells[0])
    q = np.rint(np.clip(delta, np.float32(-2.0 ** 20), np.float32(2.0 ** 20)).astype(np.float64) * 65536.0).astype(np.int64)
    e = entries(boards, cells).reshape(len(boards), -1)
    keep = valid != 0
    acc, cnt = np.zeros(size, np.int64), np.zeros(size, np.int64)
    np.add.at(cnt, e[keep].ravel(), 1)
    np.add.at(acc, e[keep].ravel(), np.repeat(q[keep], e.shape[1]))
    return acc, cnt


def apply_numpy(old, acc, cnt, step):
    """float32 restatement of apply: (increment, new tables)."""
    hit = cnt != 0
    mean = np.zeros(old.shape, np.float32)
    mean[hit] = (acc[hit].astype(np.float32) * np.float32(2.0 ** -16)) / cnt[hit].astype(np.float32)
    inc = (np.float32(step) * mean).astype(np.float32)
    return inc, (old + inc).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_accumulate_and_apply_equal_numpy(n):
    net = guarded_net("3x3")
    boards, delta, valid = update_inputs(n, n)
    fill_float(net, 5)
    old = net.tables.flatten().cpu().numpy()
    bt, dt, vt = T(boards), T(delta), T(valid)
    net.accumulate(bt, dt, vt)
    acc, cnt = sums_numpy(boards, delta, valid, net.cells)
    np.testing.assert_array_equal(net.acc.flatten().cpu().numpy(), acc)
    np.testing.assert_array_equal(net.cnt.flatten().cpu().numpy().astype(np.int64), cnt)
    assert torch.equal(net.tables.flatten().cpu(), torch.from_numpy(old))             # accumulate reads no table
    step = 0.25 / (8 * net.m)
    net.apply(bt, step, vt)
    got = net.tables.flatten().cpu().numpy()
    inc, want = apply_numpy(old, acc, cnt, step)
    # four fp32 roundings (int64 -> float, the scale is exact, the division, the product, the sum)
    # plus a possible fma contraction: 1e-6 relative on |old| + |increment|
    err = np.abs(got.astype(np.float64) - want)
    tol = 1e-6 * (np.abs(old) + np.abs(inc))
    print("apply: max err / tol %.3g" % (err / np.maximum(tol, 1e-30)).max())
    assert (err <= tol).all()
    np.testing.assert_array_equal(got[cnt == 0], old[cnt == 0])                       # untouched entries, bit for bit
    assert not bool(net.acc.any()) and not bool(net.cnt.any())                        # scratch is zero again
    assert net.guards_ok()
    # valid = None counts every board
    net.accumulate(bt, dt)
    acc, cnt = sums_numpy(boards, delta, np.ones(n, np.uint8), net.cells)
    np.testing.assert_array_equal(net.acc.flatten().cpu().numpy(), acc)
    np.testing.assert_array_equal(net.cnt.flatten().cpu().numpy().astype(np.int64), cnt)
    net.apply(bt, step)
    assert not bool(net.acc.any()) and not bool(net.cnt.any()) and net.guards_ok()


@pytest.mark.parametrize("lay", ["3x3", "lines-squares"])
def test_apply_is_bitwise_reproducible(lay):
    from rein48_amd.ntuple import NTupleNet
    boards, delta, valid = update_inputs(NMAX, 77)
    bt, dt, vt = T(boards), T(delta), T(valid)
    out = []
    for _ in range(2):
        net = NTupleNet(LAYOUTS[lay], device=DEV)
        fill_float(net, 6)
        for _ in range(3):
            net.td_update(bt, dt, 0.25, vt)
        out.append(net.tables.view(torch.int32).clone())
        assert not bool(net.acc.any()) and not bool(net.cnt.any())
    assert torch.equal(out[0], out[1])


@pytest.mark.parametrize("lay", ["3x3", "lines-squares", "4x6"])
def test_td_update_moves_value_to_the_target(lay):
    """n = 1, alpha = 1: V(s') lands on the target. The bound is the sum of: apply's 1e-6 * (|old| +
    |increment|) over the 8m hits, value's summation bound 8m * 2^-24 * sum |entries hit| (before and
    after), the fixed point's 2^-17 on the mean delta and the fp32 rounding of delta itself. 64 copies of the board move every entry
    exactly as one copy does: the sum and the count both scale by 64, a power of two, so the fp32
    conversion and division give the same bits."""
    from rein48_amd.ntuple import NTupleNet
    ref_boards = reference()[0]
    for row in (1, 7, 40, 100):                       # ONE_TILE (symmetric hits), HAS_17 (the clamp), two random
        board = np.array(ref_boards[row:row + 1], copy=True)
        net = net_of(lay)
        fill_float(net, 20 + row)
        bt = T(board)
        h0 = hit_values(net, board)
        v0 = float(net.value(bt)[0])
        target = 123.456
        delta = torch.tensor([target - v0], dtype=torch.float32, device=DEV)
        saved = net.tables.flatten()[torch.from_numpy(entries(board, net.cells).ravel()).to(DEV)].clone()
        net.td_update(bt, delta, 1.0)
        v1 = float(net.value(bt)[0])
        h1 = hit_values(net, board)
        inc = abs(target - v0) / (8 * net.m)
        bound = 1e-6 * (np.abs(h0).sum() + 8 * net.m * inc) + 8 * net.m * 2.0 ** -24 * (np.abs(h0).sum() + np.abs(h1).sum()) \
            + 2.0 ** -17 + 2.0 ** -24 * abs(target - v0)
        print("%s row %d: V %.6f -> %.6f, target %.6f, bound %.3g" % (lay, row, v0, v1, target, bound))
        assert abs(v1 - target) <= bound
        one = net.tables.flatten()[torch.from_numpy(entries(board, net.cells).ravel()).to(DEV)].clone()
        # put the entries back and repeat with 64 copies
        net.tables.flatten()[torch.from_numpy(entries(board, net.cells).ravel()).to(DEV)] = saved
        b64 = T(np.repeat(board, 64, axis=0))
        net.td_update(b64, delta.expand(64).contiguous(), 1.0)
        many = net.tables.flatten()[torch.from_numpy(entries(board, net.cells).ravel()).to(DEV)]
        assert torch.equal(one.view(torch.int32), many.view(torch.int32))
        assert not bool(net.cnt.any()) and not bool(net.acc.any())


def test_save_load_roundtrip(tmp_path):
    from rein48_amd.ntuple import NTupleNet
    net = net_of("lines-squares")
    fill_float(net, 31)
    net.save(str(tmp_path / "net.pt"))
    other = NTupleNet("lines-squares", device=DEV)
    other.load(str(tmp_path / "net.pt"))
    assert torch.equal(other.tables.view(torch.int32), net.tables.view(torch.int32))
    with pytest.raises(ValueError):
        NTupleNet(THREE, device=DEV).load(str(tmp_path / "net.pt"))
    with pytest.raises(ValueError):
        NTupleNet(((0, 1, 1),), device=DEV)
    with pytest.raises(ValueError):
        net.value(T(reference()[0][:4]).cpu())
