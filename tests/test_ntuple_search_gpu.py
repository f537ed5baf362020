"""The n-tuple network's expectimax search (k_nt_search in r48_ntuple.hip, NTupleNet.search) on the
GPU against a float64 restatement in numpy.

Boards: the first 257 of test_moves_gpu.py's reference() (exponents up to 17, EMPTY, ONE_TILE,
NO_MOVES at rows 0, 1, 2) and two crafted boards appended, 259 in all. The kernel holds one board
per wave and four waves per workgroup, so the board counts 1, 3, 4, 5, 65, 257 and 259 are a single
wave, both sides of the workgroup boundary and many workgroups with a ragged tail. Layouts 3x3 and
lines-squares at every count, 4x6 at 65.

The restatement: the children of every legal afterstate (each empty cell filled with a 2 and with a
4) are laid out once in numpy, their four moves come from the already-tested afterstates kernel,
the values from test_ntuple_gpu.hit_values(...).sum(1) in float64; leaves, S_a and Q are float64
numpy. It is computed once per (layout, tables) for the whole pool and shared by the counts.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_moves_gpu import T, reference
from test_ntuple_gpu import LAYOUTS, fill_float, fill_int, guard_ok, guarded, hit_values, net_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# LEFT and RIGHT each leave one empty cell; after LEFT a spawned 2 there ends the game
# (test_crafted_boards_do_what_they_are_for checks that with the restatement)
NEARLY_OVER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 2, 1, 3]
SYMMETRIC = [3, 7, 7, 3, 7, 1, 1, 7, 7, 1, 1, 7, 3, 7, 7, 3]    # opposite moves mirror each other
N_REF = 257
I_NEARLY, I_SYM = N_REF, N_REF + 1
N_POOL = N_REF + 2
COUNTS = [1, 3, 4, 5, 65, 257, N_POOL]
CASES = [(lay, n) for lay in ("3x3", "lines-squares") for n in COUNTS] + [("4x6", 65)]
TABLES = {"int8": lambda net: fill_int(net, 41, -8, 8), "int1": lambda net: fill_int(net, 42, -1, 1),
          "float": lambda net: fill_float(net, 43)}
EXACT = 2.0 ** 24


@functools.lru_cache(maxsize=None)
def pool():
    boards = np.concatenate([reference()[0][:N_REF], np.array([NEARLY_OVER, SYMMETRIC], np.int8)])
    boards.setflags(write=False)
    return boards


def pool_size(lay):
    return 65 if lay == "4x6" else N_POOL


@functools.lru_cache(maxsize=None)
def tree(n):
    """The search tree of pool()[:n] without values: (after1 [4, n, 16], r1 [4, n], legal1 [n], child
    keys i, a, c, e [K] each, after2 [4, K, 16], r2 [4, K], legal2 [K])."""
    from rein48_amd.moves import afterstates
    boards = pool()[:n]
    a1, r1, l1 = (x.cpu().numpy() for x in afterstates(T(boards)))
    ok = ((l1[None, :] >> np.arange(4)[:, None]) & 1).astype(bool)              # [4, n]
    aa, ii, cc = np.nonzero(ok[:, :, None] & (a1 == 0))                         # legal move, empty cell
    kids = np.repeat(a1[aa, ii], 2, axis=0)                                     # e = 1, 2 for each
    ka, ki, kc = np.repeat(aa, 2), np.repeat(ii, 2), np.repeat(cc, 2)
    ke = np.tile(np.array([1, 2]), len(aa))
    kids[np.arange(len(kids)), kc] = ke
    a2, r2, l2 = (x.cpu().numpy() for x in afterstates(T(kids)))
    return a1, r1, l1, (ki, ka, kc, ke), a2, r2, l2


@functools.lru_cache(maxsize=None)
def oracle(lay, kind):
    """float64 Q and what the bounds need, for pool()[:pool_size(lay)] under TABLES[kind]."""
    net = net_of(lay)
    TABLES[kind](net)
    n = pool_size(lay)
    a1, r1, l1, (ki, ka, kc, ke), a2, r2, l2 = tree(n)
    K = len(ki)
    h = hit_values(net, a2.reshape(4 * K, 16))                                  # [4K, 8m]
    v2, habs = h.sum(1).reshape(4, K), np.abs(h).sum(1).reshape(4, K)
    ok2 = ((l2[None, :] >> np.arange(4)[:, None]) & 1).astype(bool)
    score = np.where(ok2, r2 + v2, -np.inf)
    leaf = np.where(l2 != 0, score.max(0), 0.0)                                 # game over: 0
    u = 2.0 ** -24
    mag = np.where(ok2, np.abs(r2) + habs, 0.0)                                 # bounds |score| and its partial sums
    # one score: the value's summation bound 8m u sum |hits| and the add; the max of perturbed
    # scores moves by at most the largest perturbation
    leaf_err = np.where(ok2, 8 * net.m * u * habs + u * mag, 0.0).max(0)
    leaf_mag = mag.max(0)
    w = np.where(ke == 1, 9.0, 1.0)
    S, n_e, absx = np.zeros((4, n)), np.zeros((4, n), np.int64), np.zeros((4, n))
    s_err, s_mag = np.zeros((4, n)), np.zeros((4, n))
    np.add.at(S, (ka, ki), w * leaf)
    np.add.at(n_e, (ka, ki), (ke == 1).astype(np.int64))
    np.add.at(s_err, (ka, ki), w * leaf_err)
    np.add.at(s_mag, (ka, ki), w * leaf_mag)
    # sum over the cells of |9 leaf1 + leaf2|: bounds every partial sum of the cell reduction
    x = np.zeros((4, n, 16))
    np.add.at(x, (ka, ki, kc), w * leaf)
    absx = np.abs(x).sum(2)
    ok1 = ((l1[None, :] >> np.arange(4)[:, None]) & 1).astype(bool)
    d = np.where(ok1, 10.0 * n_e, 1.0)
    assert (n_e[ok1] >= 1).all()                                                # a legal move leaves a blank
    Q = np.where(ok1, r1 + S / d, -np.inf)
    # float tables: the fma of a cell (u on 9 |l1| + |l2|), 4 levels of the reduction (u each on
    # the partial sums), the division and the last add; 1 + 2^-16 covers products of roundings
    fbound = (s_err + u * s_mag + 4 * u * s_mag) / d + u * s_mag / d + u * (np.abs(r1) + s_mag / d)
    fbound = np.where(ok1, fbound * (1 + 2.0 ** -16), 0.0)
    # integer tables: exact up to the division and the last add
    ibound = np.where(ok1, 2 * 2.0 ** -23 * (np.abs(r1) + np.abs(S) / d), 0.0)
    big_leaf = np.zeros(n)
    np.maximum.at(big_leaf, ki, np.abs(leaf))
    exact = (big_leaf < EXACT) & (absx.max(0) < EXACT)                          # per board
    return dict(Q=Q, ok=ok1, legal=l1, S=S, n_e=n_e, r=r1, ibound=ibound, fbound=fbound, exact=exact, leaf=leaf,
                l2=l2, key=(ki, ka, kc, ke))


def run(lay, kind, n, depth=2):
    net = net_of(lay)
    TABLES[kind](net)
    bt = T(pool()[:n])
    ra, a = guarded(n, torch.int8, 0x55)
    rq, q = guarded(n, torch.float32, 7.5, row=4)
    rl, lg = guarded(n, torch.uint8, 0x55)
    net.search(bt, depth, a, q, lg)
    assert guard_ok(ra, n, 0x55) and guard_ok(rq, 4 * n, 7.5) and guard_ok(rl, n, 0x55)
    assert torch.equal(bt, T(pool()[:n]))                                        # the input is only read
    return a.cpu().numpy(), q.cpu().numpy(), lg.cpu().numpy()


def test_crafted_boards_do_what_they_are_for():
    o = oracle("lines-squares", "int8")
    ki, ka, kc, ke = o["key"]
    assert o["legal"][I_NEARLY] & 12 == 12
    assert o["n_e"][2, I_NEARLY] == 1 and o["n_e"][3, I_NEARLY] == 1
    # after LEFT the 2 spawned in the one blank ends the game and the 4 does not; after RIGHT neither
    # spawn does (column 2 still merges)
    over = {a: (o["l2"][(ki == I_NEARLY) & (ka == a)] == 0).tolist() for a in (2, 3)}
    assert over == {2: [True, False], 3: [False, False]}
    assert (o["leaf"][o["l2"] == 0] == 0).all() and (o["l2"] == 0).sum() >= 1   # game-over children, leaf = 0
    assert (o["n_e"] == 15).sum() >= 1 and (o["n_e"][:, 1] == 15).all()         # ONE_TILE: 15 blanks after any move
    assert list(o["legal"][[0, 2]]) == [0, 0] and o["legal"][1] == 15


@pytest.mark.parametrize("lay,n", CASES)
@pytest.mark.parametrize("kind", ["int8", "int1"])
def test_depth2_integer_tables(lay, n, kind):
    """Integer tables of spread 8 and 1: every leaf and S_a is an integer, so below 2^24 the fp32
    sums are exact in any order and only the division and the last add round:
    |q - Q64| <= 2 * 2^-23 * (|r_a| + |S_a| / (10 |E|)). Boards on which a leaf or the sum of the
    cells' |terms| reaches 2^24 are left out of the q and action comparisons -- their legal sets
    are still checked. That is row 7 alone, HAS_17, whose merge reward of 2^18 times 150 passes 2^24."""
    o = oracle(lay, kind)
    act, q, lg = run(lay, kind, n)
    Q, ok, bound, keep = o["Q"][:, :n].T, o["ok"][:, :n].T, o["ibound"][:, :n].T, o["exact"][:n]
    print("%s %s n=%d: %d boards left out (a sum reaches 2^24)" % (lay, kind, n, (~keep).sum()))
    assert np.flatnonzero(~o["exact"]).tolist() == [7]                          # HAS_17 alone (reward 2^18)
    np.testing.assert_array_equal(lg, o["legal"][:n])
    np.testing.assert_array_equal(act, np.argmax(q, axis=1).astype(np.int8))    # first argmax of the returned q
    assert np.isneginf(q[~ok]).all() and np.isfinite(q[ok]).all()
    with np.errstate(invalid="ignore"):                                          # -inf - -inf of the illegal moves
        err = np.abs(q.astype(np.float64) - Q)
    bad = ok & keep[:, None] & ~(err <= bound)
    ratio = (err / np.maximum(bound, 1e-300))[ok & keep[:, None] & (bound > 0)]
    print("worst err / bound %.3g" % (ratio.max() if ratio.size else 0.0))
    assert not bad.any(), (np.argwhere(bad)[:5], q[bad][:5], Q[bad][:5])
    rows = np.arange(n)
    has = keep & (o["legal"][:n] != 0)
    chosen, best = Q[rows, act.astype(np.int64)], Q.max(1)
    assert (chosen[has] >= best[has] - bound[rows, act.astype(np.int64)][has]).all()
    assert (act[o["legal"][:n] == 0] == 0).all()
    if n >= 3:
        assert act[1] == 0 and lg[1] == 15 and len(set(q[1].view(np.int32).tolist())) == 1   # ONE_TILE: four bit-equal q
        assert list(act[[0, 2]]) == [0, 0] and list(lg[[0, 2]]) == [0, 0] and np.isneginf(q[[0, 2]]).all()
    if n > I_SYM:
        s = q[I_SYM].view(np.int32)
        assert s[0] == s[1] and s[2] == s[3]                                     # mirrored moves tie bit for bit
    if kind == "int1":
        full = o["Q"].T
        tied = ((full == full.max(1, keepdims=True)) & o["ok"].T).sum(1) > 1
        assert (tied & o["exact"]).sum() >= 1                                    # exact ties exist in the pool


@pytest.mark.parametrize("lay,n", CASES)
def test_depth2_float_tables_within_bound(lay, n):
    """Random float tables. With u = 2^-24, per legal reply of a child: the value is within
    8m u sum |hits| (test_value_...within_bound's bound) and the add of the reward rounds once on at
    most |r| + sum |hits|; the leaf, a max, is off by at most the largest of those. A cell's term
    fmaf(9, leaf1, leaf2) carries 9 err1 + err2 and one rounding on at most 9 mag1 + mag2. The 16
    slots are reduced in the 4 levels of the butterfly, each rounding once on partial sums
    bounded by the sum M of the cells' magnitudes: 4 u M. The division rounds once (u M / d, d = 10
    |E| exact) and the last add once (u (|r_a| + M / d)). The whole is scaled by 1 + 2^-16 for the
    products of the ~60 chained roundings."""
    o = oracle(lay, "float")
    act, q, lg = run(lay, "float", n)
    Q, ok, bound = o["Q"][:, :n].T, o["ok"][:, :n].T, o["fbound"][:, :n].T
    np.testing.assert_array_equal(lg, o["legal"][:n])
    np.testing.assert_array_equal(act, np.argmax(q, axis=1).astype(np.int8))
    assert np.isneginf(q[~ok]).all()
    with np.errstate(invalid="ignore"):                                          # -inf - -inf of the illegal moves
        err = np.abs(q.astype(np.float64) - Q)
    if ok.any():
        print("%s n=%d float: worst err / bound %.3g" % (lay, n, (err[ok] / bound[ok]).max()))
    assert (err[ok] <= bound[ok]).all()


@pytest.mark.parametrize("lay,n", CASES)
def test_depth1_equals_act_and_afterstates_plus_value(lay, n):
    from rein48_amd.moves import afterstates
    net = net_of(lay)
    fill_float(net, 44)
    bt = T(pool()[:n])
    act, q, lg = net.search(bt, depth=1)
    a0, _, _, _, l0 = net.act(bt)
    assert torch.equal(act, a0) and torch.equal(lg, l0)
    after, reward, legal = afterstates(bt)
    want = reward.float() + net.value(after.view(4 * n, 16)).view(4, n)          # one fp32 add, as the kernel's
    ok = ((legal[None, :].int() >> torch.arange(4, device=DEV)[:, None]) & 1) != 0
    want = torch.where(ok, want, torch.full_like(want, float("-inf"))).T.contiguous()
    assert torch.equal(q.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("lay", ["3x3", "lines-squares"])
def test_q_bits_are_reproducible_and_do_not_depend_on_the_index(lay):
    net = net_of(lay)
    fill_float(net, 45)
    boards = pool()
    bt = T(boards)
    a, q, lg = net.search(bt)
    a2, q2, lg2 = net.search(bt)
    assert torch.equal(q.view(torch.int32), q2.view(torch.int32)) and torch.equal(a, a2) and torch.equal(lg, lg2)
    perm = np.random.default_rng(5).permutation(len(boards))
    ap, qp, lp = net.search(T(boards[perm]))
    p = torch.from_numpy(perm).to(DEV)
    assert torch.equal(qp.view(torch.int32), q.view(torch.int32)[p]) and torch.equal(ap, a[p]) and torch.equal(lp, lg[p])
    # alone in a batch of one, at another n
    for i in (1, 7, 100, I_NEARLY):
        a1, q1, l1 = net.search(T(boards[i:i + 1]))
        assert torch.equal(q1.view(torch.int32)[0], q.view(torch.int32)[i]) and a1[0] == a[i] and l1[0] == lg[i]


@pytest.mark.parametrize("depth", [1, 2])
def test_nullable_outputs(depth):
    from rein48_amd import _lib
    net = net_of("lines-squares")
    fill_int(net, 46, -8, 8)
    n = 65
    bt = T(pool()[:n])
    a, q, lg = net.search(bt, depth)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for want_q, want_legal in ((False, False), (True, False), (False, True)):
        ra, a2 = guarded(n, torch.int8, 0x55)
        rq, q2 = guarded(n, torch.float32, 7.5, row=4)
        rl, l2 = guarded(n, torch.uint8, 0x55)
        _lib.check(lib.r48_ntuple_search(_lib.ptr(bt), n, *net._lay(), _lib.ptr(net.tables), depth, _lib.ptr(a2),
                                         _lib.ptr(q2) if want_q else None, _lib.ptr(l2) if want_legal else None, stream))
        assert torch.equal(a2, a) and guard_ok(ra, n, 0x55)
        assert torch.equal(q2.view(torch.int32), q.view(torch.int32)) if want_q else bool((rq == 7.5).all())
        assert torch.equal(l2, lg) if want_legal else bool((rl == 0x55).all())
        assert guard_ok(rq, 4 * n, 7.5) and guard_ok(rl, n, 0x55) and torch.equal(bt, T(pool()[:n]))
    with pytest.raises(ValueError):
        net.search(bt, depth=3)
    with pytest.raises(ValueError):
        net.policy(depth=0)


def test_policy_depth():
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    net = net_of("lines-squares")
    fill_float(net, 47)
    bt = T(pool())
    assert torch.equal(net.policy(depth=2)(bt, 0), net.search(bt)[0])
    assert torch.equal(net.policy()(bt, 0), net.act(bt)[0])
    assert torch.equal(net.policy(depth=1)(bt, 0), net.act(bt)[0])
    assert not torch.equal(net.search(bt)[0], net.act(bt)[0])                    # the two depths do differ somewhere
    tr = NTupleTrainer(NTupleConfig(n_boards=8, layout=LAYOUTS["3x3"]), device=DEV)
    tr.net.tables.copy_(net_of("3x3").tables)
    assert torch.equal(tr.policy(depth=2)(bt, 0), tr.net.search(bt)[0])
    assert torch.equal(tr.policy()(bt, 0), tr.net.act(bt)[0])
