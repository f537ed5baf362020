"""The n-tuple network's ruled expectimax search (k_nt_search_ruled in r48_ntuple.hip,
NTupleNet.search_ruled): the depth of a board, 1..4 plies, is rule[its number of blanks].

Boards: the 3-ply test's pool of 34 (EMPTY, ONE_TILE, NO_MOVES at rows 0, 1, 2, random boards,
NEARLY_OVER, SYMMETRIC, CORNER_BLANK), plus SIXTEEN_TWOS where depth 4's second leaf register is
looked for, and a crowded pool of nine for the float64 tree four plies deep. One board per
workgroup of 16 waves (4 beyond 8,192 boards), so the counts 1, 2, 5 and 34 are single and many
workgroups. Layouts 3x3 and lines-squares, float and integer tables.

What is held bit for bit: a uniform rule of 1s, 2s or 3s against search(1), search(2) and search3;
a mixed rule's rows against the uniform runs at each row's own depth; two calls, a permuted batch,
batches of one and both workgroup sizes. What is held to a float64 bound: depth 4. Its outer level
is checked on the 3-ply kernel's own leaves (search3 on the root's children laid out in numpy), with
the outer level's bound alone -- the fma, the four butterfly levels, the division and the last add
on exact leaves -- so a wrong child, slot rank, spawn or leaf register shows; and the whole tree in
float64, independent of every search kernel, with the 3-ply test's bound (its module docstring)
carried up one more level: level() is applied three times instead of twice.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_moves_gpu import NO_MOVES, T
from test_ntuple_gpu import LAYOUTS, fill_float, fill_int, guard_ok, guarded, hit_values, net_of
from test_ntuple_search3_gpu import (CHUNK, CORNER_BLANK, COUNTS, I_CORNER, I_ONE, LAYS, N_POOL, TABLES, U, best_of,
                                     expand, level, moves_of, pool)
from test_ntuple_search_gpu import NEARLY_OVER

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SIXTEEN_TWOS = [1] * 16                                  # every move merges eight pairs and leaves eight blanks
KINDS = ("float", "int")


def rule_of(d3, d4=-1, base=2):
    from rein48_amd.ntuple import NTupleNet
    return NTupleNet.depth_rule(d3, d4, base)


MIXED = (4, 4, 4, 3, 3, 3, 3) + (2,) * 10                # depth_rule(6, 2), checked below


def blanks(boards):
    return (np.asarray(boards) == 0).sum(1)


def run(lay, kind, boards, rule):
    """search_ruled into poisoned guard buffers -> numpy (actions, q, legal, depth); the input is only read."""
    net = net_of(lay)
    TABLES[kind](net)
    n = len(boards)
    bt = T(boards)
    ra, a = guarded(n, torch.int8, 0x55)
    rq, q = guarded(n, torch.float32, 7.5, row=4)
    rl, lg = guarded(n, torch.uint8, 0x55)
    rd, d = guarded(n, torch.uint8, 0x55)
    out = net.search_ruled(bt, rule, a, q, lg, d)
    assert all(x is y for x, y in zip(out, (a, q, lg, d)))
    assert guard_ok(ra, n, 0x55) and guard_ok(rq, 4 * n, 7.5) and guard_ok(rl, n, 0x55) and guard_ok(rd, n, 0x55)
    assert torch.equal(bt, T(boards))
    return a.cpu().numpy(), q.cpu().numpy(), lg.cpu().numpy(), d.cpu().numpy()


@functools.lru_cache(maxsize=None)
def uniform(lay, kind, depth):
    """The whole pool under the rule of seventeen `depth`s, computed once and shared."""
    out = run(lay, kind, pool(), (depth,) * 17)
    for x in out:
        x.setflags(write=False)
    return out


def same(got, want, rows=slice(None)):
    """actions, q as int32 bits and legal of two runs agree (want taken at `rows`)."""
    return (np.array_equal(got[0], want[0][rows]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32)[rows])
            and np.array_equal(got[2], want[2][rows]))


def test_depth_rule_builds_the_mixed_rule():
    assert rule_of(6, 2) == MIXED and rule_of(16) == (3,) * 17 and rule_of(16, 16) == (4,) * 17


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", COUNTS)
def test_uniform_rules_equal_the_existing_searches(lay, kind, n):
    """Seventeen 1s, 2s and 3s reproduce search(1), search(2) and search3 bit for bit; depth_out is the constant."""
    net = net_of(lay)
    bt = T(pool()[:n])
    for depth in (1, 2, 3):
        got = run(lay, kind, pool()[:n], (depth,) * 17)                          # fills the tables
        want = net.search3(bt) if depth == 3 else net.search(bt, depth)
        want = tuple(x.cpu().numpy() for x in want)
        assert same(got, want), (lay, kind, n, depth)
        assert (got[3] == depth).all()


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_rule_rows_equal_the_uniform_runs_at_their_depth(lay, kind):
    got = run(lay, kind, pool(), MIXED)
    want_depth = np.array(MIXED, np.uint8)[blanks(pool())]
    np.testing.assert_array_equal(got[3], want_depth)
    assert {2, 3, 4} <= set(want_depth.tolist())                                 # all three depths occur in the pool
    for depth in (2, 3, 4):
        rows = np.flatnonzero(want_depth == depth)
        assert same(tuple(x[rows] for x in got[:3]), uniform(lay, kind, depth), rows), (lay, kind, depth)
    none = np.flatnonzero(got[2] == 0)                                           # no legal move: depth_out is still the rule's
    assert len(none) >= 2 and (got[0][none] == 0).all() and np.isneginf(got[1][none]).all()
    assert len(set(want_depth[none].tolist())) >= 2


@functools.lru_cache(maxsize=None)
def outer_tree():
    """pool() + SIXTEEN_TWOS: the root's moves and children, and how many children each child has."""
    boards = np.concatenate([pool(), np.array([SIXTEEN_TWOS], np.int8)])
    a1, r1, l1, ok1 = moves_of(boards)
    key1, kids1 = expand(a1, ok1)
    a2, _, l2, ok2 = moves_of(kids1)
    kids_of_child = 2 * (ok2[:, :, None] & (a2 == 0)).sum((0, 2))
    return dict(boards=boards, r1=r1, l1=l1, ok1=ok1, key1=key1, kids1=kids1, l2=l2, kids_of_child=kids_of_child)


def test_the_outer_pool_covers_the_ground():
    t = outer_tree()
    ki = t["key1"][0]
    kids_of_board = np.bincount(ki, minlength=N_POOL + 1)
    assert kids_of_board[I_ONE] == 120 and kids_of_board[I_CORNER] == 4          # the most and the fewest root children
    assert t["kids_of_child"][ki == N_POOL].max() > 64                           # nt_wave_q3's second leaf register
    assert (t["l2"] == 0).any()                                                  # a child without a move: leaf 0


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("kind", KINDS)
def test_depth4_outer_level_on_the_3ply_kernels_leaves(lay, kind):
    t = outer_tree()
    act, q, lg, d = run(lay, kind, t["boards"], (4,) * 17)
    assert same((act[:N_POOL], q[:N_POOL], lg[:N_POOL]), uniform(lay, kind, 4)) and (d == 4).all()
    net = net_of(lay)
    q3 = np.concatenate([net.search3(T(t["kids1"][k:k + CHUNK]))[1].cpu().numpy()
                         for k in range(0, len(t["kids1"]), CHUNK)]).astype(np.float64)
    leaf = np.where(t["l2"] != 0, q3.max(1), 0.0)
    Q, bound, _ = level(t["r1"], t["ok1"], t["key1"], leaf, np.zeros_like(leaf), np.abs(leaf))
    ok = t["ok1"].T
    np.testing.assert_array_equal(lg, t["l1"])
    np.testing.assert_array_equal(act, np.argmax(q, axis=1).astype(np.int8))     # first argmax of the returned q
    assert np.isneginf(q[~ok]).all() and np.isfinite(q[ok]).all()
    err = np.abs(q.astype(np.float64)[ok] - Q.T[ok])
    print("%s %s: worst err / outer bound %.3g" % (lay, kind, (err / bound.T[ok]).max()))
    assert (err <= bound.T[ok]).all()


@functools.lru_cache(maxsize=None)
def crowded():
    """NO_MOVES, NEARLY_OVER, CORNER_BLANK and six random boards of at most 2 blanks."""
    rng = np.random.default_rng(64)
    rand = rng.integers(1, 12, size=(6, 16)).astype(np.int8)                    # few equal neighbours: small trees
    for i, holes in enumerate((0, 1, 1, 2, 2, 2)):
        rand[i, rng.choice(16, holes, replace=False)] = 0
    boards = np.concatenate([np.array([NO_MOVES, NEARLY_OVER, CORNER_BLANK], np.int8), rand])
    boards.setflags(write=False)
    return boards


@functools.lru_cache(maxsize=None)
def crowded_tree():
    """The crowded pool's tree four plies deep, without values (only the legal last replies are kept, flat)."""
    t, boards = {}, crowded()
    for k in (1, 2, 3):
        a, t["r%d" % k], t["l%d" % k], t["ok%d" % k] = moves_of(boards)
        t["key%d" % k], boards = expand(a, t["ok%d" % k])
    a4, t["r4"], t["l4"], t["ok4"] = moves_of(boards)
    t["replies"] = a4[t["ok4"]]
    t["sizes"] = tuple(len(t["key%d" % k][0]) for k in (1, 2, 3)) + (len(t["replies"]),)
    return t


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("kind", KINDS)
def test_depth4_within_the_bound_of_the_float64_tree(lay, kind):
    t = crowded_tree()
    act, q, lg, d = run(lay, kind, crowded(), (4,) * 17)
    net = net_of(lay)
    v, habs = np.zeros(len(t["replies"])), np.zeros(len(t["replies"]))
    for k in range(0, len(v), CHUNK):                                            # never the whole tree at once
        h = hit_values(net, t["replies"][k:k + CHUNK])
        v[k:k + CHUNK], habs[k:k + CHUNK] = h.sum(1), np.abs(h).sum(1)
    ok4, r4 = t["ok4"], t["r4"]
    score, mag, err = np.full(ok4.shape, -np.inf), np.zeros(ok4.shape), np.zeros(ok4.shape)
    score[ok4] = r4[ok4] + v
    mag[ok4] = np.abs(r4[ok4]) + habs
    err[ok4] = 8 * net.m * U * habs + U * mag[ok4]
    best = best_of(score, err, mag, t["l4"])                                     # best_1 three spawns down
    for k in (3, 2, 1):
        Q, e, m = level(t["r%d" % k], t["ok%d" % k], t["key%d" % k], *best)
        best = best_of(Q, e, m, t["l%d" % k])
    Q, bound, ok, legal = Q.T, e.T, t["ok1"].T, t["l1"]
    n = len(legal)
    np.testing.assert_array_equal(lg, legal)
    assert (d == 4).all() and legal[0] == 0 and (legal[1:3] != 0).all()
    np.testing.assert_array_equal(act, np.argmax(q, axis=1).astype(np.int8))
    assert np.isneginf(q[~ok]).all() and np.isfinite(q[ok]).all()
    with np.errstate(invalid="ignore"):                                          # -inf - -inf of the illegal moves
        dq = np.abs(q.astype(np.float64) - Q)
    some = ok & (bound > 0)                                                      # bound 0: every child is game over, r = 0
    print("%s %s: children %d, grandchildren %d, great-grandchildren %d, legal replies %d; worst err / bound %.3g"
          % ((lay, kind) + t["sizes"] + ((dq[some] / bound[some]).max(),)))
    assert (dq[ok] <= bound[ok]).all(), np.argwhere(ok & ~(dq <= bound))[:5]
    rows, a = np.arange(n), act.astype(np.int64)                                 # the action maximises the float64 Q
    has = legal != 0
    assert ok[rows, a][has].all() and (act[~has] == 0).all()
    slack = bound[rows, a][:, None] + bound
    assert (np.where(ok, Q - slack, -np.inf)[has] <= Q[rows, a][has, None]).all()


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("rule", [(4,) * 17, MIXED], ids=["all4", "mixed"])
def test_bits_are_reproducible_and_do_not_depend_on_the_index(lay, rule):
    net = net_of(lay)
    fill_float(net, 61)
    boards = pool()
    first = net.search_ruled(T(boards), rule)
    again = net.search_ruled(T(boards), rule)
    assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32)
                           if y.dtype == torch.float32 else y) for x, y in zip(first, again))
    a, q, lg, d = first
    qi = q.view(torch.int32)
    perm = np.random.default_rng(6).permutation(len(boards))
    ap, qp, lp, dp = net.search_ruled(T(boards[perm]), rule)
    p = torch.from_numpy(perm).to(DEV)
    assert torch.equal(qp.view(torch.int32), qi[p]) and torch.equal(ap, a[p]) and torch.equal(lp, lg[p]) and torch.equal(dp, d[p])
    for i in (I_ONE, 7, 20, N_POOL - 3, I_CORNER):                               # alone in a batch of one
        a1, q1, l1, d1 = net.search_ruled(T(boards[i:i + 1]), rule)
        assert torch.equal(q1.view(torch.int32)[0], qi[i]) and a1[0] == a[i] and l1[0] == lg[i] and d1[0] == d[i]
    for n in (8192, 8193):                                                       # 16 waves share a board, beyond 8,192 four
        idx = np.arange(n) % N_POOL
        an, qn, ln, dn = net.search_ruled(T(boards[idx]), rule)
        p = torch.from_numpy(idx).to(DEV)
        assert torch.equal(qn.view(torch.int32), qi[p]) and torch.equal(an, a[p]) and torch.equal(ln, lg[p]) and torch.equal(dn, d[p])


def test_nullable_outputs_and_a_side_stream():
    from rein48_amd import _lib
    net = net_of("lines-squares")
    fill_int(net, 62, -8, 8)
    n = N_POOL
    bt = T(pool())
    a, q, lg, d = net.search_ruled(bt, MIXED)
    lib = _lib.load()
    rule = (C.c_uint8 * 17)(*MIXED)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for want_q, want_legal, want_depth in ((False, False, False), (True, False, False), (False, True, False),
                                           (False, False, True)):
        ra, a2 = guarded(n, torch.int8, 0x55)
        rq, q2 = guarded(n, torch.float32, 7.5, row=4)
        rl, l2 = guarded(n, torch.uint8, 0x55)
        rd, d2 = guarded(n, torch.uint8, 0x55)
        _lib.check(lib.r48_ntuple_search_ruled(_lib.ptr(bt), n, *net._lay(), _lib.ptr(net.tables), rule, _lib.ptr(a2),
                                               _lib.ptr(q2) if want_q else None, _lib.ptr(l2) if want_legal else None,
                                               _lib.ptr(d2) if want_depth else None, stream))
        assert torch.equal(a2, a) and guard_ok(ra, n, 0x55)
        assert torch.equal(q2.view(torch.int32), q.view(torch.int32)) if want_q else bool((rq == 7.5).all())
        assert torch.equal(l2, lg) if want_legal else bool((rl == 0x55).all())
        assert torch.equal(d2, d) if want_depth else bool((rd == 0x55).all())
        assert guard_ok(rq, 4 * n, 7.5) and guard_ok(rl, n, 0x55) and guard_ok(rd, n, 0x55) and torch.equal(bt, T(pool()))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        outs = net.search_ruled(bt, MIXED)
        finished = torch.cuda.Event()
        finished.record(side)
    finished.synchronize()
    assert torch.equal(outs[1].view(torch.int32), q.view(torch.int32))
    assert torch.equal(outs[0], a) and torch.equal(outs[2], lg) and torch.equal(outs[3], d)


def test_bad_rules_are_refused_by_the_wrapper():
    net = net_of("lines-squares")
    bt = T(pool()[:2])
    for bad in ((2,) * 16, (2,) * 18, (0,) + (2,) * 16, (2,) * 16 + (5,)):
        with pytest.raises(ValueError):
            net.search_ruled(bt, bad)
        with pytest.raises(ValueError):
            net.policy(rule=bad)


def test_policy_and_play_episodes_take_a_rule():
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    net = net_of("lines-squares")
    fill_float(net, 63)
    bt = T(pool())
    assert torch.equal(net.policy(rule=MIXED)(bt, 0), net.search_ruled(bt, MIXED)[0])
    assert torch.equal(net.policy(depth=3, rule=(2,) * 17)(bt, 0), net.search(bt, 2)[0])   # the rule decides
    assert not torch.equal(net.search_ruled(bt, MIXED)[0], net.search(bt, 2)[0])  # the depths do differ somewhere
    for depth in (0, 4):                                                          # without a rule nothing has changed
        with pytest.raises(ValueError):
            net.policy(depth=depth)
    tr = NTupleTrainer(NTupleConfig(n_boards=8, layout=LAYOUTS["3x3"]), device=DEV)
    tr.net.tables.copy_(net_of("3x3").tables)
    assert torch.equal(tr.policy(rule=MIXED)(bt, 0), tr.net.search_ruled(bt, MIXED)[0])
    with pytest.raises(ValueError):
        tr.policy(depth=4)
    ruled = net.play_episodes(64, seed=3, rule=(3,) * 17, return_scores=True)
    plain = net.play_episodes(64, seed=3, depth=3, return_scores=True)
    assert torch.equal(ruled.pop("scores"), plain.pop("scores")) and ruled == plain
    assert ruled["finished"] == 1.0
