"""The n-tuple network's 3-ply expectimax search (k_nt_search3 in r48_ntuple.hip, NTupleNet.search3)
on the GPU against a float64 restatement in numpy.

Boards: the first 31 of test_moves_gpu.py's reference() (EMPTY, ONE_TILE, NO_MOVES at rows 0, 1, 2,
HAS_17 at row 7, random boards after the crafted ones), NEARLY_OVER and SYMMETRIC of the depth-2
test, and CORNER_BLANK, 34 in all. The kernel holds one board per workgroup, whose 16 waves (4 in
batches beyond 8,192 boards, test_both_workgroup_sizes_give_the_same_bits) share the board's
children, so the board counts 1, 2, 5 and 34 are single and many workgroups. Layouts 3x3 and
lines-squares.

CORNER_BLANK stands where a board "whose only legal move leaves exactly one blank" (two children,
two idle waves) was asked for: there is no such board. A move that leaves one blank starts from a
full board with one merge, and then the opposite move merges the same pair; or from a board with
one blank and no merge, and then a tile of the blank's row and one of its column can each slide
into it, two moves. The fewest children a board with a legal move has is therefore four, and
CORNER_BLANK has exactly four (test_the_pool_covers_the_ground): 12 of its 16 waves have nothing
to do. Uneven deals are all over the random rows.

The restatement: one level of the tree is laid out in numpy (expand: every empty cell of every
legal afterstate filled with a 2 and with a 4), the moves come from the already-tested afterstates
kernel, the values from test_ntuple_gpu.hit_values(...).sum(1) in float64 over the legal replies of
the grandchildren, in chunks of at most 2^18 boards. One function (level) maps the children's best,
error and magnitude to the parents' Q, error and magnitude; depth 3 applies it twice. It is computed
once per (layout, tables) for the whole pool and shared by the counts.

The bound (u = 2^-24), the depth-2 test's, carried up the tree: a reply's score is within 8m u
sum |hits| + u (|r| + sum |hits|); a max is off by at most the largest error below it; one level
adds the cells' 9 err1 + err2, one rounding of the fma and four of the butterfly on partial sums
bounded by the sum M of the cells' magnitudes (5 u M), the division (u M / d) and the last add
(u (|r_a| + M / d)), times 1 + 2^-16 for the products of the level's chained roundings. Integer
tables do not make depth 3 exact (the inner division rounds), so they are held to the same bound.

Ties. With integer tables the values and the inner level's sums are exact, so boards that are
images of one another have bit-equal best_2. The outer sum adds the same leaves, now not integers,
in the butterfly's order, and that order is invariant under the relabelings c -> c ^ k of the cells
alone: moves that mirror each other (UP / DOWN are c ^ 12, LEFT / RIGHT c ^ 3) tie bit for bit,
moves that are each other's transpose add the same numbers in another order and may differ in the
last bit. So SYMMETRIC's and ONE_TILE's mirrored pairs are held to bit equality, and ONE_TILE's
four moves, which the depth-2 kernel ties bit for bit, are held to equal float64 Q and to the bound:
measured, its q is [69.21882, 69.21882, 69.21881, 69.21881] (3x3, integer tables), one ulp between
the pairs, and the first maximiser is then 0 or 2.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_moves_gpu import T, reference
from test_ntuple_gpu import LAYOUTS, fill_float, fill_int, guard_ok, guarded, hit_values, net_of
from test_ntuple_search_gpu import NEARLY_OVER, SYMMETRIC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CORNER_BLANK = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 3, 0]   # DOWN and RIGHT, one blank after each
N_REF = 31
I_ONE, I_NEARLY, I_SYM, I_CORNER = 1, N_REF, N_REF + 1, N_REF + 2
N_POOL = N_REF + 3
COUNTS = [1, 2, 5, N_POOL]
LAYS = ("3x3", "lines-squares")
CASES = [(lay, n) for lay in LAYS for n in COUNTS]
TABLES = {"int": lambda net: fill_int(net, 51, -8, 8), "float": lambda net: fill_float(net, 53)}
CHUNK = 2 ** 18
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def pool():
    boards = np.concatenate([reference()[0][:N_REF], np.array([NEARLY_OVER, SYMMETRIC, CORNER_BLANK], np.int8)])
    boards.setflags(write=False)
    return boards


def moves_of(boards):
    """after int8 [4, n, 16], reward [4, n], legal uint8 [n], ok bool [4, n] from the afterstates kernel,
    at most CHUNK boards per call."""
    from rein48_amd.moves import afterstates
    parts = [[x.cpu().numpy() for x in afterstates(T(boards[k:k + CHUNK]))] for k in range(0, len(boards), CHUNK)]
    after, reward, legal = (np.concatenate([p[j] for p in parts], axis=-1 if j == 2 else 1) for j in range(3))
    ok = ((legal[None, :] >> np.arange(4)[:, None]) & 1).astype(bool)
    return after, reward.astype(np.float64), legal, ok


def expand(after, ok):
    """The children of the legal afterstates: keys (parent i, move a, cell c, spawn e) [K] each, ordered by
    (a, i, c, e), and the boards int8 [K, 16]."""
    aa, ii, cc = np.nonzero(ok[:, :, None] & (after == 0))
    kids = np.repeat(after[aa, ii], 2, axis=0)
    ka, ki, kc = np.repeat(aa, 2), np.repeat(ii, 2), np.repeat(cc, 2)
    ke = np.tile(np.array([1, 2]), len(aa))
    kids[np.arange(len(kids)), kc] = ke
    return (ki, ka, kc, ke), kids


def best_of(Q, err, mag, legal):
    """best_k of boards from their moves' Q, error and magnitude [4, K] (illegal: -inf, 0, 0): a max is off
    by at most the largest error below it; a board without a move is worth exactly 0."""
    return np.where(legal != 0, Q.max(0), 0.0), err.max(0), mag.max(0)


def level(r, ok, key, best, err, mag):
    """One level of the search in float64: the children's best, error and magnitude [K] -> the parents' Q
    (-inf where illegal), error and magnitude [4, n], with the bound of the module docstring."""
    ki, ka, kc, ke = key
    n = r.shape[1]
    w = np.where(ke == 1, 9.0, 1.0)
    S, n_e, s_err, s_mag = np.zeros((4, n)), np.zeros((4, n), np.int64), np.zeros((4, n)), np.zeros((4, n))
    np.add.at(S, (ka, ki), w * best)
    np.add.at(n_e, (ka, ki), (ke == 1).astype(np.int64))
    np.add.at(s_err, (ka, ki), w * err)
    np.add.at(s_mag, (ka, ki), w * mag)
    assert (n_e[ok] >= 1).all()                                                 # a legal move leaves a blank
    d = np.where(ok, 10.0 * n_e, 1.0)
    Q = np.where(ok, r + S / d, -np.inf)
    bound = (s_err + U * s_mag + 4 * U * s_mag) / d + U * s_mag / d + U * (np.abs(r) + s_mag / d)
    return Q, np.where(ok, bound * (1 + 2.0 ** -16), 0.0), np.where(ok, np.abs(r) + s_mag / d, 0.0)


@functools.lru_cache(maxsize=None)
def tree():
    """The pool's search tree without values: the root's moves, its children, their moves, the
    grandchildren, their moves (only the legal replies' afterstates are kept, flat)."""
    a1, r1, l1, ok1 = moves_of(pool())
    key1, kids1 = expand(a1, ok1)
    a2, r2, l2, ok2 = moves_of(kids1)
    key2, kids2 = expand(a2, ok2)
    a3, r3, l3, ok3 = moves_of(kids2)
    return dict(r1=r1, l1=l1, ok1=ok1, key1=key1, kids1=kids1, r2=r2, l2=l2, ok2=ok2, key2=key2, n2=len(kids2),
                replies=a3[ok3], r3=r3, l3=l3, ok3=ok3)


@functools.lru_cache(maxsize=None)
def oracle(lay, kind):
    """float64 Q_3 [4, N_POOL], its bound, and the legal sets, under TABLES[kind]."""
    net = net_of(lay)
    TABLES[kind](net)
    t = tree()
    v, habs = np.zeros(len(t["replies"])), np.zeros(len(t["replies"]))
    for k in range(0, len(v), CHUNK):                                           # never the whole tree at once
        h = hit_values(net, t["replies"][k:k + CHUNK])
        v[k:k + CHUNK], habs[k:k + CHUNK] = h.sum(1), np.abs(h).sum(1)
    ok3, r3 = t["ok3"], t["r3"]
    score, mag, err = np.full(ok3.shape, -np.inf), np.zeros(ok3.shape), np.zeros(ok3.shape)
    score[ok3] = r3[ok3] + v
    mag[ok3] = np.abs(r3[ok3]) + habs
    err[ok3] = 8 * net.m * U * habs + U * mag[ok3]
    b1 = best_of(score, err, mag, t["l3"])                                      # best_1 of the grandchildren
    Q2, e2, m2 = level(t["r2"], t["ok2"], t["key2"], *b1)
    b2 = best_of(Q2, e2, m2, t["l2"])                                           # best_2 of the children
    Q3, e3, _ = level(t["r1"], t["ok1"], t["key1"], *b2)
    return dict(Q=Q3, bound=e3, ok=t["ok1"], legal=t["l1"])


def run(lay, kind, n):
    net = net_of(lay)
    TABLES[kind](net)
    bt = T(pool()[:n])
    ra, a = guarded(n, torch.int8, 0x55)
    rq, q = guarded(n, torch.float32, 7.5, row=4)
    rl, lg = guarded(n, torch.uint8, 0x55)
    net.search3(bt, a, q, lg)
    assert guard_ok(ra, n, 0x55) and guard_ok(rq, 4 * n, 7.5) and guard_ok(rl, n, 0x55)
    assert torch.equal(bt, T(pool()[:n]))                                        # the input is only read
    return a.cpu().numpy(), q.cpu().numpy(), lg.cpu().numpy()


def test_the_pool_covers_the_ground():
    t = tree()
    ki1, ki2 = t["key1"][0], t["key2"][0]
    kids_of_board = np.bincount(ki1, minlength=N_POOL)
    kids_of_child = np.bincount(ki2, minlength=len(t["kids1"]))
    print("children %d, grandchildren %d, legal replies %d" % (len(ki1), len(ki2), len(t["replies"])))
    assert kids_of_board[I_ONE] == 120 and kids_of_board.max() == 120           # more than 64 root children
    assert kids_of_child.max() > 64                                             # a child with more than 64 of its own
    assert (t["l2"] == 0).sum() >= 1 and (t["l3"] == 0).sum() >= 1              # game over one and two spawns down
    assert list(t["l1"][[0, 2]]) == [0, 0] and t["l1"][I_ONE] == 15              # boards with no legal move
    has = t["l1"] != 0
    assert kids_of_board[has].min() == 4 and kids_of_board[I_CORNER] == 4        # the fewest there can be
    assert (kids_of_board[has] % 4 != 0).any()                                   # the waves' shares differ
    assert t["l1"][I_CORNER] == 0b1010 and t["l1"][I_NEARLY] & 12 == 12
    assert len(t["replies"]) > CHUNK or len(ki2) <= CHUNK                        # what the chunks are for


@pytest.mark.parametrize("lay,n", CASES)
@pytest.mark.parametrize("kind", ["float", "int"])
def test_q_within_the_bound_of_the_float64_tree(lay, n, kind):
    o = oracle(lay, kind)
    act, q, lg = run(lay, kind, n)
    Q, ok, bound, legal = o["Q"][:, :n].T, o["ok"][:, :n].T, o["bound"][:, :n].T, o["legal"][:n]
    np.testing.assert_array_equal(lg, legal)
    np.testing.assert_array_equal(act, np.argmax(q, axis=1).astype(np.int8))    # first argmax of the returned q
    assert np.isneginf(q[~ok]).all() and np.isfinite(q[ok]).all()
    with np.errstate(invalid="ignore"):                                          # -inf - -inf of the illegal moves
        err = np.abs(q.astype(np.float64) - Q)
    if ok.any():
        print("%s %s n=%d: worst err / bound %.3g" % (lay, kind, n, (err[ok] / bound[ok]).max()))
    assert (err[ok] <= bound[ok]).all(), (np.argwhere(ok & ~(err <= bound))[:5])
    # the action maximises the float64 Q up to the two bounds involved
    rows, a = np.arange(n), act.astype(np.int64)
    has = legal != 0
    assert ok[rows, a][has].all() and (act[~has] == 0).all()
    slack = bound[rows, a][:, None] + bound
    assert (np.where(ok, Q - slack, -np.inf)[has] <= Q[rows, a][has, None]).all()
    none = np.flatnonzero(~has)
    assert np.isneginf(q[none]).all() and (lg[none] == 0).all()
    # Ties (module docstring): integer tables, mirrored moves bit for bit, ONE_TILE's four in float64
    for i in (I_ONE, I_SYM):
        if kind == "int" and n > i:
            s = q[i].view(np.int32)
            assert s[0] == s[1] and s[2] == s[3] and act[i] in (0, 2)
    if n > I_ONE:
        assert lg[I_ONE] == 15 and np.ptp(Q[I_ONE]) <= 1e-9 * (np.abs(Q[I_ONE]).max() + 1)


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("kind", ["float", "int"])
def test_outer_level_on_the_depth2_kernels_leaves(lay, kind):
    """The root's children laid out by numpy, their leaves from the existing kernel (the max of
    search(children, 2)'s q, 0 where the child has no move: fp32 numbers the 3-ply kernel must hold
    bit for bit), combined in float64. The bound is the outer level's alone -- the fma, the 4
    butterfly levels, the division and the last add on exact leaves -- so a wrong child, slot rank
    or spawn shows, which the whole tree's looser bound could hide."""
    t = tree()
    act, q, lg = run(lay, kind, N_POOL)
    net = net_of(lay)
    q2 = np.concatenate([net.search(T(t["kids1"][k:k + CHUNK]), 2)[1].cpu().numpy()
                         for k in range(0, len(t["kids1"]), CHUNK)]).astype(np.float64)
    leaf = np.where(t["l2"] != 0, q2.max(1), 0.0)
    Q, bound, _ = level(t["r1"], t["ok1"], t["key1"], leaf, np.zeros_like(leaf), np.abs(leaf))
    ok = t["ok1"].T
    err = np.abs(q.astype(np.float64)[ok] - Q.T[ok])
    print("%s %s: worst err / outer bound %.3g" % (lay, kind, (err / bound.T[ok]).max()))
    assert (err <= bound.T[ok]).all()


@pytest.mark.parametrize("lay", LAYS)
def test_q_bits_are_reproducible_and_do_not_depend_on_the_index(lay):
    net = net_of(lay)
    fill_float(net, 55)
    boards = pool()
    bt = T(boards)
    a, q, lg = net.search3(bt)
    a2, q2, lg2 = net.search3(bt)
    assert torch.equal(q.view(torch.int32), q2.view(torch.int32)) and torch.equal(a, a2) and torch.equal(lg, lg2)
    perm = np.random.default_rng(5).permutation(len(boards))
    ap, qp, lp = net.search3(T(boards[perm]))
    p = torch.from_numpy(perm).to(DEV)
    assert torch.equal(qp.view(torch.int32), q.view(torch.int32)[p]) and torch.equal(ap, a[p]) and torch.equal(lp, lg[p])
    for i in (I_ONE, 7, 20, I_NEARLY, I_CORNER):                                 # alone in a batch of one
        a1, q1, l1 = net.search3(T(boards[i:i + 1]))
        assert torch.equal(q1.view(torch.int32)[0], q.view(torch.int32)[i]) and a1[0] == a[i] and l1[0] == lg[i]


@pytest.mark.parametrize("lay", LAYS)
def test_both_workgroup_sizes_give_the_same_bits(lay):
    """Up to 8,192 boards (kSearch3SmallBatch in r48_ntuple.hip) a board's children are shared by 16
    waves, beyond by 4: the pool repeated to 8,192 and to 8,193 boards gives the pool's bits."""
    net = net_of(lay)
    fill_float(net, 58)
    a, q, lg = net.search3(T(pool()))
    for n in (8192, 8193):
        idx = np.arange(n) % N_POOL
        an, qn, ln = net.search3(T(pool()[idx]))
        p = torch.from_numpy(idx).to(DEV)
        assert torch.equal(qn.view(torch.int32), q.view(torch.int32)[p]) and torch.equal(an, a[p]) and torch.equal(ln, lg[p])


def test_nullable_outputs():
    from rein48_amd import _lib
    net = net_of("lines-squares")
    fill_int(net, 56, -8, 8)
    n = N_POOL
    bt = T(pool())
    a, q, lg = net.search3(bt)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for want_q, want_legal in ((False, False), (True, False), (False, True)):
        ra, a2 = guarded(n, torch.int8, 0x55)
        rq, q2 = guarded(n, torch.float32, 7.5, row=4)
        rl, l2 = guarded(n, torch.uint8, 0x55)
        _lib.check(lib.r48_ntuple_search3(_lib.ptr(bt), n, *net._lay(), _lib.ptr(net.tables), _lib.ptr(a2),
                                          _lib.ptr(q2) if want_q else None, _lib.ptr(l2) if want_legal else None, stream))
        assert torch.equal(a2, a) and guard_ok(ra, n, 0x55)
        assert torch.equal(q2.view(torch.int32), q.view(torch.int32)) if want_q else bool((rq == 7.5).all())
        assert torch.equal(l2, lg) if want_legal else bool((rl == 0x55).all())
        assert guard_ok(rq, 4 * n, 7.5) and guard_ok(rl, n, 0x55) and torch.equal(bt, T(pool()))


def test_policy_depth():
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    net = net_of("lines-squares")
    fill_float(net, 57)
    bt = T(pool())
    assert torch.equal(net.policy(depth=3)(bt, 0), net.search3(bt)[0])
    assert not torch.equal(net.search3(bt)[0], net.search(bt)[0])                # the two depths do differ somewhere
    for depth in (0, 4):
        with pytest.raises(ValueError):
            net.policy(depth=depth)
    with pytest.raises(ValueError):
        net.search(bt, depth=3)                                                  # the third ply has its own method
    tr = NTupleTrainer(NTupleConfig(n_boards=8, layout=LAYOUTS["3x3"]), device=DEV)
    tr.net.tables.copy_(net_of("3x3").tables)
    assert torch.equal(tr.policy(depth=3)(bt, 0), tr.net.search3(bt)[0])
    with pytest.raises(ValueError):
        tr.policy(depth=4)
