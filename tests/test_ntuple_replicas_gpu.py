"""Replicas on the GPU (k_nt_td_act_rep, k_nt_apply_rep, k_nt_apply_tc_rep in r48_ntuple.hip;
NTupleReplicaTrainer), every comparison bitwise.

Kernels: one call on [replicas * per] boards against one call of the unstaged parent
(r48_ntuple_td_act, r48_ntuple_apply, r48_ntuple_apply_tc) per replica on that replica's slices.
Shapes: two tables of 256 entries (every entry hot) at 3 x 37 boards -- lanes 37 and 74 cut waves 0
and 1 -- with replicas 0 and 1 holding the same boards and afterstates under different prev_value, so
a lost offset mixes their sums; lines-squares at 3 x 37; one 6-tuple at 2 x 65 (a base of 2^24, and
the boundary at lane 65 in wave 1); 5 x 1 (every lane its own replica); 1 x 130 (the plain entry
points). Boards have at least half their cells empty, two per replica have no legal move, about a
quarter of the rows are done and about a quarter not valid.

Trainer: replica r against a solo NTupleTrainer(fused=True) with alpha_r on VecGame(per, seed,
board_offset=per * r), in the middle and after the last of K = 400 steps, for TD and for TC."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from rein48_amd import _lib
from rein48_amd._lib import check, ptr
from test_moves_gpu import NO_MOVES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TWO_BY_TWO = ((0, 1), (5, 6))
SHAPES = {
    "2x2-3x37": (TWO_BY_TWO, 3, 37),
    "lines-squares-3x37": ("lines-squares", 3, 37),
    "1x6-2x65": (((0, 1, 2, 3, 4, 5),), 2, 65),
    "2x2-5x1": (TWO_BY_TWO, 5, 1),
    "2x2-1x130": (TWO_BY_TWO, 1, 130),
}
OUTS = (("actions", torch.int8, ()), ("after", torch.int8, (16,)), ("value", torch.float32, ()),
        ("reward", torch.int32, ()), ("legal", torch.uint8, ()), ("valid", torch.uint8, ()), ("delta", torch.float32, ()))
K = 400


def steps_for(R):
    return (0.0, 0.125, 0.03125) if R == 3 else tuple(0.125 / (1 << k) for k in range(R))


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return torch.equal(bits(a), bits(b))


class Side:
    """One side of a comparison: the tables, scratch, TC sums and td_act's outputs, all full size."""

    def __init__(self, cells, R, n, tables, tc_e, tc_a):
        m, size = len(cells), 16 ** len(cells[0])
        self.tables, self.tc_e, self.tc_a = tables.clone(), tc_e.clone(), tc_a.clone()
        self.acc = torch.zeros((R, m, size), dtype=torch.int64, device=DEV)
        self.cnt = torch.zeros((R, m, size), dtype=torch.int32, device=DEV)
        self.out = {name: torch.zeros((n,) + tail, dtype=dtype, device=DEV) for name, dtype, tail in OUTS}


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """The host half of one shape's inputs: (boards, prev_after, prev_value, prev_done, prev_valid) as
    numpy arrays. At least half the random cells are empty; boards without a legal move are put in
    afterwards."""
    _, R, per = SHAPES[shape]
    n = R * per
    rng = np.random.default_rng(sorted(SHAPES).index(shape))
    boards = np.where(rng.random((n, 16)) < 0.35, rng.integers(1, 8, (n, 16)), 0).astype(np.int8)
    after = np.where(rng.random((n, 16)) < 0.35, rng.integers(1, 12, (n, 16)), 0).astype(np.int8)
    assert (boards == 0).mean() >= 0.5 and (after == 0).mean() >= 0.5
    value = (rng.normal(size=n) * 40).astype(np.float32)
    done = (rng.random(n) < 0.25).astype(np.uint8)
    valid = (rng.random(n) >= 0.25).astype(np.uint8)
    if per >= 8:
        for r in range(R):                                      # two boards per replica have no legal move
            boards[r * per + 3] = NO_MOVES
            boards[r * per + per - 1] = NO_MOVES
        assert all(0 < x[r * per:(r + 1) * per].sum() < per for x in (done, valid) for r in range(R))
    else:
        boards[n - 1] = NO_MOVES
        valid[0], valid[1] = 1, 0
    if shape.startswith("2x2-3"):                               # replicas 0 and 1: the same rows, other values
        for x in (boards, after, done, valid):
            x[per:2 * per] = x[:per]
        assert not np.array_equal(value[per:2 * per], value[:per])
    return boards, after, value, done, valid


@functools.lru_cache(maxsize=None)
def case(shape):
    """The inputs of one shape (device tensors, read-only by convention) and the layout's C arrays."""
    from rein48_amd.ntuple import layout_cells
    layout, R, per = SHAPES[shape]
    cells = layout_cells(layout)
    boards, after, value, done, valid = inputs(shape)
    g = torch.Generator(device=DEV).manual_seed(11)
    shape3 = (R, len(cells), 16 ** len(cells[0]))
    tables = torch.randn(shape3, generator=g, device=DEV) * 37.0
    tc_e = torch.randn(shape3, generator=g, device=DEV) * 5.0
    tc_a = tc_e.abs() + torch.rand(shape3, generator=g, device=DEV) * 5.0
    flat = [c for t in cells for c in t]
    dev = lambda a: torch.from_numpy(a.copy()).to(DEV)
    return dict(cells=cells, c_cells=(C.c_uint8 * len(flat))(*flat), m=len(cells), L=len(cells[0]), R=R, per=per,
                n=R * per, boards=dev(boards), prev_after=dev(after), prev_value=dev(value), prev_done=dev(done),
                prev_valid=dev(valid), tables=tables, tc_e=tc_e, tc_a=tc_a,
                steps=torch.tensor(steps_for(R), dtype=torch.float32, device=DEV))


def td_act_both(c, got, want):
    lib, R, per, n = _lib.load(), c["R"], c["per"], c["n"]
    lay = (c["c_cells"], c["m"], c["L"])
    check(lib.r48_ntuple_td_act_replicas(
        ptr(c["boards"]), n, R, *lay, ptr(got.tables), ptr(c["prev_after"]), ptr(c["prev_value"]), ptr(c["prev_done"]),
        ptr(c["prev_valid"]), *(ptr(got.out[name]) for name, _, _ in OUTS), ptr(got.acc), ptr(got.cnt), None))
    for r in range(R):
        s = slice(r * per, (r + 1) * per)
        check(lib.r48_ntuple_td_act(
            ptr(c["boards"][s]), per, *lay, ptr(want.tables[r]), ptr(c["prev_after"][s]), ptr(c["prev_value"][s]),
            ptr(c["prev_done"][s]), ptr(c["prev_valid"][s]), *(ptr(want.out[name][s]) for name, _, _ in OUTS),
            ptr(want.acc[r]), ptr(want.cnt[r]), None))


def apply_both(c, got, want, tc):
    lib, R, per, n = _lib.load(), c["R"], c["per"], c["n"]
    lay = (c["c_cells"], c["m"], c["L"])
    if tc:
        check(lib.r48_ntuple_apply_tc_replicas(ptr(c["prev_after"]), n, R, ptr(c["prev_valid"]), *lay, ptr(c["steps"]),
                                               ptr(got.tables), ptr(got.tc_e), ptr(got.tc_a), ptr(got.acc), ptr(got.cnt),
                                               None))
    else:
        check(lib.r48_ntuple_apply_replicas(ptr(c["prev_after"]), n, R, ptr(c["prev_valid"]), *lay, ptr(c["steps"]),
                                            ptr(got.tables), ptr(got.acc), ptr(got.cnt), None))
    for r in range(R):
        s = slice(r * per, (r + 1) * per)
        step = steps_for(R)[r]
        if tc:
            check(lib.r48_ntuple_apply_tc(ptr(c["prev_after"][s]), per, ptr(c["prev_valid"][s]), *lay, step,
                                          ptr(want.tables[r]), ptr(want.tc_e[r]), ptr(want.tc_a[r]), ptr(want.acc[r]),
                                          ptr(want.cnt[r]), None))
        else:
            check(lib.r48_ntuple_apply(ptr(c["prev_after"][s]), per, ptr(c["prev_valid"][s]), *lay, step,
                                       ptr(want.tables[r]), ptr(want.acc[r]), ptr(want.cnt[r]), None))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_kernels_equal_the_parents_on_each_replica(shape):
    c = case(shape)
    got, want = (Side(c["cells"], c["R"], c["n"], c["tables"], c["tc_e"], c["tc_a"]) for _ in range(2))
    # td_act: the seven outputs, acc and cnt
    td_act_both(c, got, want)
    for name, _, _ in OUTS:
        assert same(got.out[name], want.out[name]), name
    assert same(got.acc, want.acc) and same(got.cnt, want.cnt)
    assert same(got.tables, c["tables"])                        # only read
    hit = want.cnt.view(c["R"], -1).ne(0).any(dim=1)
    assert bool(hit.all()) or c["per"] == 1                     # every replica accumulated something
    assert bool(got.out["legal"].eq(0).any()) and bool(got.out["legal"].ne(0).any())
    # apply: the tables; the scratch is zero again
    apply_both(c, got, want, tc=False)
    assert same(got.tables, want.tables)
    for side in (got, want):
        assert not bool(side.acc.any()) and not bool(side.cnt.any())
    for r, step in enumerate(steps_for(c["R"])):
        moved = not same(got.tables[r], c["tables"][r])
        assert moved == (step != 0.0 and bool(hit[r])), (r, step)
    # apply_tc from the updated tables and random E, A >= |E|: tables, tc_e, tc_a
    td_act_both(c, got, want)
    assert same(got.acc, want.acc) and same(got.cnt, want.cnt)
    apply_both(c, got, want, tc=True)
    assert same(got.tables, want.tables) and same(got.tc_e, want.tc_e) and same(got.tc_a, want.tc_a)
    assert not same(got.tc_e, c["tc_e"]) and not same(got.tc_a, c["tc_a"])
    for side in (got, want):
        assert not bool(side.acc.any()) and not bool(side.cnt.any())


# ---- the trainer ---------------------------------------------------------------------------------

def solo(per, r, alpha, seed, tc, layout="lines-squares"):
    from rein48_amd import VecGame
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    tr = NTupleTrainer(NTupleConfig(n_boards=per, layout=layout, alpha=alpha, seed=seed, tc=tc, fused=True), device=DEV)
    tr.env = VecGame(per, device=DEV, seed=seed, board_offset=per * r)
    tr.env.reset()
    return tr


def assert_replica_is_solo(tr, r, one):
    rep = lambda t: tr.replica(t, r)
    assert same(tr.tables[r], one.net.tables), r
    assert same(rep(tr.prev_after), one.prev_after) and same(rep(tr.prev_value), one.prev_value), r
    assert same(rep(tr.prev_done), one.prev_done) and same(rep(tr.prev_valid), one.prev_valid), r
    assert same(rep(tr.env.boards), one.env.boards), r
    for name in ("actions", "reward", "legal", "delta"):
        assert same(rep(getattr(tr, name)), getattr(one, name)), (r, name)
    if tr.tc:
        assert same(tr.tc_e[r], one.net.tc_e) and same(tr.tc_a[r], one.net.tc_a), r
    assert tr.updates == one.updates and tr.env.counters == one.env.counters
    assert not bool(tr.acc.any()) and not bool(tr.cnt.any())


@pytest.mark.parametrize("mode,alphas", [("td", (0.25, 0.1, 0.0)), ("tc", (1.0, 0.5, 1.0))])
def test_every_replica_is_its_solo_trainer(mode, alphas):
    """K = 400 steps of lines-squares at 3 x 37 boards, checked after step 200 and step 400. Every
    replica sees auto-resets on the way (asserted): greedy-merge games last on the order of 10^2 moves."""
    from rein48_amd.ntuple import NTupleConfig, NTupleReplicaTrainer
    per, seed, tc = 37, 5, mode == "tc"
    tr = NTupleReplicaTrainer(NTupleConfig(n_boards=per, layout="lines-squares", seed=seed, tc=tc, alpha=7.0), 3,
                              alphas=alphas, device=DEV)
    solos = [solo(per, r, alphas[r], seed, tc) for r in range(3)]
    ended = torch.zeros(3 * per, dtype=torch.int32, device=DEV)
    for half in range(2):
        for _ in range(K // 2):
            tr.train_step()
            ended += tr.prev_done
        for one in solos:
            one.train_steps(K // 2)
        for r, one in enumerate(solos):
            assert_replica_is_solo(tr, r, one)
    per_replica = ended.view(3, per).sum(dim=1).tolist()
    print("%s: episodes ended per replica in %d steps: %r" % (mode, K, per_replica))
    assert min(per_replica) >= 1
    assert tr.updates == K
    for r, alpha in enumerate(alphas):
        assert bool(tr.tables[r].any()) == (alpha != 0.0), r
    if tc:
        assert bool(tr.tc_a.any())


def test_one_replica_is_the_fused_trainer():
    """replicas = 1 at 130 boards, 100 steps: NTupleTrainer(fused=True) in every tensor."""
    from rein48_amd.ntuple import NTupleConfig, NTupleReplicaTrainer, NTupleTrainer
    cfg = dict(n_boards=130, layout="lines-squares", alpha=0.25, seed=3)
    tr = NTupleReplicaTrainer(NTupleConfig(**cfg), 1, device=DEV)
    one = NTupleTrainer(NTupleConfig(fused=True, **cfg), device=DEV)
    tr.train_steps(100)
    one.train_steps(100)
    assert_replica_is_solo(tr, 0, one)
    assert same(tr.after, one.after) and same(tr.value, one.value) and same(tr.valid, one.valid)
    assert bool(tr.tables.any())


@functools.lru_cache(maxsize=None)
def trained():
    from rein48_amd.ntuple import NTupleConfig, NTupleReplicaTrainer
    tr = NTupleReplicaTrainer(NTupleConfig(n_boards=37, layout="lines-squares", seed=1, tc=True, alpha=1.0), 3, device=DEV)
    tr.train_steps(100)
    return tr


def test_net_is_a_view_and_a_whole_net(tmp_path):
    from rein48_amd.ntuple import NTupleNet
    tr = trained()
    net = tr.net(1)
    for name in ("tables", "acc", "cnt", "tc_e", "tc_a"):
        whole, part = getattr(tr, name), getattr(net, name)
        assert part.data_ptr() == whole.data_ptr() + whole[0].numel() * whole.element_size(), name
        assert part.shape == whole.shape[1:]
    assert net.tc and net.cuts == () and net.own is None
    boards = tr.env.boards.clone()
    fresh = NTupleNet("lines-squares", device=DEV)
    fresh.tables.copy_(tr.tables[1])
    assert same(net.value(boards), fresh.value(boards))
    assert bool(net.value(boards).any())
    assert not same(net.value(boards), tr.net(0).value(boards))
    assert same(net.act(boards)[0], fresh.act(boards)[0])
    # what it saves, a solo net loads
    path = str(tmp_path / "replica.pt")
    net.save(path)
    loaded = NTupleNet("lines-squares", device=DEV, tc=True)
    loaded.load(path)
    assert same(loaded.tables, tr.tables[1]) and same(loaded.tc_e, tr.tc_e[1]) and same(loaded.tc_a, tr.tc_a[1])
    st = net.state_dict()
    assert sorted(st) == ["cells", "tables", "tc_a", "tc_e"]
    # a write through the view lands in the trainer's tensor
    keep = tr.tables[1].clone()
    net.tables.zero_()
    assert not bool(tr.tables[1].any()) and bool(tr.tables[0].any())
    tr.tables[1].copy_(keep)
    with pytest.raises(ValueError):
        tr.net(3)


def test_a_replica_plays_whole_episodes():
    tr = trained()
    before = tr.tables.clone()
    out = tr.net(2).play_episodes(64, max_steps=200)
    assert out["boards"] == 64 and out["mean_score"] > 0 and out["mean_length"] > 0
    assert out == tr.net(2).play_episodes(64, max_steps=200)
    policy = tr.policy(2)
    assert same(policy(tr.env.boards, 0), tr.net(2).act(tr.env.boards.contiguous())[0])
    assert same(tr.tables, before)


def test_refusals():
    from rein48_amd.ntuple import NTupleConfig, NTupleReplicaTrainer
    with pytest.raises(ValueError):
        NTupleReplicaTrainer(NTupleConfig(n_boards=8, layout="lines-squares", stages=(8,)), 2, device=DEV)
    with pytest.raises(ValueError):
        NTupleReplicaTrainer(NTupleConfig(n_boards=8, layout="lines-squares", carousel=(8,)), 2, device=DEV)
    for alphas in ((0.1,), (0.1, 0.2, 0.3), ()):
        with pytest.raises(ValueError):
            NTupleReplicaTrainer(NTupleConfig(n_boards=8, layout="lines-squares"), 2, alphas=alphas, device=DEV)
    for replicas in (0, 65):
        with pytest.raises(ValueError):
            NTupleReplicaTrainer(NTupleConfig(n_boards=8, layout="lines-squares"), replicas, device=DEV)
