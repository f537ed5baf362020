"""The temporal-coherence kernels (k_nt_apply_tc, k_nt_tc_rate in r48_ntuple.hip) on the GPU against
float32 numpy restatements of the rule stated in r48_ntuple.h:

    rate = A[e] > 0 ? min(|E[e]| / A[e], 1) : 1;  tables[e] += step * (rate * mean);
    E[e] += mean;  A[e] += |mean|

Layouts and board counts are test_ntuple_gpu.py's (lines-squares and the 3 x 3-tuple layout at 1,
63, 64, 65, 257 and 4099 boards; 4x6 at 257), the boards its update_inputs (many copies of few
boards, a valid mask with both values). The three tables and the scratch are slices of poisoned
buffers. Restatements run over the entries hit only (the 4x6 tables have 2^26 entries); everything
else is compared on the device.
"""
import numpy as np
import pytest
import torch

from test_moves_gpu import NMAX, T, reference
from test_ntuple_gpu import CASES, GUARD, LAYOUTS, entries, fill_float, guard_ok, guarded, sums_numpy, update_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
TABLES = ("tables", "tc_e", "tc_a")


def guarded_tc_net(name, tc=True):
    """A fresh net whose tables / tc_e / tc_a / acc / cnt are slices of poisoned buffers."""
    from rein48_amd.ntuple import NTupleNet
    net = NTupleNet(LAYOUTS[name], device=DEV, tc=tc)
    k = net.tables.numel()
    raws = []
    for attr, dtype, fill in (("tables", torch.float32, 7.5), ("tc_e", torch.float32, 7.5), ("tc_a", torch.float32, 7.5),
                              ("acc", torch.int64, 0x5555), ("cnt", torch.int32, 0x5555)):
        if getattr(net, attr) is None:
            continue
        raw = torch.full((k + GUARD,), fill, dtype=dtype, device=DEV)
        raw[:k] = 0
        raws.append((raw, fill))
        setattr(net, attr, raw[:k].view(net.m, -1))
    net.guards_ok = lambda: all(guard_ok(raw, k, fill) for raw, fill in raws)
    return net


def inputs(n, seed):
    """update_inputs' boards and valid mask (the only board of n = 1 is valid), and three rounds of
    deltas: round 2 opposes round 1 board by board, so every entry hit carries |E| < A into round 3
    at the latest, round 3 is of mixed sign again. Some deltas lie beyond the +-2^20 clamp."""
    boards, d1, valid = update_inputs(n, seed)
    if n == 1:
        valid[:] = 1
    rng = np.random.default_rng(1000 + seed)
    d2 = (-np.sign(d1) * np.abs(rng.normal(size=n)) * 200).astype(F)
    d3 = (rng.normal(size=n) * 300).astype(F)
    return boards, valid, (d1, d2, d3)


def flat(net):
    return [getattr(net, k).flatten() for k in TABLES]


def rate_numpy(e, a):
    rate = np.ones(e.shape, F)
    pos = a > 0
    rate[pos] = np.minimum(np.abs(e[pos]) / a[pos], F(1))
    return rate


def tc_numpy(old, e, a, acc, cnt, step):
    """float32 restatement of apply_tc on entries that are all hit (cnt != 0)."""
    mean = (acc.astype(F) * F(2.0 ** -16)) / cnt.astype(F)
    rate = rate_numpy(e, a)
    inc = (F(step) * (rate * mean)).astype(F)
    return rate, mean, inc, (old + inc).astype(F), (e + mean).astype(F), (a + np.abs(mean)).astype(F)


def three_rounds(net, bt, vt, deltas, step):
    for d in deltas:
        net.accumulate(bt, T(d), vt)
        net.apply(bt, step, vt)


@pytest.mark.parametrize("lay,n", CASES)
def test_three_rounds_equal_the_numpy_restatement(lay, n):
    """tables, E and A within 1e-6 relative on |old| + |increment| (the existing apply test's bound:
    the rule adds one division and one multiply of a few ulp each), entries not hit bit-equal,
    scratch zero, guards intact, and entries with a rate below 1 among those updated."""
    net = guarded_tc_net(lay)
    fill_float(net, 5)
    boards, valid, deltas = inputs(n, n)
    assert n == 1 or (valid.any() and not valid.all())
    bt, vt = T(boards), T(valid)
    step = 1.0 / (8 * net.m)
    below, worst = 0, 0.0
    for rnd, delta in enumerate(deltas):
        acc, cnt = sums_numpy(boards, delta, valid, net.cells)
        idx = np.flatnonzero(cnt)
        # invalid boards contribute nothing: the entries hit are those of the valid boards
        np.testing.assert_array_equal(idx, np.unique(entries(boards[valid != 0], net.cells)))
        it = torch.from_numpy(idx).to(DEV)
        before = [x.clone() for x in flat(net)]
        old, e, a = (x[it].cpu().numpy() for x in before)
        net.accumulate(bt, T(delta), vt)
        net.apply(bt, step, vt)
        rate, mean, inc, *want = tc_numpy(old, e, a, acc[idx], cnt[idx], step)
        for name, x, b, w, o, d in zip(TABLES, flat(net), before, want, (old, e, a), (inc, mean, mean)):
            got = x[it].cpu().numpy()
            err, tol = np.abs(got.astype(np.float64) - w), 1e-6 * (np.abs(o) + np.abs(d))
            ratio = float((err / np.maximum(tol, 1e-30)).max())
            print("round %d %s: max err / tol %.3g" % (rnd, name, ratio))
            worst = max(worst, ratio)
            assert (err <= tol).all(), name
            patched = x.clone()
            patched[it] = b[it]
            assert torch.equal(patched.view(torch.int32), b.view(torch.int32)), name + ": an entry not hit changed"
        assert not bool(net.acc.any()) and not bool(net.cnt.any())
        assert net.guards_ok()
        if rnd == 0:
            assert (rate == 1).all()                       # no history yet
        else:
            below += int((rate < 1).sum())
    print("%s n=%d: %d entry updates ran at a rate below 1, worst err / tol %.3g" % (lay, n, below, worst))
    assert below > 0
    assert torch.equal(bt, T(boards)) and torch.equal(vt, T(valid))


@pytest.mark.parametrize("lay,n", CASES)
def test_without_history_tc_is_td(lay, n):
    """From zero E / A one apply_tc leaves the tables bit-identical to plain apply on a twin net."""
    boards, valid, deltas = inputs(n, 50 + n)
    bt, vt, dt = T(boards), T(valid), T(deltas[0])
    out = []
    for tc in (True, False):
        net = guarded_tc_net(lay, tc=tc)
        fill_float(net, 8)
        net.td_update(bt, dt, 0.25, vt)
        assert net.guards_ok() and not bool(net.acc.any()) and not bool(net.cnt.any())
        out.append(net.tables.view(torch.int32).clone())
        if tc:
            changed = int((net.tc_a != 0).sum())                 # a mean of exactly 0 leaves A at 0
            assert 0 < changed <= len(np.unique(entries(boards[valid != 0], net.cells)))
            assert torch.equal(net.tc_e.abs().view(torch.int32), net.tc_a.view(torch.int32))
        del net
    assert torch.equal(out[0], out[1])


@pytest.mark.parametrize("lay,n", [("lines-squares", NMAX), ("3x3", NMAX), ("4x6", 257)])
def test_three_rounds_are_reproducible_and_order_free(lay, n):
    """Run twice, and once with the batch permuted by one permutation in every round: the same bits
    in tables, E and A."""
    from rein48_amd.ntuple import NTupleNet
    boards, valid, deltas = inputs(n, 77)
    perm = np.random.default_rng(5).permutation(n)
    runs = []
    for order in (None, None, perm):
        b, v, ds = (boards, valid, deltas) if order is None else (boards[order], valid[order], [d[order] for d in deltas])
        net = NTupleNet(LAYOUTS[lay], device=DEV, tc=True)
        fill_float(net, 6)
        three_rounds(net, T(b), T(v), ds, 1.0 / (8 * net.m))
        assert not bool(net.acc.any()) and not bool(net.cnt.any())
        runs.append([x.view(torch.int32).clone() for x in flat(net)])
        del net
    assert bool((runs[0][2] != 0).any())
    for other in runs[1:]:
        for name, x, y in zip(TABLES, runs[0], other):
            assert torch.equal(x, y), name


@pytest.mark.parametrize("lay", ["3x3", "lines-squares", "4x6"])
def test_64_copies_move_the_tables_as_one_copy_does(lay):
    """The sum and the count both scale by 64, a power of two, so the mean has the same bits; three
    rounds, the second opposing the first, so the third runs at a rate below 1."""
    from rein48_amd.ntuple import NTupleNet
    ref_boards = reference()[0]
    for row in (1, 7, 40, 100):                       # ONE_TILE (symmetric hits), HAS_17 (the clamp), two random
        board = np.array(ref_boards[row:row + 1], copy=True)
        out = []
        for copies in (1, 64):
            net = NTupleNet(LAYOUTS[lay], device=DEV, tc=True)
            fill_float(net, 20 + row)
            bt = T(np.repeat(board, copies, axis=0))
            for d in (123.456, -77.25, 31.5):
                net.td_update(bt, torch.full((copies,), d, dtype=torch.float32, device=DEV), 1.0)
            it = torch.from_numpy(np.unique(entries(board, net.cells))).to(DEV)
            out.append([x[it].view(torch.int32).clone() for x in flat(net)])
            assert bool((net.tc_rate(bt) < 1).all())
            assert not bool(net.cnt.any()) and not bool(net.acc.any())
            del net
        for name, x, y in zip(TABLES, *out):
            assert torch.equal(x, y), name


@pytest.mark.parametrize("lay,n", CASES)
def test_tc_rate_equals_the_numpy_mean(lay, n):
    """Exactly 1 on a fresh net; after three rounds the mean of rate(e) over each board's hits within
    8m * 2^-24 * sum of the rates; E, A and the boards unmodified, guard bytes intact."""
    net = guarded_tc_net(lay)
    boards, valid, deltas = inputs(n, 200 + n)
    bt, vt = T(boards), T(valid)
    raw, out = guarded(n, torch.float32, 7.5)
    assert net.tc_rate(bt, out=out) is out
    assert bool((out == 1).all()) and guard_ok(raw, n, 7.5)
    fill_float(net, 9)
    three_rounds(net, bt, vt, deltas, 1.0 / (8 * net.m))
    before = [x.clone() for x in flat(net)]
    raw, out = guarded(n, torch.float32, 7.5)
    got = net.tc_rate(bt, out=out).double().cpu().numpy()
    e = torch.from_numpy(entries(boards, net.cells).reshape(n, -1)).to(DEV)
    rate = rate_numpy(before[1][e].cpu().numpy(), before[2][e].cpu().numpy()).astype(np.float64)
    want = rate.sum(1) / (8 * net.m)
    bound = 8 * net.m * 2.0 ** -24 * rate.sum(1)
    err = np.abs(got - want)
    print("tc_rate: mean %.4f, min %.4f, max err %.3g, min slack %.3g" % (want.mean(), want.min(), err.max(), (bound - err).min()))
    assert (err <= bound).all()
    assert want.min() < 1 and guard_ok(raw, n, 7.5) and net.guards_ok()
    for x, b in zip(flat(net), before):
        assert torch.equal(x.view(torch.int32), b.view(torch.int32))
    assert torch.equal(bt, T(boards))


def test_tc_state_roundtrip_and_refusals(tmp_path):
    from rein48_amd.ntuple import NTupleNet
    net = NTupleNet("lines-squares", device=DEV, tc=True)
    fill_float(net, 31)
    boards, valid, deltas = inputs(257, 3)
    three_rounds(net, T(boards), T(valid), deltas, 1.0 / (8 * net.m))
    net.save(str(tmp_path / "tc.pt"))
    other = NTupleNet("lines-squares", device=DEV, tc=True)
    other.load(str(tmp_path / "tc.pt"))
    for x, y in zip(flat(net), flat(other)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    plain = NTupleNet("lines-squares", device=DEV)
    assert plain.tc is False and plain.tc_e is None and sorted(plain.state_dict()) == ["cells", "tables"]
    plain.load(str(tmp_path / "tc.pt"))                    # a plain net takes the tables of a TC file
    assert torch.equal(plain.tables.view(torch.int32), net.tables.view(torch.int32))
    plain.save(str(tmp_path / "plain.pt"))
    with pytest.raises(ValueError):
        other.load(str(tmp_path / "plain.pt"))             # a TC net needs tc_e / tc_a
    with pytest.raises(ValueError):
        plain.tc_rate(T(boards))
