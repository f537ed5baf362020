"""Carousel shaping (r48_ntuple_carousel: k_nt_carousel_restart, then k_nt_carousel_record) on the GPU
against a numpy restatement of the contract in r48_ntuple.h, everything compared bitwise: boards,
pool, pool_has, seen, turn and starts.

The restatement decides every board from a copy of the state before the call: the donor from
update_refs.philox4x32_10 over {gid lo, gid hi, ctr, 0xCA70} under the seed, the stage from a numpy
max over the cells clamped to 15.

  single calls   n in {1, 63, 64, 65, 257} (below, at and above a wave, more than one workgroup), cuts
                 (4,) and (3, 4, 6), gid0 0 and 2^32 + 5; boards whose largest tile is at every cut - 1,
                 at every cut, at 15 and at 17; done all 0, all 1 and random; pools empty, full and half
                 full; seen and turn anywhere in 0 .. S - 1; with and without starts
  chain          50 calls with random done and boards that move on between the calls, equal to the
                 restatement after every call
  reproducible   the same call twice, on two streams, gives the same bits. The result is a function
                 of n and gid0, not of the launch: the halves of a batch, run as batches of their own
                 with gid0 moved along, equal the restatement for THEIR n and gid0; with every pool
                 slot full they restart in the same stages as the whole batch and from the same board
                 exactly where the half's donor is the whole batch's donor slot
"""
import ctypes as C

import numpy as np
import pytest
import torch

import update_refs as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAG = 0xCA70
SEED = 0x0123456789ABCDEF
NAMES = ("boards", "pool", "pool_has", "seen", "turn", "starts")


def stage_np(board, cuts):
    top = int(np.minimum(board.astype(np.int64), 15).max())
    return sum(1 for c in cuts if top >= c)


def donors(n, seed, gid0, ctr):
    gid = np.arange(n, dtype=np.uint64) + np.uint64(gid0)
    c = np.stack([gid & np.uint64(0xFFFFFFFF), gid >> np.uint64(32), np.full(n, ctr, np.uint64), np.full(n, TAG, np.uint64)], 1)
    w0 = U.philox4x32_10(c, (seed & 0xFFFFFFFF, seed >> 32))[:, 0].astype(np.uint64)
    return ((w0 * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def carousel_numpy(st, done, cuts, seed, gid0, ctr):
    """One call on a dict of numpy arrays (NAMES) -> the new dict."""
    old = {k: v.copy() for k, v in st.items()}
    new = {k: v.copy() for k, v in st.items()}
    n, S = len(old["boards"]), len(cuts) + 1
    j = donors(n, seed, gid0, ctr)
    for i in range(n):
        b = old["boards"][i]
        if done[i]:
            t = (int(old["turn"][i]) + 1) % S
            if t > 0:
                if old["pool_has"][t - 1, j[i]]:
                    b = old["pool"][t - 1, j[i]]
                else:
                    t = 0
            new["boards"][i] = b
            new["turn"][i] = t
            new["seen"][i] = stage_np(b, cuts)
            new["starts"][t] += np.uint64(1)
        else:
            s = stage_np(b, cuts)
            if s > old["seen"][i]:
                new["pool"][s - 1, i] = b
                new["pool_has"][s - 1, i] = 1
                new["seen"][i] = s
    return new


def to_gpu(st):
    return {k: torch.from_numpy(v.view(np.int64) if k == "starts" else v).to(DEV) for k, v in st.items()}


def to_numpy(gt):
    return {k: (v.cpu().numpy().view(np.uint64) if k == "starts" else v.cpu().numpy()) for k, v in gt.items()}


def carousel_gpu(gt, done, cuts, seed, gid0, ctr, stream=None, starts=True):
    from rein48_amd import _lib
    from rein48_amd._lib import check, ptr
    s = torch.cuda.current_stream(DEV) if stream is None else stream
    check(_lib.load().r48_ntuple_carousel(ptr(gt["boards"]), len(gt["boards"]), ptr(done), (C.c_uint8 * len(cuts))(*cuts),
                                         len(cuts), ptr(gt["pool"]), ptr(gt["pool_has"]), ptr(gt["seen"]), ptr(gt["turn"]),
                                         ptr(gt["starts"]) if starts else None, seed, gid0, ctr, C.c_void_p(s.cuda_stream)))


def same(got, want, what):
    for k in NAMES:
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4].tolist())


def crafted_boards(rng, n, cuts):
    """Board i has its largest tile at tops[i % len(tops)]: every cut - 1, every cut, 15 and 17, in a
    random cell over smaller random tiles."""
    tops = sorted({c - 1 for c in cuts} | set(cuts) | {15, 17})
    boards = np.zeros((n, 16), np.int8)
    for i in range(n):
        top = tops[i % len(tops)]
        boards[i] = rng.integers(0, max(1, top), 16)
        boards[i, rng.integers(0, 16)] = top
    return boards


def random_state(rng, n, cuts, pool):
    S = len(cuts) + 1
    st = {"boards": crafted_boards(rng, n, cuts),
          "pool": rng.integers(0, 18, (S - 1, n, 16)).astype(np.int8),
          "pool_has": {"empty": np.zeros((S - 1, n), np.uint8), "full": np.ones((S - 1, n), np.uint8),
                       "half": rng.integers(0, 2, (S - 1, n)).astype(np.uint8)}[pool],
          "seen": rng.integers(0, S, n).astype(np.uint8), "turn": rng.integers(0, S, n).astype(np.uint8),
          "starts": rng.integers(0, 1 << 40, S).astype(np.uint64)}
    return st


def done_of(rng, n, kind):
    if kind == "random":   # any non-zero byte is done
        return (rng.integers(0, 2, n) * rng.integers(1, 256, n)).astype(np.uint8)
    return np.full(n, 1 if kind == "ones" else 0, np.uint8)


@pytest.mark.parametrize("gid0", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("cuts", [(4,), (3, 4, 6)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_one_call_equals_the_restatement(n, cuts, gid0):
    rng = np.random.default_rng(1000 * n + len(cuts) + (gid0 & 1))
    ctr = 0
    for kind in ("zeros", "ones", "random"):
        for pool in ("empty", "full", "half"):
            st = random_state(rng, n, cuts, pool)
            done = done_of(rng, n, kind)
            ctr = (ctr * 0x9E3779B1 + 0xFFFFFFF0) & 0xFFFFFFFF   # counters all over the 32 bits
            want = carousel_numpy(st, done, cuts, SEED, gid0, ctr)
            gt = to_gpu(st)
            carousel_gpu(gt, torch.from_numpy(done).to(DEV), cuts, SEED, gid0, ctr)
            same(to_numpy(gt), want, (kind, pool))
            # without starts: everything else the same, starts untouched
            gt = to_gpu(st)
            carousel_gpu(gt, torch.from_numpy(done).to(DEV), cuts, SEED, gid0, ctr, starts=False)
            same(to_numpy(gt), dict(want, starts=st["starts"]), (kind, pool, "no starts"))
            if kind == "ones" and pool == "full":   # every board restarts from the pool unless its turn wraps
                wraps = int((st["turn"] == len(cuts)).sum())
                assert int(want["starts"][0] - st["starts"][0]) == wraps and int((want["turn"] > 0).sum()) == n - wraps


@pytest.mark.parametrize("cuts", [(4,), (3, 4, 6)])
def test_a_chain_of_calls_equals_the_restatement(cuts):
    """50 calls on 257 boards from the all-zero start. Between the calls a finished board becomes a fresh
    one and most running boards grow by up to two exponents (now and then to 15..17), as an env step
    would leave them; the pools fill, and boards restart in every stage."""
    n, S, gid0 = 257, len(cuts) + 1, 2 ** 32 + 5
    rng = np.random.default_rng(7 + S)
    st = {"boards": np.zeros((n, 16), np.int8), "pool": np.zeros((S - 1, n, 16), np.int8),
          "pool_has": np.zeros((S - 1, n), np.uint8), "seen": np.zeros(n, np.uint8), "turn": np.zeros(n, np.uint8),
          "starts": np.zeros(S, np.uint64)}
    gt = to_gpu(st)
    for call in range(50):
        done = (rng.random(n) < 0.3).astype(np.uint8)
        boards = st["boards"].copy()
        for i in range(n):
            if done[i]:
                boards[i] = 0
                boards[i, rng.integers(0, 16)] = rng.integers(1, 3)
            elif rng.random() < 0.7:
                top = 15 + int(rng.integers(0, 3)) if rng.random() < 0.03 else min(17, int(boards[i].max()) + int(rng.integers(0, 3)))
                boards[i] = rng.integers(0, max(1, top), 16)
                boards[i, rng.integers(0, 16)] = top
        st["boards"] = boards
        gt["boards"].copy_(torch.from_numpy(boards))
        st = carousel_numpy(st, done, cuts, SEED, gid0, call)
        carousel_gpu(gt, torch.from_numpy(done).to(DEV), cuts, SEED, gid0, call)
        same(to_numpy(gt), st, call)
    assert all(int(x) > 0 for x in st["starts"]) and bool(st["pool_has"].any(axis=1).all())


def test_two_runs_on_two_streams_give_the_same_bits():
    n, cuts = 257, (3, 4, 6)
    rng = np.random.default_rng(5)
    st = random_state(rng, n, cuts, "half")
    done = torch.from_numpy(done_of(rng, n, "random")).to(DEV)
    outs = []
    for _ in range(2):
        gt = to_gpu(st)
        stream = torch.cuda.Stream(DEV)
        torch.cuda.synchronize()
        carousel_gpu(gt, done, cuts, SEED, 11, 3, stream=stream)
        stream.synchronize()
        outs.append(to_numpy(gt))
    same(outs[0], outs[1], "two streams")
    same(outs[0], carousel_numpy(st, done.cpu().numpy(), cuts, SEED, 11, 3), "and the restatement")


def test_the_result_is_a_function_of_n_and_gid0():
    """The halves of a batch of 256, run as batches of 128 with gid0 moved along, are what the contract
    says for n = 128 at their gid0 -- not the halves of the whole batch's result: the donor is
    mulhi(w0, n) within the batch given. With every pool slot full (and all pool boards distinct)
    a board restarts in the same stage either way, and from the same board exactly where the half's
    donor is the whole batch's donor slot."""
    n, h, cuts, gid0, ctr = 256, 128, (3, 4, 6), 2 ** 32 + 6, 16   # at this ctr three donors coincide
    rng = np.random.default_rng(12)
    st = random_state(rng, n, cuts, "full")
    st["turn"] = rng.integers(0, len(cuts), n).astype(np.uint8)   # no turn wraps: every board restarts from the pool
    for s in range(len(cuts)):   # the slot number in binary in cells 0..7, the pool's stage in cell 8: all distinct
        for i in range(n):
            st["pool"][s, i, :8] = [(i >> k) & 1 for k in range(8)]
            st["pool"][s, i, 8] = s
    done = done_of(rng, n, "ones")
    whole = carousel_numpy(st, done, cuts, SEED, gid0, ctr)
    gt = to_gpu(st)
    carousel_gpu(gt, torch.from_numpy(done).to(DEV), cuts, SEED, gid0, ctr)
    same(to_numpy(gt), whole, "whole")
    j_whole = donors(n, SEED, gid0, ctr)
    agree = 0
    for off in (0, h):
        part = {k: (v[:, off:off + h].copy() if k in ("pool", "pool_has") else v.copy() if k == "starts" else v[off:off + h].copy())
                for k, v in st.items()}
        want = carousel_numpy(part, done[off:off + h], cuts, SEED, gid0 + off, ctr)
        gp = to_gpu(part)
        carousel_gpu(gp, torch.from_numpy(done[off:off + h]).to(DEV), cuts, SEED, gid0 + off, ctr)
        got = to_numpy(gp)
        same(got, want, ("half", off))
        assert np.array_equal(got["turn"], whole["turn"][off:off + h])
        j_half = donors(h, SEED, gid0 + off, ctr) + off
        from_pool = got["turn"] > 0
        same_board = (got["boards"] == whole["boards"][off:off + h]).all(axis=1)
        assert np.array_equal(same_board[from_pool], (j_half == j_whole[off:off + h])[from_pool])
        agree += int(same_board[from_pool].sum())
    assert agree == 3   # a few donors coincide, most do not
