"""k_step_n's auto-reset from the line-form LDS table vs the C oracle (GPU, bit-exact).

Every AUTO_RESET instantiation of k_step_n resets a finished board by reading
r48::reset_lines(action, cell, tile) from a 128-entry LDS table, the board staying in the line form
of the step's action. Near-full start boards (5 % blanks, exponents up to 12) end > 10 % of the
boards within a few steps, so a call of 2, 3 or 8 steps resets ~10^4 boards; the oracle
(oracle/r48_oracle.c, rows only, independent of every GPU kernel) is stepped once per board offset
and shared. n = 2^16 + 37: 128 full 512-board tiles (the fast path, where the table is used) and a
partial tile (the guarded per-board path); offset 3 sends the whole grid down the guarded path.
The coverage test (CPU only) shows that the oracle's resets inside the full tiles at offset 0 hit
all 128 (action, cell, tile) table entries.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import native as O
from test_env_gpu import DEV, host, put, rand_boards, vec

N = (1 << 16) + 37
FULL = (N // 512) * 512          # boards in full tiles: k_step_n's fast path at an even offset
SEED = 20480
KMAX = 8
KS = [2, 3, 8]


@functools.lru_cache(maxsize=None)
def start_boards():
    b = rand_boards(np.random.default_rng(4801), N, emax=12, p_empty=0.05)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def oracle_steps(off):
    """The oracle's KMAX random-policy auto-reset steps (merge reward and score recorded)."""
    out, b = [], start_boards()
    for t in range(KMAX):
        r = O.step_philox(b, SEED, t, O.RANDOM_POLICY | O.AUTO_RESET | O.MERGE_REWARD, board_offset=off,
                          want_score=True)
        b = r["boards"]
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def given_actions():
    rng = np.random.default_rng(4802)
    acts = rng.integers(0, 4, N).astype(np.int8)
    bad = rng.random(N) < 0.25
    acts[bad] = rng.choice(np.array([-128, -1, 4, 5, 6, 7, 100, 127], np.int8), int(bad.sum()))
    acts.setflags(write=False)
    return acts


@functools.lru_cache(maxsize=None)
def oracle_given(off):
    out, b, acts = [], start_boards(), given_actions()
    for t in range(KMAX):
        r = O.step_philox(b, SEED, t, O.AUTO_RESET | O.MERGE_REWARD, actions=acts, board_offset=off, want_score=True)
        b = r["boards"]
        out.append(r)
    return out


def reset_combos(r, lo=0, hi=N):
    """(action & 3, cell, tile 4?) of every board the oracle reset in step result r."""
    idx = np.flatnonzero(r["done"][lo:hi]) + lo
    nb = r["boards"][idx]
    assert ((nb != 0).sum(axis=1) == 1).all()          # a reset board is one tile
    cell = (nb != 0).argmax(axis=1)
    tile = nb[np.arange(len(idx)), cell]
    assert np.isin(tile, (1, 2)).all()
    return (r["actions"][idx].astype(np.int64) & 3) << 5 | (tile == 2).astype(np.int64) << 4 | cell


def test_oracle_resets_cover_every_table_entry():
    """No GPU: the resets the oracle reports inside the fast path's full tiles (offset 0) use all
    128 table entries, the ones of tile 4 (p ~ 1/640 per reset) included."""
    per_step = [reset_combos(r, 0, FULL) for r in oracle_steps(0)]
    combos = np.concatenate(per_step)
    print("resets per step:", [len(c) for c in per_step], "distinct entries:", len(np.unique(combos)))
    assert len(combos) >= 5000
    assert len(np.unique(combos)) == 128
    # the short calls reset boards too, with every action
    for K in KS:
        assert len(np.unique(np.concatenate(per_step[:K]) >> 5)) == 4
    # given actions: dead boards with a bad action byte are reset as well
    g = oracle_given(0)
    bad = (given_actions().view(np.uint8) > 3)
    assert sum(int((r["done"][:FULL] != 0)[bad[:FULL]].sum()) for r in g[:2]) > 100


def check_last_step(v, want, reward, score):
    assert np.array_equal(host(v.boards), want["boards"])
    assert np.array_equal(host(v.actions), want["actions"])
    assert np.array_equal(host(v.done), want["done"])
    assert np.array_equal(host(v.changed), want["changed"])
    assert np.array_equal(host(score), want["score"])
    if reward:
        assert np.array_equal(host(v.reward), want["reward"])


@pytest.mark.gpu
@pytest.mark.parametrize("reward", [False, True])
@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("K", KS)
def test_step_n_auto_reset_matches_oracle(K, off, reward):
    want = oracle_steps(off)[K - 1]
    v = vec(N, seed=SEED, offset=off)
    put(v, start_boards())
    score = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    v.step_n(K, auto_reset=True, merge_reward=reward, want_changed=True, score=score)
    torch.cuda.synchronize()
    check_last_step(v, want, reward, score)
    assert v.counters == (K, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("K", KS)
def test_rollout_rows_match_oracle(K, off):
    want = oracle_steps(off)
    v = vec(N, seed=SEED, offset=off)
    put(v, start_boards())
    acts = torch.full((K, N), -1, dtype=torch.int8, device=DEV)
    dn = torch.full((K, N), 255, dtype=torch.uint8, device=DEV)
    v.rollout(K, actions=acts, done=dn)
    torch.cuda.synchronize()
    acts, dn = host(acts), host(dn)
    for t in range(K):
        assert np.array_equal(acts[t], want[t]["actions"]), t
        assert np.array_equal(dn[t], want[t]["done"]), t
    assert np.array_equal(host(v.boards), want[K - 1]["boards"])


@pytest.mark.gpu
@pytest.mark.parametrize("reward", [False, True])
@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("K", KS)
def test_step_n_given_actions_auto_reset_matches_oracle(K, off, reward):
    want = oracle_given(off)
    acts = given_actions()
    v = vec(N, seed=SEED, offset=off)
    put(v, start_boards())
    v.error_count(clear=True)
    score = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    a_dev = torch.from_numpy(acts.copy()).to(DEV)
    v.step_n(K, a_dev, auto_reset=True, merge_reward=reward, want_changed=True, score=score)
    torch.cuda.synchronize()
    w = want[K - 1]
    assert np.array_equal(host(v.boards), w["boards"])
    assert np.array_equal(host(v.done), w["done"])
    assert np.array_equal(host(v.changed), w["changed"])
    assert np.array_equal(host(score), w["score"])
    if reward:
        assert np.array_equal(host(v.reward), w["reward"])
    assert np.array_equal(host(a_dev), acts)                      # the caller's actions are not written
    assert v.error_count() == K * int((acts.view(np.uint8) > 3).sum()) == sum(r["bad"] for r in want[:K])
