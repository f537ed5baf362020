"""Legal-move masks, afterstates and the masked selection / TD-target kernels (r48_moves.hip) on
the GPU against the C oracle's update_matrix (oracle.native.move) and numpy restatements.

Board counts 1, 63, 64, 65, 257 and 4099: a single lane, both sides of a wave boundary and a
ragged tail across workgroups. The oracle's four moves of the 4099 test boards are computed once
(module cache) and shared, unchanged, by every test.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import native as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 63, 64, 65, 257, 4099]
NMAX = max(SIZES)

EMPTY = [0] * 16
ONE_TILE = [0] * 5 + [1] + [0] * 10                                    # all four moves legal
NO_MOVES = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]            # full, game over
VERTICAL_ONLY = [1, 2, 3, 4, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]    # full; only UP / DOWN merge
HORIZONTAL_ONLY = [1, 1, 5, 9, 2, 2, 6, 10, 3, 3, 7, 11, 4, 4, 8, 12]  # its transpose: only LEFT / RIGHT
ROW_1111 = [0] * 4 + [1, 1, 1, 1] + [0] * 8                            # merge-once rule
ROW_2002 = [0] * 8 + [2, 0, 0, 2] + [0] * 4
HAS_17 = [17, 17, 16, 0, 0, 3, 0, 0, 0, 0, 0, 0, 1, 0, 0, 17]
CRAFTED = [EMPTY, ONE_TILE, NO_MOVES, VERTICAL_ONLY, HORIZONTAL_ONLY, ROW_1111, ROW_2002, HAS_17]


@functools.lru_cache(maxsize=None)
def reference():
    """(boards int8 [NMAX, 16], after int8 [4, NMAX, 16], reward int32 [4, NMAX], legal uint8 [NMAX])
    from the oracle: crafted boards first, then random exponent boards 0..17 of varied density, a
    third of them already pushed against a wall by one oracle move (so many have illegal moves)."""
    rng = np.random.default_rng(2048)
    boards = np.zeros((NMAX, 16), np.int8)
    boards[:len(CRAFTED)] = np.array(CRAFTED, np.int8)
    for i in range(len(CRAFTED), NMAX):
        emax = int(rng.integers(1, 18))
        fill = rng.integers(0, 17) / 16.0
        b = np.where(rng.random(16) < fill, rng.integers(1, emax + 1, 16), 0).astype(np.int8)
        if i % 3 == 0:
            b = O.move(b, int(rng.integers(0, 4)))[0]
        boards[i] = b
    after = np.zeros((4, NMAX, 16), np.int8)
    reward = np.zeros((4, NMAX), np.int32)
    legal = np.zeros(NMAX, np.uint8)
    for i in range(NMAX):
        for a in range(4):
            new, changed, rw = O.move(boards[i], a, with_reward=True)
            after[a, i] = new
            reward[a, i] = rw if changed else 0
            assert bool(changed) == bool((new != boards[i]).any())
            legal[i] |= (1 << a) if changed else 0
    for arr in (boards, after, reward, legal):
        arr.setflags(write=False)
    return boards, after, reward, legal


def T(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)     # a copy: the shared reference is read-only


def bits(legal):
    """uint8 [n] -> bool [n, 4]; no legal move counts as all-legal (the masked kernels' rule)."""
    ok = ((legal[:, None] >> np.arange(4)) & 1).astype(bool)
    ok[legal == 0] = True
    return ok


def test_crafted_boards_have_the_intended_legal_sets():
    _, _, reward, legal = reference()
    assert list(legal[:8]) == [0, 15, 0, 3, 12, 15, 15, 15]
    assert list(reward[:, 5]) == [0, 0, 8, 8] and list(reward[:, 6]) == [0, 0, 8, 8]   # merge once; [2,0,0,2]
    assert reward[2, 7] == 1 << 18                                                        # 17 + 17 -> 2^18


@pytest.mark.parametrize("n", SIZES)
def test_legal_and_afterstates_equal_the_oracle(n):
    """legal, the four planes and the merge rewards bit for bit; guard bytes behind every output
    stay as they were poisoned; each plane is a boards array other entry points accept."""
    from rein48_amd import _lib
    from rein48_amd.moves import afterstates, legal_actions
    boards, after, reward, legal = reference()
    boards, after, reward, legal = boards[:n], after[:, :n], reward[:, :n], legal[:n]
    bt = T(boards)
    guard = 256
    raw_after = torch.full((4 * n * 16 + guard,), 0x55, dtype=torch.int8, device=DEV)
    raw_reward = torch.full((4 * n + guard,), 0x55555555, dtype=torch.int32, device=DEV)
    raw_legal = torch.full((n + guard,), 0x55, dtype=torch.uint8, device=DEV)
    raw_legal2 = raw_legal.clone()
    a_t, r_t, l_t = afterstates(bt, after=raw_after[:4 * n * 16].view(4, n, 16), reward=raw_reward[:4 * n].view(4, n),
                                legal=raw_legal[:n])
    l2 = legal_actions(bt, out=raw_legal2[:n])
    np.testing.assert_array_equal(l2.cpu().numpy(), legal)
    np.testing.assert_array_equal(l_t.cpu().numpy(), legal)
    np.testing.assert_array_equal(a_t.cpu().numpy(), after)
    np.testing.assert_array_equal(r_t.cpu().numpy(), reward)
    assert bool((raw_after[4 * n * 16:] == 0x55).all()) and bool((raw_reward[4 * n:] == 0x55555555).all())
    assert bool((raw_legal[n:] == 0x55).all()) and bool((raw_legal2[n:] == 0x55).all())
    assert torch.equal(bt, T(boards))                                     # the input is only read
    # nullable outputs: NULL reward and legal through the C-ABI, and through the wrapper
    lib = _lib.load()
    only = torch.full((4, n, 16), 0x55, dtype=torch.int8, device=DEV)
    _lib.check(lib.r48_boards_afterstates(_lib.ptr(bt), n, _lib.ptr(only), None, None,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(only, a_t)
    a3, r3, l3 = afterstates(bt, want_reward=False, want_legal=False)
    assert r3 is None and l3 is None and torch.equal(a3, a_t)
    # every plane is itself a boards array: its legal set is the oracle's for that plane's boards
    for a in range(4):
        plane = a_t[a]
        assert plane.is_contiguous() and plane.data_ptr() % 16 == 0
        again = afterstates(plane)[0][a]                                  # the same move twice
        want = np.stack([O.move(after[a, i], a)[0] for i in range(min(n, 65))])
        np.testing.assert_array_equal(again[:min(n, 65)].cpu().numpy(), want)


def test_afterstate_planes_feed_the_env_score():
    """A plane bound as a VecGame's boards scores as the oracle scores that plane."""
    from rein48_amd import VecGame
    from rein48_amd.moves import afterstates
    boards, after, _, _ = reference()
    n = 257
    a_t = afterstates(T(boards[:n]))[0]
    env = VecGame(n, device=DEV, seed=1)
    for a in range(4):
        env.boards.copy_(a_t[a])
        np.testing.assert_array_equal(env.score().cpu().numpy(), O.score(after[a, :n]))


def test_wrapper_argument_errors():
    from rein48_amd.moves import afterstates, legal_actions
    b = T(reference()[0][:64])
    with pytest.raises(ValueError):
        legal_actions(b.cpu())
    with pytest.raises(TypeError):
        legal_actions(b.to(torch.int32))
    with pytest.raises(ValueError):
        legal_actions(b[:, :8])
    with pytest.raises(ValueError):
        legal_actions(b.view(-1)[:64 * 16 - 16].view(-1, 8))
    with pytest.raises(ValueError):
        legal_actions(b, out=torch.empty(63, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        afterstates(b, after=torch.empty((64, 4, 16), dtype=torch.int8, device=DEV))
    with pytest.raises(TypeError):
        afterstates(b, reward=torch.empty((4, 64), dtype=torch.float32, device=DEV))


def test_vecgame_legal_actions_agree_with_the_env_step():
    """Stepping with action a changes exactly the boards whose bit a is set (4099 boards, each a);
    after a Philox-mode step a board has no legal move iff it is done."""
    from rein48_amd import VecGame
    boards, _, _, legal = reference()
    n = NMAX
    env = VecGame(n, device=DEV, seed=77)
    bt = T(boards)
    for a in range(4):
        env.boards.copy_(bt)
        got = env.legal_actions()
        np.testing.assert_array_equal(got.cpu().numpy(), legal)
        env.step(torch.full((n,), a, dtype=torch.int8, device=DEV), want_changed=True)
        np.testing.assert_array_equal(env.changed.cpu().numpy(), (legal >> a) & 1)
    env.boards.copy_(bt)
    for _ in range(3):
        _, _, done = env.step(None)
        tiles = (env.boards != 0).any(dim=1)
        # an empty board (row 0 and the density-0 random ones; no move changes it, so it stays
        # empty) has no legal move and is not game over -- has_game_over needs a full board; every
        # board with a tile: no legal move iff done
        lg = env.legal_actions()
        assert not bool(tiles[0]) and bool((lg[~tiles] == 0).all()) and not bool(done[~tiles].any())
        assert torch.equal((lg == 0) & tiles, done != 0)
        assert bool((done != 0).any())
    after, reward, lg = env.afterstates()
    assert after.shape == (4, n, 16) and reward.shape == (4, n) and torch.equal(lg, env.legal_actions())


def _logits(n, rng):
    z = (rng.normal(size=(n, 4)) * 2).astype(np.float32)
    z[::5] = z[::5, :1]                                       # rows of equal logits
    z[1::11, 1] = z[1::11, 0]
    if n > 3:
        z[3] = [80.0, -80.0, 0.0, 79.5]                       # +-80 spread
    return z


@pytest.mark.parametrize("n", SIZES)
def test_masked_sampling(n):
    from rein48_amd.a3c.kernels import sample_actions
    boards, _, _, legal = reference()
    boards, legal = boards[:n], legal[:n]
    ok = bits(legal)
    rng = np.random.default_rng(n)
    z = _logits(n, rng)
    zm = np.where(ok, z, -np.inf).astype(np.float32)
    seed, ctr, gid0 = 0xA11CE, 7, 1000
    a_m, lp_m, en_m = sample_actions(T(z), seed, ctr, gid0=gid0, want_logp=True, want_entropy=True, boards=T(boards))
    a_u, lp_u, en_u = sample_actions(T(zm), seed, ctr, gid0=gid0, want_logp=True, want_entropy=True)
    a_m_h, a_u_h = a_m.cpu().numpy().astype(np.int64), a_u.cpu().numpy().astype(np.int64)
    rows = np.arange(n)
    assert ok[rows, a_m_h].all()                              # never an illegal action
    same = ok[rows, a_u_h]                                    # the unmasked draw on logits' was legal
    np.testing.assert_array_equal(a_m_h[same], a_u_h[same])
    st = torch.from_numpy(same).to(DEV)
    assert torch.equal(lp_m.view(torch.int32)[st], lp_u.view(torch.int32)[st])
    assert torch.equal(en_m.view(torch.int32), en_u.view(torch.int32))    # entropy does not depend on the draw
    # the other rows (rounding left the cumulative sum at or below u): the highest legal code, and rare
    other = ~same
    print("rows whose unmasked draw fell through to an illegal action: %d of %d" % (other.sum(), n))
    assert other.sum() <= int(0.001 * n)
    highest = 3 - np.argmax(ok[:, ::-1], axis=1)
    np.testing.assert_array_equal(a_m_h[other], highest[other])
    # all-legal boards: the masked kernel is the unmasked one bit for bit
    full = T(np.tile(np.array(ONE_TILE, np.int8), (n, 1)))
    a1, lp1, en1 = sample_actions(T(z), seed, ctr, gid0=gid0, want_logp=True, want_entropy=True, boards=full)
    a0, lp0, en0 = sample_actions(T(z), seed, ctr, gid0=gid0, want_logp=True, want_entropy=True)
    assert torch.equal(a1, a0) and torch.equal(lp1.view(torch.int32), lp0.view(torch.int32))
    assert torch.equal(en1.view(torch.int32), en0.view(torch.int32))


def _philox_rows(n, gid0, ctr, tag, seed):
    w = np.array([O.philox([(gid0 + i) & 0xFFFFFFFF, (gid0 + i) >> 32, ctr, tag], [seed & 0xFFFFFFFF, seed >> 32])
                  for i in range(n)], np.uint64)
    return w


def _egreedy_numpy(q, ok, w, eps):
    u = (w[:, 0] >> np.uint64(8)).astype(np.float64) / 16777216.0
    k = ok.sum(1).astype(np.uint64)
    j = ((w[:, 1] * k) >> np.uint64(32)).astype(np.int64)
    rank = np.cumsum(ok, axis=1) - 1                                       # rank of each legal action in code order
    explore = np.argmax(ok & (rank == j[:, None]), axis=1)
    greedy = np.argmax(np.where(ok, q, -np.inf), axis=1)
    return np.where(u < float(np.float32(eps)), explore, greedy).astype(np.int8)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("eps", [0.0, 0.3, 1.0])
def test_masked_egreedy_equals_numpy(n, eps):
    from rein48_amd.dqn.kernels import egreedy_actions
    boards, _, _, legal = reference()
    boards, legal = boards[:n], legal[:n]
    ok = bits(legal)
    rng = np.random.default_rng(100 + n)
    q = rng.normal(size=(n, 4)).astype(np.float32)
    q[::7, 1] = q[::7, 0]                                                   # ties -> first legal argmax
    q[::9] = q[::9, :1]
    worst = np.argmax(~ok, axis=1)                                          # an illegal action where there is one
    has_illegal = ~ok.all(1)
    q[has_illegal, worst[has_illegal]] = 50.0                               # the global argmax is illegal
    seed, ctr, gid0 = 5 + (9 << 32), 9, 300
    w = _philox_rows(n, gid0, ctr, 0xD0E, seed)
    got = egreedy_actions(T(q), eps, seed, ctr, gid0=gid0, boards=T(boards)).cpu().numpy()
    np.testing.assert_array_equal(got, _egreedy_numpy(q, ok, w, eps))
    assert ok[np.arange(n), got.astype(np.int64)].all()
    # all-legal boards: the masked kernel is r48_egreedy_actions bit for bit
    full = T(np.tile(np.array(ONE_TILE, np.int8), (n, 1)))
    assert torch.equal(egreedy_actions(T(q), eps, seed, ctr, gid0=gid0, boards=full),
                       egreedy_actions(T(q), eps, seed, ctr, gid0=gid0))


def test_masked_egreedy_explores_both_of_two_legal_moves():
    from rein48_amd.dqn.kernels import egreedy_actions
    n = NMAX
    q = np.random.default_rng(4).normal(size=(n, 4)).astype(np.float32)
    for board, allowed in ((VERTICAL_ONLY, (0, 1)), (HORIZONTAL_ONLY, (2, 3))):
        b = T(np.tile(np.array(board, np.int8), (n, 1)))
        got = egreedy_actions(T(q), 1.0, 11, 3, boards=b).cpu().numpy()
        assert set(np.unique(got)) == set(allowed)
        assert abs((got == allowed[0]).mean() - 0.5) < 0.05               # 4099 fair draws: sd 0.008


def _td_numpy(r, d, qt, qo, ok, terminal, gamma, log2):
    """fp32, in the kernel's order: boot = Q'(s', a*) or 0; y = R + gamma * boot."""
    sel = np.where(ok, qt if qo is None else qo, -np.inf)
    a = np.argmax(sel, axis=1)
    boot = qt[np.arange(qt.shape[0]), a].astype(np.float32)
    boot = np.where((d != 0) | terminal, np.float32(0), boot).astype(np.float32)
    R = np.log2(np.float32(1) + r).astype(np.float32) if log2 else r
    return (R + (np.float32(gamma) * boot).astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("log2", [False, True])
def test_masked_td_target_equals_numpy(n, double, log2):
    from rein48_amd.dqn.kernels import td_target
    boards, _, _, legal = reference()
    boards, legal = boards[:n], legal[:n]
    ok, terminal = bits(legal), legal == 0
    rng = np.random.default_rng(200 + n)
    r = (np.where(rng.random(n) < 0.5, 0.0, 2.0 ** rng.integers(1, 18, n)) if log2 else rng.normal(size=n)).astype(np.float32)
    d = (rng.random(n) < 0.2).astype(np.uint8)
    qt, qo = (rng.normal(size=(n, 4)).astype(np.float32) for _ in range(2))
    sel = qo if double else qt
    worst = np.argmax(~ok, axis=1)
    has_illegal = ~ok.all(1)
    sel[has_illegal, worst[has_illegal]] = 50.0                             # the unmasked a* is illegal
    y = td_target(T(r), T(d), T(qt), T(qo) if double else None, 0.97, log2_reward=log2, next_boards=T(boards))
    want = _td_numpy(r, d, qt, qo if double else None, ok, terminal, 0.97, log2)
    np.testing.assert_allclose(y.cpu().numpy(), want, rtol=1e-6, atol=1e-6)
    if n >= 8:   # the crafted rows: empty and game-over next boards bootstrap nothing even when not done
        y0 = td_target(T(r), None, T(qt), T(qo) if double else None, 0.97, log2_reward=log2, next_boards=T(boards))
        R = np.log2(np.float32(1) + r) if log2 else r
        np.testing.assert_allclose(y0.cpu().numpy()[[0, 2]], R[[0, 2]], rtol=1e-6, atol=1e-6)
    # all-legal next boards: r48_td_target bit for bit
    full = T(np.tile(np.array(ONE_TILE, np.int8), (n, 1)))
    args = (T(r), T(d), T(qt), T(qo) if double else None, 0.97)
    assert torch.equal(td_target(*args, log2_reward=log2, next_boards=full).view(torch.int32),
                       td_target(*args, log2_reward=log2).view(torch.int32))


@pytest.mark.parametrize("kw", [dict(net="cnn", bf16=True, features="exponents"), dict(net="mlp"),
                                dict(net="mlp", fused_policy=False)], ids=["cnn_fused", "mlp_fused", "torch"])
def test_a3c_masked_policy_draws_only_legal_moves(kw):
    """A3CTrainer.policy(mask_illegal=True) on the fused CNN, the fused MLP and the PyTorch path: every
    action is legal wherever a legal move exists, while the default policy stays the unmasked draw,
    some of whose actions on these boards are no-ops."""
    from rein48_amd.a3c import A3CConfig, A3CTrainer
    boards, _, _, legal = reference()
    n = 257
    bt, ok = T(boards[:n]), bits(legal[:n])
    tr = A3CTrainer(A3CConfig(n_boards=n, max_steps=5, seed=2, **kw), device=DEV)
    got = tr.policy(seed=9, mask_illegal=True)(bt, 4).cpu().numpy().astype(np.int64)
    assert ok[np.arange(n), got].all()
    assert (ok.sum(1) < 4).sum() > 20                      # the boards do have illegal moves to avoid
    plain = tr.policy(seed=9)(bt, 4)
    assert torch.equal(plain, tr.policy(seed=9, mask_illegal=False)(bt, 4))
    rows = torch.from_numpy(ok[np.arange(n), plain.cpu().numpy().astype(np.int64)]).to(DEV)
    assert bool(rows.any()) and not bool(rows.all())       # unmasked, some draws are no-ops
