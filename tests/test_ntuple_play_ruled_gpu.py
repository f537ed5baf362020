"""Whole games at a per-board search depth in one launch (k_nt_play_ruled in r48_ntuple.hip,
NTupleNet.play_ruled and play_episodes' depth 3 and rules) on the GPU against the composition they
replace, bit for bit: n_steps x (NTupleNet.search_ruled, then VecGame.step) on a twin env with the same
seed, offset, boards and counters -- boards, done, length, gain and the env's counters.

Boards: the fused tests' pool of running games with a full board that still has a move at row 1 and
the board without a move at row 2, on an env with an odd board_offset whose step counter is already
150. Counts 1, 3 and 257 (one workgroup, a few, many; one board per workgroup of 16 waves), every tuple
length 2..6, the rules all-1 and all-2 (which must also equal play at depths 1 and 2), all-3 and a mixed
rule under which all four depths occur, depth 4 at no more than one blank; 0, 1 and 37 steps, 20 + 17
against 37, and 8,193 boards for the mapping with 4 waves per board. Every output is a slice of a
poisoned buffer, the env's boards included; length and gain start from nonzero words, since the
kernel adds to them.
"""
import functools
import types

import numpy as np
import pytest
import torch

from test_moves_gpu import NO_MOVES, T
from test_ntuple_fused_gpu import LAYOUTS, pool
from test_ntuple_gpu import guard_ok
from test_ntuple_play_gpu import GAIN0, LEN0, POISON, envs, net_of, outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FULL_WITH_A_MOVE = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 3, 3]     # no blank; LEFT and RIGHT merge the last pair
I_FULL, I_NO_MOVES = 1, 2
ALL1, ALL2, ALL3 = (1,) * 17, (2,) * 17, (3,) * 17
MIXED = (4, 4, 3, 3, 2, 2) + (1,) * 11                                  # by blanks: <= 1 four plies, 2..3 three, 4..5 two
RULES = {"all-1": ALL1, "all-2": ALL2, "all-3": ALL3, "mixed": MIXED}
OFFSET, COUNTER = 1, 150


@functools.lru_cache(maxsize=None)
def start():
    """int8 [NMAX, 16] on the host, read-only: running games, the full board with a move, the finished one."""
    boards = pool().copy()
    boards[I_FULL] = FULL_WITH_A_MOVE
    boards[I_NO_MOVES] = NO_MOVES
    boards.setflags(write=False)
    return boards


def compose(net, twin, n_steps, rule):
    """n_steps x (search_ruled, env.step) on the twin -> (length, gain, the depths that were searched)."""
    length = torch.zeros(twin.n, dtype=torch.int32, device=DEV)
    gain = torch.zeros(twin.n, dtype=torch.int32, device=DEV)
    reward = torch.zeros(twin.n, dtype=torch.int32, device=DEV)
    seen = torch.zeros(5, dtype=torch.int64, device=DEV)
    for _ in range(n_steps):
        actions, _, legal, depth = net.search_ruled(twin.boards, rule)
        seen += torch.bincount(depth[legal != 0].long(), minlength=5)
        twin.step(actions, merge_reward=True, want_changed=True, reward_out=reward)
        length += twin.changed.int()
        gain += reward
    return length, gain, seen.cpu().numpy()


def play_equals_composition(net, boards, n_steps, rule, offset=OFFSET, counter=COUNTER):
    n = len(boards)
    env, twin, rb = envs(n, offset, boards, counter)
    want_len, want_gain, seen = compose(net, twin, n_steps, rule)
    (rl, rg, rd), (length, gain, done) = outputs(n)
    before = done.clone()
    out = net.play_ruled(env, n_steps, rule, length, gain, done)
    assert out[0] is env.boards and out[1] is length and out[2] is gain and out[3] is done
    assert torch.equal(env.boards, twin.boards), "boards differ"
    assert torch.equal(done, twin.done if n_steps else before), "done differs"
    assert env.counters == twin.counters == ((counter + n_steps) & 0xFFFFFFFF, 0)
    assert torch.equal(length, want_len + LEN0), "length differs"
    assert torch.equal(gain, want_gain + GAIN0), "gain differs"
    assert guard_ok(rb, 16 * n, POISON) and guard_ok(rl, n, 0x55555555) and guard_ok(rg, n, 0x55555555)
    assert guard_ok(rd, n, POISON)
    # the env is where the composition left it: the next step draws the same spawns
    actions = net.act(twin.boards)[0]
    env.step(actions)
    twin.step(actions)
    assert torch.equal(env.boards, twin.boards) and torch.equal(env.done, twin.done)
    return want_len, want_gain, twin, seen


@pytest.mark.parametrize("n", [1, 3, 257])
@pytest.mark.parametrize("lay", sorted(LAYOUTS))
@pytest.mark.parametrize("name", sorted(RULES))
def test_play_ruled_equals_search_ruled_and_env_step(name, lay, n):
    net = net_of(lay)
    rule = RULES[name]
    for n_steps in (0, 1, 37):
        want_len, want_gain, twin, seen = play_equals_composition(net, start()[:n], n_steps, rule)
    # what the 37 steps covered
    if n > I_NO_MOVES:
        assert int(want_len[I_NO_MOVES]) == 0 and int(want_gain[I_NO_MOVES]) == 0 and int(twin.done[I_NO_MOVES]) == 1
        assert int(want_len[I_FULL]) > 0 and int(want_gain[I_FULL]) > 0
    assert int(want_len.max()) > 1
    if n == 257:
        want_depths = set(rule)
        assert {d for d in range(1, 5) if seen[d] > 0} == want_depths, seen


@pytest.mark.parametrize("lay", ["lines-squares", "1x6"])
@pytest.mark.parametrize("depth", [1, 2])
def test_uniform_rules_of_ones_and_twos_equal_play(lay, depth):
    net = net_of(lay)
    n = 257
    ruled, plain, _ = envs(n, OFFSET, start()[:n], COUNTER)
    (_, _, _), (rl, rg, rd) = outputs(n)
    (_, _, _), (pl, pg, pd) = outputs(n)
    net.play_ruled(ruled, 37, (depth,) * 17, rl, rg, rd)
    net.play(plain, 37, depth, pl, pg, pd)
    assert torch.equal(ruled.boards, plain.boards) and torch.equal(rd, pd) and ruled.counters == plain.counters
    assert torch.equal(rl, pl) and torch.equal(rg, pg) and int(rl.max()) > LEN0


@pytest.mark.parametrize("name", sorted(RULES))
def test_chunked_calls_add_up(name):
    net = net_of("lines-squares")
    rule = RULES[name]
    n = 257
    whole, parts, _ = envs(n, OFFSET, start()[:n], COUNTER)
    (_, _, _), (wl, wg, wd) = outputs(n)
    (_, _, _), (pl, pg, pd) = outputs(n)
    net.play_ruled(whole, 37, rule, wl, wg, wd)
    net.play_ruled(parts, 20, rule, pl, pg, pd)
    assert parts.counters[0] == COUNTER + 20
    net.play_ruled(parts, 17, rule, pl, pg, pd)
    assert torch.equal(whole.boards, parts.boards) and torch.equal(wd, pd) and whole.counters == parts.counters
    assert torch.equal(wl, pl) and torch.equal(wg, pg) and int(wl.max()) > LEN0
    # no steps: nothing is touched, the counter stays
    before = parts.boards.clone()
    net.play_ruled(parts, 0, rule, pl, pg, pd)
    assert torch.equal(parts.boards, before) and torch.equal(wl, pl) and torch.equal(wd, pd)
    assert whole.counters == parts.counters


def test_the_other_wave_mapping_beyond_8192_boards():
    """8,193 boards run 4 waves per board instead of 16: the same bits. depth_rule(2): three plies at
    no more than 2 blanks, two elsewhere."""
    from rein48_amd.ntuple import NTupleNet
    net = net_of("lines-squares")
    rule = NTupleNet.depth_rule(2)
    n, few = 8193, 257
    boards = start()[np.arange(n) % len(start())]
    env, twin, rb = envs(n, OFFSET, boards, COUNTER)
    want_len, want_gain, seen = compose(net, twin, 3, rule)
    assert seen[2] > 0 and seen[3] > 0 and seen[1] == 0 and seen[4] == 0
    (rl, rg, rd), (length, gain, done) = outputs(n)
    net.play_ruled(env, 3, rule, length, gain, done)
    assert torch.equal(env.boards, twin.boards) and torch.equal(done, twin.done) and env.counters == twin.counters
    assert torch.equal(length, want_len + LEN0) and torch.equal(gain, want_gain + GAIN0)
    assert guard_ok(rb, 16 * n, POISON) and guard_ok(rl, n, 0x55555555) and guard_ok(rg, n, 0x55555555)
    assert guard_ok(rd, n, POISON)
    # board i of a small batch is board i of the large one: the mapping does not reach the bits
    small, _, _ = envs(few, OFFSET, boards[:few], COUNTER)
    _, sl, sg, sd = net.play_ruled(small, 3, rule)
    assert torch.equal(small.boards, env.boards[:few]) and torch.equal(sd, done[:few])
    assert torch.equal(sl + LEN0, length[:few]) and torch.equal(sg + GAIN0, gain[:few])


def test_the_call_follows_the_current_stream():
    net = net_of("lines-squares")
    n = 257
    env, twin, _ = envs(n, OFFSET, start()[:n], COUNTER)
    compose(net, twin, 37, MIXED)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        _, length, gain, done = net.play_ruled(env, 37, MIXED)
        finished = torch.cuda.Event()
        finished.record(side)
    finished.synchronize()
    assert torch.equal(env.boards, twin.boards) and torch.equal(done, twin.done) and env.counters == twin.counters


def test_games_played_to_the_end_under_three_plies_and_play_episodes():
    from rein48_amd import evaluate
    from rein48_amd.ntuple import ruled_chunk
    net = net_of("lines-squares", seed=8)
    n = 64
    want = evaluate.play_episodes(net.policy(3), n, device=DEV, seed=13, return_scores=True)
    got = net.play_episodes(n, seed=13, depth=3, return_scores=True)
    assert set(got) == set(want) | {"mean_gain"}
    assert torch.equal(got["scores"], want["scores"])
    for k in want:
        if k not in ("steps_run", "scores"):
            assert got[k] == want[k], k
    assert got["finished"] == 1.0 and got["mean_gain"] > 0 and got["steps_run"] % ruled_chunk(3, n) == 0
    print("64 games to the end at depth 3: mean length %.1f, steps run %d (evaluate: %d)"
          % (got["mean_length"], got["steps_run"], want["steps_run"]))
    ruled = net.play_episodes(n, seed=13, rule=ALL3, chunk=50, return_scores=True)
    assert ruled["steps_run"] % 50 == 0 and torch.equal(ruled["scores"], want["scores"])
    assert all(ruled[k] == got[k] for k in got if k not in ("steps_run", "scores"))
    mixed = net.play_episodes(n, seed=13, rule=MIXED, return_scores=True)
    want_mixed = evaluate.play_episodes(net.policy(rule=MIXED), n, device=DEV, seed=13, return_scores=True)
    assert torch.equal(mixed["scores"], want_mixed["scores"]) and mixed["finished"] == 1.0
    assert mixed["mean_length"] == want_mixed["mean_length"]


def test_the_default_chunk_depends_on_the_largest_depth_and_the_board_count_alone():
    from rein48_amd.ntuple import RULED_BUDGET, RULED_MAX_CHUNK, ruled_chunk
    assert sorted(RULED_BUDGET) == sorted(RULED_MAX_CHUNK) == [1, 2, 3, 4]
    assert all(RULED_BUDGET[d] > RULED_BUDGET[d + 1] and RULED_MAX_CHUNK[d] > RULED_MAX_CHUNK[d + 1] for d in (1, 2, 3))
    for d in (1, 2, 3, 4):
        assert ruled_chunk(d, 4096) == min(RULED_BUDGET[d] // 4096, RULED_MAX_CHUNK[d]) >= 1
        assert ruled_chunk(d, 2 ** 30) == 1 and ruled_chunk(d, 1) == RULED_MAX_CHUNK[d]


def test_bad_arguments_are_refused():
    net = net_of("lines-squares")
    env, _, _ = envs(4, 0)
    for bad in ((2,) * 16, (2,) * 18, (0,) + (2,) * 16, (2,) * 16 + (5,)):
        with pytest.raises(ValueError):
            net.play_ruled(env, 1, bad)
        with pytest.raises(ValueError):
            net.play_episodes(4, rule=bad)
    with pytest.raises(ValueError):
        net.play_ruled(types.SimpleNamespace(boards=torch.zeros((4, 16), dtype=torch.int8)), 1, ALL3)
    with pytest.raises(ValueError):
        net.play_ruled(env, 1, ALL3, length=torch.zeros(5, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        net.play_ruled(env, 1, ALL3, length=torch.zeros(4, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        net.play(env, 1, 3)                                      # play itself still stops at two plies
    assert env.counters[0] == 0                                  # a refused call moves nothing
