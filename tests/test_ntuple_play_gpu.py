"""Whole games in one launch (k_nt_play1 / k_nt_play2 in r48_ntuple.hip, NTupleNet.play and
play_episodes) on the GPU against the composition they replace, bit for bit: n_steps x (NTupleNet.act
or search(depth 2), then VecGame.step) on a twin env with the same seed.

Depth 1: board counts 1, 63, 257 and 1,000 (a single lane, a partial wave, one workgroup plus one
lane, a ragged last workgroup), test_ntuple_fused_gpu.py's five layouts so that every tuple length's
instantiation runs, 1, 2 and 37 steps, envs with board_offset 0 and 1 (an odd offset takes the other
half of every Philox pair), from fresh games; and from that module's pool of running games with its
board without a move at row 3, on an env whose step counter is already 150. Depth 2: counts 1, 5 and
257 (more boards than one workgroup's four waves), layouts lines-squares and 1x6, 37 steps. Every
output is a slice of a poisoned buffer, the env's boards included; length and gain start from
nonzero words, since the kernel adds to them.
"""
import types

import pytest
import torch

from test_moves_gpu import T
from test_ntuple_fused_gpu import I_NO_MOVES, LAYOUTS, fill, nets, pool
from test_ntuple_gpu import guard_ok, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x2048
LEN0, GAIN0 = 3, 5                      # what length and gain hold before the call
POISON = 0x55


def net_of(lay, seed=5):
    net, twin = nets(lay)
    fill(net, twin, seed, 37.0)
    return net


def envs(n, offset, start=None, counter=None):
    """(env, its twin, the env's boards' guarded raw buffer): the same seed, offset, boards and counters."""
    from rein48_amd import VecGame, _lib
    out = []
    for _ in range(2):
        env = VecGame(n, device=DEV, seed=SEED, board_offset=offset)
        if start is None:
            env.reset()
        else:
            env.boards.copy_(T(start))
        if counter is not None:
            env.counters = (counter, 0)
        out.append(env)
    env, twin = out
    raw, view = guarded(n, torch.int8, POISON, row=16)          # the played env's boards live in a poisoned buffer
    view.copy_(env.boards)
    _lib.check(_lib.load().r48_env_bind_boards(env._env, _lib.ptr(view)))
    env.boards = view
    return env, twin, raw


def compose(net, twin, n_steps, depth):
    """n_steps x (act or search, env.step) on the twin -> (length, gain) summed from the env's changed
    and merge-reward outputs."""
    length = torch.zeros(twin.n, dtype=torch.int32, device=DEV)
    gain = torch.zeros(twin.n, dtype=torch.int32, device=DEV)
    reward = torch.zeros(twin.n, dtype=torch.int32, device=DEV)
    for _ in range(n_steps):
        actions = net.act(twin.boards)[0] if depth == 1 else net.search(twin.boards, 2)[0]
        twin.step(actions, merge_reward=True, want_changed=True, reward_out=reward)
        length += twin.changed.int()
        gain += reward
    return length, gain


def outputs(n):
    rl, length = guarded(n, torch.int32, 0x55555555)
    rg, gain = guarded(n, torch.int32, 0x55555555)
    rd, done = guarded(n, torch.uint8, POISON)
    length.fill_(LEN0)
    gain.fill_(GAIN0)
    return (rl, rg, rd), (length, gain, done)


def play_equals_composition(net, n, n_steps, depth, offset, start=None, counter=None):
    env, twin, rb = envs(n, offset, start, counter)
    want_len, want_gain = compose(net, twin, n_steps, depth)
    (rl, rg, rd), (length, gain, done) = outputs(n)
    out = net.play(env, n_steps, depth, length, gain, done)
    assert out[0] is env.boards and out[1] is length and out[2] is gain and out[3] is done
    assert torch.equal(env.boards, twin.boards), "boards differ"
    assert torch.equal(done, twin.done), "done differs"
    assert env.counters == twin.counters
    assert torch.equal(length, want_len + LEN0) and torch.equal(gain, want_gain + GAIN0)
    assert guard_ok(rb, 16 * n, POISON) and guard_ok(rl, n, 0x55555555) and guard_ok(rg, n, 0x55555555)
    assert guard_ok(rd, n, POISON)
    # the env is where the composition left it: the next step draws the same spawns
    actions = net.act(twin.boards)[0]
    env.step(actions)
    twin.step(actions)
    assert torch.equal(env.boards, twin.boards) and torch.equal(env.done, twin.done)
    return want_len, want_gain, twin


@pytest.mark.parametrize("n", [1, 63, 257, 1000])
@pytest.mark.parametrize("lay", sorted(LAYOUTS))
def test_depth_one_equals_act_and_env_step(lay, n):
    net = net_of(lay)
    for n_steps in (1, 2, 37):
        for offset in (0, 1):
            want_len, _, _ = play_equals_composition(net, n, n_steps, 1, offset)
            assert int(want_len.max()) == n_steps               # fresh games: some board moved at every step


@pytest.mark.parametrize("n", [1, 63, 257, 1000])
@pytest.mark.parametrize("lay", sorted(LAYOUTS))
def test_depth_one_on_running_games_with_a_finished_board_at_step_150(lay, n):
    net = net_of(lay)
    for offset in (0, 1):
        want_len, want_gain, twin = play_equals_composition(net, n, 37, 1, offset, start=pool()[:n], counter=150)
        assert twin.counters[0] == 150 + 37 + 1
        if n > I_NO_MOVES:
            assert int(want_len[I_NO_MOVES]) == 0 and int(want_gain[I_NO_MOVES]) == 0 and int(twin.done[I_NO_MOVES]) == 1
        if n >= 63:
            assert int(want_gain.max()) > 0


@pytest.mark.parametrize("n", [1, 5, 257])
@pytest.mark.parametrize("lay", ["lines-squares", "1x6"])
def test_depth_two_equals_search_and_env_step(lay, n):
    net = net_of(lay)
    play_equals_composition(net, n, 37, 2, 0)
    play_equals_composition(net, n, 37, 2, 1, start=pool()[:n], counter=150)


@pytest.mark.parametrize("depth", [1, 2])
def test_chunked_calls_add_up(depth):
    net = net_of("lines-squares")
    n = 257
    whole, parts, _ = envs(n, 1, start=pool()[:n], counter=150)
    (_, _, _), (wl, wg, wd) = outputs(n)
    (_, _, _), (pl, pg, pd) = outputs(n)
    net.play(whole, 37, depth, wl, wg, wd)
    net.play(parts, 20, depth, pl, pg, pd)
    assert parts.counters[0] == 170
    net.play(parts, 17, depth, pl, pg, pd)
    assert torch.equal(whole.boards, parts.boards) and torch.equal(wd, pd) and whole.counters == parts.counters
    assert torch.equal(wl, pl) and torch.equal(wg, pg) and int(wl.max()) > LEN0
    # no steps: nothing is touched, the counter stays
    before = parts.boards.clone()
    net.play(parts, 0, depth, pl, pg, pd)
    assert torch.equal(parts.boards, before) and torch.equal(wl, pl) and torch.equal(wd, pd)
    assert whole.counters == parts.counters


def test_games_played_to_the_end_and_play_episodes():
    from rein48_amd import evaluate
    net = net_of("lines-squares", seed=8)
    n, cap = 257, 4000
    env, twin, rb = envs(n, 0)
    want_len = torch.zeros(n, dtype=torch.int32, device=DEV)
    t = 0
    while t < cap:                                              # the composition, checked every 50 steps
        for _ in range(50):
            twin.step(net.act(twin.boards)[0], want_changed=True)
            want_len += twin.changed.int()
        t += 50
        if bool((twin.done != 0).all()):
            break
    assert bool((twin.done != 0).all()), "the cap of %d steps is too small for these tables: raise it" % cap
    (rl, rg, rd), (length, gain, done) = outputs(n)
    for _ in range(4):                                          # chunks of 1,000 steps, up to the cap
        net.play(env, cap // 4, 1, length, gain, done)
        if bool((done != 0).all()):
            break
    assert torch.equal(env.boards, twin.boards) and torch.equal(done, twin.done)
    assert torch.equal(length, want_len + LEN0)
    assert guard_ok(rb, 16 * n, POISON) and guard_ok(rl, n, 0x55555555) and guard_ok(rd, n, POISON)
    print("257 games to the end: %d steps by composition, longest game %d moves" % (t, int(want_len.max())))

    want = evaluate.play_episodes(net.policy(1), n, device=DEV, seed=13, return_scores=True)
    got = net.play_episodes(n, seed=13, depth=1, return_scores=True)
    assert set(got) == set(want) | {"mean_gain"}
    assert torch.equal(got["scores"], want["scores"])
    for k in want:
        if k not in ("steps_run", "scores"):
            assert got[k] == want[k], k
    from rein48_amd.ntuple import PLAY_CHUNK
    assert got["finished"] == 1.0 and got["mean_gain"] > 0 and got["steps_run"] % PLAY_CHUNK[1] == 0
    chunked = net.play_episodes(n, seed=13, depth=1, chunk=64, return_scores=True)
    assert chunked["steps_run"] % 64 == 0 and torch.equal(chunked["scores"], want["scores"])
    assert all(chunked[k] == got[k] for k in got if k not in ("steps_run", "scores"))


def test_the_call_follows_the_current_stream():
    net = net_of("lines-squares")
    n = 1000
    env, twin, _ = envs(n, 0, start=pool()[:n], counter=150)
    compose(net, twin, 37, 1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        _, length, gain, done = net.play(env, 37, 1)
        finished = torch.cuda.Event()
        finished.record(side)
    finished.synchronize()
    assert torch.equal(env.boards, twin.boards) and torch.equal(done, twin.done) and env.counters == twin.counters


def test_bad_arguments_are_refused():
    net = net_of("lines-squares")
    env, _, _ = envs(4, 0)
    for depth in (0, 3):
        with pytest.raises(ValueError):
            net.play(env, 1, depth)
    with pytest.raises(ValueError):
        net.play(types.SimpleNamespace(boards=torch.zeros((4, 16), dtype=torch.int8)), 1)
    with pytest.raises(ValueError):
        net.play(env, 1, 1, length=torch.zeros(5, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        net.play(env, 1, 1, gain=torch.zeros(4, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        net.play_episodes(4, depth=4)
    assert env.counters[0] == 0                                  # a refused call moves nothing
