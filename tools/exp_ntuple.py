"""GPU experiment: the n-tuple network's kernels (r48_ntuple.hip) and trainer.

    python tools/exp_ntuple.py [--out DIR] [--sizes 65536,1048576] [--scores]
    python tools/exp_ntuple.py --search [--out DIR] [--sizes 4096,65536] [--scores] [--long]
    python tools/exp_ntuple.py --tc [--out DIR] [--sizes 65536,1048576] [--scores]
    python tools/exp_ntuple.py --search3 [--out DIR] [--sizes 256,4096,16384] [--scores] [--episodes N] [--ab-lib SO]
    python tools/exp_ntuple.py --fused [--out DIR] [--sizes 1024,4096,65536,1048576] [--scores] [--episodes N]
    python tools/exp_ntuple.py --play [--out DIR] [--sizes 4096,65536] [--episodes N] [--ab-lib SO]
    python tools/exp_ntuple.py --ruled [--out DIR] [--sizes 256,4096,16384] [--scores] [--episodes N]

For both named layouts and each board count: device-event times (5 warm-up calls, median of 7
windows of 20 calls) of value, act, accumulate and apply with their table loads or atomics per
second, act against the unfused path (afterstates -> value on 4n boards -> torch argmax,
evaluate.afterstate_policy(net.value)), and a whole train_step (host clock around 50 steps ending in
a synchronise). Boards are those of running games: 150 greedy-merge steps from reset with auto-reset
(games last ~257 steps under that policy); the update kernels get their afterstates. Tables are
random floats, so the gathers are spread as after training.

--scores: train each layout for the stated budgets and play 4,096 whole episodes
(evaluate.play_episodes) next to the greedy-merge policy -- the rows of BASELINE.md's policy table.
Writes exp_ntuple.json (and prints the same) under --out.

--search: the 2-ply expectimax search instead. For both layouts and each board count (default 4,096
and 65,536), the same device-event method on (a) search(depth=2), (b) act and (c) the unfused
composition of existing entry points written here (unfused_search: afterstates -> the children of
every legal afterstate laid out by torch -> act on the children -> torch reduction), with how often
(c) picks the fused search's action. With --scores: whole-episode scores of policy(depth=1) against
policy(depth=2) on the same trained tables (1,024 x 2,000 steps for both layouts; --long adds 4,096 x
10,000 for 4x6), 4,096 episodes, eval seed 13. Writes exp_ntuple_search.json under --out.

--search3: the 3-ply search. For both layouts and each board count (default 256, 4,096 and 2^14), the
same device-event method with alternated windows on (a) search3, (b) search(depth=2) and (c) the
unfused composition written here (unfused_search with the depth-2 kernel for the leaves: afterstates
-> the root's children laid out by torch, a host sync -> search(children, 2) -> torch max, scatter-add
and argmax), with the share of boards on which (c) picks search3's action. --ab-lib SO[,SO...]: other
builds of the library (-DR48_NT_SEARCH3_WAVES=4, 16, ...: the waves that share a board) whose
r48_ntuple_search3 are alternated with this one's in the same windows, outputs compared bit for bit. With --scores: play_episodes at depths
2 and 3 with the recorded recipes' tables (lines-squares and 4x6 at 1,024 x 2,000 steps TD(0), 4x6 at
4,096 x 10,000 TC; --episodes each, default 4,096, eval seed 13) and the learning test's recipe
(lines-squares 1,024 x 1,000, 512 episodes, eval seed 1). Writes exp_ntuple_search3.json.

--tc: temporal-coherence learning rates against plain TD(0). For both layouts and each board count,
device-event times in one process with alternated windows (TD window, TC window, TD window, ...;
5 warm-up calls each, median of 7 windows of 20 calls): accumulate + apply on a tc=False net against
accumulate + apply_tc on a tc=True net (the same boards and deltas; apply and apply_tc derived by
subtracting accumulate alone, as above), tc_rate next to value, and a whole train_step of a TD
trainer against a TC one -- once with alpha 0 for both (frozen zero tables: the two play the same
games, so each pair of windows sees the same boards) and once with the recipes' alphas. With --scores: TD(0) alpha 0.25 against TC alpha 1.0 at depth 1 and 2 for
lines-squares and 4x6 at 1,024 x 2,000 steps and 4x6 at 4,096 x 10,000, 4,096 episodes, eval seed
13, and the 1,024 x 1,000 lines-squares recipe of the learning test. Writes exp_ntuple_tc.json.

--fused: the fused training step (NTupleConfig.fused: td_act, apply, env.step) against the unfused
one of the same build. For both layouts, each board count (default 1,024, 4,096, 2^16 and 2^20) and
TD (alpha 0.25) and TC (alpha 1.0): a fused and an unfused trainer from the same seed -- they are
bit-identical, which is checked at the end, so each pair of windows sees the same boards -- stepped
in alternated windows on the host clock (20 warm-up steps each, median of 7 windows of 20 steps and
a synchronise), with the windows' min-max spread next to the difference. Then device-event times of
td_act against act + accumulate, act and accumulate on the same inputs. With --scores: the 4x6 TC
recipe (4,096 boards, alpha 1.0, seed 0) for 10,000 unfused steps, the fused steps that fit in the
same wall time, and the depth-1 score of each (--episodes, eval seed 13). Writes exp_ntuple_fused.json.

--play: whole games in one launch (NTupleNet.play / play_episodes, r48_ntuple_play). On the tables of
the recorded recipes (lines-squares 1,024 x 2,000 TD(0), 4x6 4,096 x 10,000 TC) and at depths 1 and 2:
--episodes (default 4,096, eval seed 13) whole episodes through play_episodes and through
evaluate.play_episodes(net.policy(depth)) in the same process, each run twice and the second timed
(wall seconds ending in a synchronise, device milliseconds between events around the call), scores
compared bit for bit; the device time per step on 4,096 and 2^16 live boards of play against act (or
search) + env.step in alternated windows; and the device time of single launches of 250 .. 2,000
(depth 1) and 25 .. 200 (depth 2) steps at 2^16 boards, the figures behind ntuple.PLAY_CHUNK.
--ab-lib SO: another build of the library (-DR48_NT_PLAY_LANES=4: four lanes per board at depth 1)
whose r48_ntuple_play is alternated with this one's, boards compared bit for bit. Writes
exp_ntuple_play.json.

--ruled: the search at a depth chosen per board (NTupleNet.search_ruled, r48_ntuple_search_ruled). (a)
For both layouts and each board count (default 256, 4,096 and 2^14): search_ruled under the all-3 rule
against search3 on the same boards of running games, alternated windows, outputs compared bit for bit
-- what the shared deal-and-finish body costs over k_nt_search3; --ab-lib SO[,SO...]: other builds
of the library whose r48_ntuple_search_ruled is alternated with them in the same windows. (b) For both layouts, by rule --
depth_rule(d3) for d3 = 2, 4, 6, 8, 16 and depth_rule(16, d4) for d4 = 0 .. 4, next to search(2) and
search3: the time per call at 4,096 boards of running games (alternated windows of 5 calls), the
share of boards at each depth from depth_out, and the longest of 5 single launches at 2^16 boards.
With --scores: play_episodes under policy(2), policy(3) and those rules on the recorded recipes'
tables (lines-squares 1,024 x 2,000 TD(0), 4x6 4,096 x 10,000 TC; --episodes each, eval seed 13; d4
up to --max-d4, default 3) with the evaluation seconds next to each, and policy(2), policy(3) and
the rules on the learning test's recipe (lines-squares 1,024 x 1,000, 512 episodes, eval seed 1).
Writes exp_ntuple_ruled.json.

--play-ruled: whole games at a per-board depth in one launch (NTupleNet.play_ruled, r48_ntuple_play_ruled;
play_episodes at depth 3 and under a rule). On the tables of the recorded recipes (lines-squares 1,024 x
2,000 TD(0), 4x6 4,096 x 10,000 TC): (a) --episodes (default 4,096, eval seed 13) whole episodes under
depth 3 and depth_rule(16, 1) (--long: depth_rule(16, 3) too) through play_episodes and through
evaluate.play_episodes(net.policy(...)) -- the Python loop, which is what play_episodes was before -- in
the same process, a first run of each and then the timed ones (two at depth 3, whose difference is the
A/A spread; one under the rules), scores compared bit for bit and with the recorded ones; (b) the device
time per step on 4,096 and 2^14 boards of running games, play_ruled's 20 steps in one launch against 20 x
(search_ruled, env.step), alternated windows, for all-3 and depth_rule(16, 1); --ab-lib SO[,SO...]: other
builds of the library (-DR48_NT_PLAY_RULED_WAVES=4 / 8 / 16) alternated in the same windows, boards
compared bit for bit; (c) single launches at 4,096 boards from running games and from reset, and of
play_episodes' chunk at 64 boards, the figures behind ntuple.RULED_BUDGET and RULED_MAX_CHUNK; the whole
evaluations of (a) also with 64 and 512 episodes. Writes exp_ntuple_play_ruled.json. With --waves-ab, only the A/B of waves per
board on whole evaluations: --episodes episodes to the end in play_episodes' chunks through each --ab-lib
build, and single launches and whole evaluations of 64 boards, where one board's latency is what counts.
Writes exp_ntuple_play_ruled_waves.json.

With --stages, multi-stage tables with weight promotion: (a) value, act, search depth 2, search3, accumulate +
apply, accumulate + apply_tc and the TC trainer's fused and unfused step with stages=(9,) against the unstaged
net on the same boards, --sizes boards (default 4096,65536), the two builds' windows interleaved; (b) with
--scores, the 4x6 TC recipe (4,096 boards, alpha 1.0, seed 0, fused) for --budgets steps (default 10000,40000)
with the cuts (), (9,), (10,) and (8, 10): --episodes whole games at eval seed 13 at depths 1, 2 and 3, the share
of games reaching 2,048 / 4,096 / 8,192 and the share of own[1] set. --no-kernels skips (a). Writes
exp_ntuple_stages.json.

With --carousel, carousel shaping (NTupleConfig.carousel): (a) the carousel call alone and the fused TC
trainer's step with carousel=(10,) against the same trainer without, windows interleaved, after 300 steps of
each, --sizes boards (default 1024,4096,65536); (b) with --scores, the 4x6 TC recipe of --stages for --budgets
steps with stages (), (10,) and (8, 10), each without carousel and with the carousel on the net's cuts ((10,)
for the unstaged net): --episodes whole games at eval seed 13 at depths 1, 2 and 3, the difference to the
row without carousel in standard errors of the difference, own[k], carousel_stats() and the training's wall
time; the rows without carousel are checked against the recorded exp_ntuple_stages.json
(reproduces_recorded). --no-kernels skips (a). Writes exp_ntuple_carousel.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from rein48_amd import VecGame  # noqa: E402
from rein48_amd.evaluate import afterstate_policy, play_episodes  # noqa: E402
from rein48_amd.ntuple import NTupleConfig, NTupleNet, NTupleTrainer  # noqa: E402

DEV = "cuda:0"


def event_ms(fn, warmup=5, windows=7, calls=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return statistics.median(out), min(out), max(out)


def kernels(layout, n):
    net = NTupleNet(layout, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    net.tables.copy_(torch.randn(net.tables.shape, generator=g, device=DEV) * 30.0)
    env = VecGame(n, device=DEV, seed=7)
    env.reset()
    greedy = afterstate_policy(None)
    for t in range(150):
        env.step(greedy(env.boards, t), auto_reset=True)
    boards = env.boards.clone()
    delta = torch.randn(n, generator=g, device=DEV) * 100.0
    hits = 8 * net.m * n
    a, after, v, r, legal = net.act(boards)
    n_legal = int(sum(((legal >> k) & 1).sum() for k in range(4)))
    unfused = afterstate_policy(net.value)
    same = bool(torch.equal(unfused(boards, 0), a))
    res = {"layout": layout, "boards": n, "tuples": net.m, "length": net.L, "legal_moves": n_legal,
           "unfused_actions_equal": same}

    def row(name, fn, count, unit):
        med, lo, hi = event_ms(fn)
        res[name] = {"ms": med, "ms_min": lo, "ms_max": hi, unit + "_per_s": count / (med * 1e-3)}

    row("value", lambda: net.value(boards, out=v), hits, "loads")
    row("act", lambda: net.act(boards, a, after, v, r, legal), 8 * net.m * n_legal, "loads")
    row("act_unfused", lambda: unfused(boards, 0), 8 * net.m * 4 * n, "loads")
    # accumulate needs zero scratch: each timed call is accumulate + apply; apply alone = the pair - accumulate,
    # with accumulate alone timed against a scratch that is cleared outside the windows
    row("accumulate_apply", lambda: net.td_update(after, delta, 0.25), 3 * hits, "atomics")

    def accumulate_only():
        net.accumulate(after, delta)
    med, lo, hi = event_ms(accumulate_only)              # sums grow; the integer adds cost the same
    res["accumulate"] = {"ms": med, "ms_min": lo, "ms_max": hi, "atomics_per_s": 2 * hits / (med * 1e-3)}
    net.acc.zero_()                                        # scratch back to zero
    net.cnt.zero_()
    ap = max(res["accumulate_apply"]["ms"] - res["accumulate"]["ms"], 1e-6)
    res["apply"] = {"ms": ap, "derived": "accumulate_apply - accumulate", "exchanges_per_s": hits / (ap * 1e-3)}
    res["act_speedup_vs_unfused"] = res["act_unfused"]["ms"] / res["act"]["ms"]
    del net
    torch.cuda.empty_cache()
    return res


def train_step_ms(layout, n):
    tr = NTupleTrainer(NTupleConfig(n_boards=n, layout=layout, alpha=0.25, seed=3), device=DEV)
    for _ in range(20):
        tr.train_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        tr.train_step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 50 * 1e3
    del tr
    torch.cuda.empty_cache()
    return {"layout": layout, "boards": n, "train_step_ms": ms, "env_steps_per_s": n / (ms * 1e-3)}


def scores(layout, n_boards, steps, eval_seed=13):
    tr = NTupleTrainer(NTupleConfig(n_boards=n_boards, layout=layout, alpha=0.25, seed=0), device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_step()
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    ev = play_episodes(tr.net.policy(), 4096, device=DEV, seed=eval_seed)
    del tr
    torch.cuda.empty_cache()
    return {"layout": layout, "train_boards": n_boards, "train_steps": steps, "alpha": 0.25, "train_seconds": train_s,
            "eval_seed": eval_seed, "eval": ev}


def unfused_search(net, leaves=None):
    """leaves(kids) -> float32 [K]: the value of every child; the default is depth 2's, act's best
    score. The depth-2 search composed from the entry points that existed before it: one afterstates
    launch, the children of every legal afterstate (each empty cell filled with a 2 and with a 4)
    gathered by torch, act on the children for their leaves, a torch scatter-add for S_a and the
    argmax. Returns (actions, q [4, n]). The scatter-add uses float atomics, so q is not
    reproducible to the bit as the fused search's is."""
    from rein48_amd.moves import afterstates
    bit = torch.tensor([[1], [2], [4], [8]], dtype=torch.uint8, device=DEV)
    ninf = float("-inf")

    def search(boards):
        after, reward, legal = afterstates(boards)                    # [4, n, 16]
        n = legal.shape[0]
        ok = (legal.unsqueeze(0) & bit) != 0                            # [4, n]
        empty = (after == 0) & ok.unsqueeze(2)
        ia, ii, ic = empty.nonzero(as_tuple=True)                       # host sync: the child count
        k = ia.numel()
        kids = after[ia, ii].repeat_interleave(2, dim=0)                # [2k, 16]: e = 1, 2 per cell
        e = torch.tensor([1, 2], dtype=torch.int8, device=DEV).repeat(k)
        kids[torch.arange(2 * k, device=DEV), ic.repeat_interleave(2)] = e
        if leaves is None:
            _, _, v, r, lg = net.act(kids)
            leaf = torch.where(lg != 0, r.float() + v, torch.zeros_like(v))
        else:
            leaf = leaves(kids)
        w = torch.tensor([9.0, 1.0], device=DEV).repeat(k)
        s = torch.zeros((4, n), dtype=torch.float32, device=DEV)
        s.index_put_((ia.repeat_interleave(2), ii.repeat_interleave(2)), w * leaf, accumulate=True)
        n_e = empty.sum(2).clamp(min=1).float()
        q = torch.where(ok, reward.float() + s / (10.0 * n_e), torch.full_like(s, ninf))
        best = q.max(dim=0, keepdim=True).values
        code = torch.arange(4, dtype=torch.int8, device=DEV).view(4, 1).expand(4, n)
        first = torch.where((q == best) & ok, code, torch.full_like(code, 4)).min(dim=0).values
        return torch.where(first == 4, torch.zeros_like(first), first), q
    return search


def search_kernels(layout, n):
    net = NTupleNet(layout, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    net.tables.copy_(torch.randn(net.tables.shape, generator=g, device=DEV) * 30.0)
    env = VecGame(n, device=DEV, seed=7)
    env.reset()
    greedy = afterstate_policy(None)
    for t in range(150):
        env.step(greedy(env.boards, t), auto_reset=True)
    boards = env.boards.clone()
    a, q, legal = net.search(boards, 2)
    a1, after, v, r, legal1 = net.act(boards)
    unfused = unfused_search(net)
    ua, uq = unfused(boards)
    fin = torch.isfinite(q)
    rel = ((uq.T[fin] - q[fin]).abs() / q[fin].abs().clamp(min=1.0)).max()
    from rein48_amd.moves import afterstates
    af, _, lg = afterstates(boards)
    ok = ((lg.unsqueeze(0) >> torch.arange(4, device=DEV).view(4, 1)) & 1) != 0
    children = 2 * int(((af == 0) & ok.unsqueeze(2)).sum())
    res = {"layout": layout, "boards": n, "tuples": net.m, "length": net.L, "children": children,
           "children_per_board": children / n, "unfused_actions_equal_fraction": float((ua == a).float().mean()),
           "unfused_q_max_rel_diff": float(rel), "depth2_differs_from_act_fraction": float((a != a1).float().mean())}
    for name, fn in (("search_depth2", lambda: net.search(boards, 2, a, q, legal)),
                     ("search_depth1", lambda: net.search(boards, 1, a, q, legal)),
                     ("act", lambda: net.act(boards, a1, after, v, r, legal1)),
                     ("search_unfused", lambda: unfused(boards))):
        med, lo, hi = event_ms(fn)
        res[name] = {"ms": med, "ms_min": lo, "ms_max": hi}
    res["search_depth2"]["children_per_s"] = children / (res["search_depth2"]["ms"] * 1e-3)
    res["unfused_over_fused"] = res["search_unfused"]["ms"] / res["search_depth2"]["ms"]
    res["fused_over_act"] = res["search_depth2"]["ms"] / res["act"]["ms"]
    del net
    torch.cuda.empty_cache()
    return res


def search_scores(layout, n_boards, steps, eval_seed=13, episodes=4096):
    tr = NTupleTrainer(NTupleConfig(n_boards=n_boards, layout=layout, alpha=0.25, seed=0), device=DEV)
    for _ in range(steps):
        tr.train_step()
    torch.cuda.synchronize()
    out = {"layout": layout, "train_boards": n_boards, "train_steps": steps, "alpha": 0.25, "eval_seed": eval_seed}
    for depth in (1, 2):
        t0 = time.perf_counter()
        ev = play_episodes(tr.policy(depth=depth), episodes, device=DEV, seed=eval_seed, return_scores=True)
        sc = ev.pop("scores").numpy()
        ev["score_std"] = float(sc.std(ddof=1))
        ev["eval_seconds"] = time.perf_counter() - t0
        out["depth%d" % depth] = ev
    se = (out["depth1"]["score_std"] ** 2 / episodes + out["depth2"]["score_std"] ** 2 / episodes) ** 0.5
    out["difference_in_standard_errors"] = (out["depth2"]["mean_score"] - out["depth1"]["mean_score"]) / se
    del tr
    torch.cuda.empty_cache()
    return out


def alternated_ms(fns, warmup=5, windows=7, calls=20):
    """event_ms for several callables with their windows interleaved: {name: (median, min, max)}."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / calls)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def _ms(t):
    return {"ms": t[0], "ms_min": t[1], "ms_max": t[2]}


def tc_kernels(layout, n):
    td, tc = NTupleNet(layout, device=DEV), NTupleNet(layout, device=DEV, tc=True)
    g = torch.Generator(device=DEV).manual_seed(1)
    td.tables.copy_(torch.randn(td.tables.shape, generator=g, device=DEV) * 30.0)
    tc.tables.copy_(td.tables)
    env = VecGame(n, device=DEV, seed=7)
    env.reset()
    greedy = afterstate_policy(None)
    for t in range(150):
        env.step(greedy(env.boards, t), auto_reset=True)
    after = td.act(env.boards.clone())[1]
    delta = torch.randn(n, generator=g, device=DEV) * 100.0
    hits = 8 * td.m * n
    td.accumulate(after, delta)
    touched = int((td.cnt != 0).sum())
    td.apply(after, 0.0)
    res = {"layout": layout, "boards": n, "tuples": td.m, "length": td.L, "hits": hits, "touched_entries": touched,
           "hits_per_touched_entry": hits / touched}
    rate, value = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    t = alternated_ms({"td": lambda: td.td_update(after, delta, 0.25), "tc": lambda: tc.td_update(after, delta, 1.0),
                       "value": lambda: td.value(after, out=value), "tc_rate": lambda: tc.tc_rate(after, out=rate)})
    res["accumulate_apply"], res["accumulate_apply_tc"] = _ms(t["td"]), _ms(t["tc"])
    res["value"], res["tc_rate"] = _ms(t["value"]), _ms(t["tc_rate"])
    res["mean_tc_rate_after_timing"] = float(tc.tc_rate(after).mean())
    med, lo, hi = event_ms(lambda: td.accumulate(after, delta))     # sums grow; the integer adds cost the same
    td.acc.zero_()
    td.cnt.zero_()
    res["accumulate"] = {"ms": med, "ms_min": lo, "ms_max": hi}
    res["apply"] = {"ms": max(t["td"][0] - med, 1e-6), "derived": "accumulate_apply - accumulate"}
    res["apply_tc"] = {"ms": max(t["tc"][0] - med, 1e-6), "derived": "accumulate_apply_tc - accumulate"}
    res["apply_tc_over_apply"] = res["apply_tc"]["ms"] / res["apply"]["ms"]
    res["pair_tc_over_td"] = t["tc"][0] / t["td"][0]
    del td, tc
    torch.cuda.empty_cache()
    return res


def tc_train_step(layout, n, frozen):
    """frozen: alpha 0 for both, so the tables stay zero, both trainers play the same greedy-merge
    games from the same seed and every pair of windows sees the same boards -- the like-for-like
    cost of the step. Otherwise the recipes' alphas (0.25 / 1.0): the two then play different games,
    and the share of hot entries (patterns of empty cells) differs with them."""
    trs = {"td": NTupleTrainer(NTupleConfig(n_boards=n, layout=layout, alpha=0.0 if frozen else 0.25, seed=3), device=DEV),
           "tc": NTupleTrainer(NTupleConfig(n_boards=n, layout=layout, alpha=0.0 if frozen else 1.0, seed=3, tc=True),
                               device=DEV)}
    t = alternated_ms({k: tr.train_step for k, tr in trs.items()}, warmup=20)
    same = bool(torch.equal(trs["td"].env.boards, trs["tc"].env.boards))
    res = {"layout": layout, "boards": n, "frozen_tables": frozen, "same_boards_at_the_end": same,
           "train_step_td": _ms(t["td"]), "train_step_tc": _ms(t["tc"]),
           "tc_over_td": t["tc"][0] / t["td"][0], "env_steps_per_s_td": n / (t["td"][0] * 1e-3),
           "env_steps_per_s_tc": n / (t["tc"][0] * 1e-3)}
    del trs
    torch.cuda.empty_cache()
    return res


def tc_scores(layout, n_boards, steps, eval_seed=13, episodes=4096):
    out = {"layout": layout, "train_boards": n_boards, "train_steps": steps, "eval_seed": eval_seed, "episodes": episodes}
    for name, alpha, tc in (("td", 0.25, False), ("tc", 1.0, True)):
        tr = NTupleTrainer(NTupleConfig(n_boards=n_boards, layout=layout, alpha=alpha, seed=0, tc=tc), device=DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.train_step()
        torch.cuda.synchronize()
        row = {"alpha": alpha, "tc": tc, "train_seconds": time.perf_counter() - t0}
        if tc:
            row["mean_tc_rate_on_env_boards"] = float(tr.net.tc_rate(tr.env.boards).mean())
        for depth in (1, 2):
            ev = play_episodes(tr.policy(depth=depth), episodes, device=DEV, seed=eval_seed, return_scores=True)
            sc = ev.pop("scores").numpy()
            ev["score_std"] = float(sc.std(ddof=1))
            ev["standard_error"] = ev["score_std"] / episodes ** 0.5
            row["depth%d" % depth] = ev
        out[name] = row
        del tr
        torch.cuda.empty_cache()
    for depth in ("depth1", "depth2"):
        a, b = out["tc"][depth], out["td"][depth]
        se = (a["standard_error"] ** 2 + b["standard_error"] ** 2) ** 0.5
        out[depth + "_tc_minus_td_in_standard_errors"] = (a["mean_score"] - b["mean_score"]) / se
        out[depth + "_tc_over_td"] = a["mean_score"] / b["mean_score"]
    return out


def main_tc(args):
    out = {"device": torch.cuda.get_device_name(0), "kernels": [], "train_step": [], "scores": []}
    for layout in ("lines-squares", "4x6"):
        for n in (int(s) for s in (args.sizes or "65536,1048576").split(",")):
            r = tc_kernels(layout, n)
            out["kernels"].append(r)
            print(json.dumps(r), flush=True)
            for frozen in (True, False):
                r = tc_train_step(layout, n, frozen)
                out["train_step"].append(r)
                print(json.dumps(r), flush=True)
    if args.scores:
        for layout, n_boards, steps, episodes, seed in (("lines-squares", 1024, 1000, 512, 1), ("lines-squares", 1024, 2000, 4096, 13),
                                                        ("4x6", 1024, 2000, 4096, 13), ("4x6", 4096, 10000, 4096, 13)):
            r = tc_scores(layout, n_boards, steps, eval_seed=seed, episodes=episodes)
            out["scores"].append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "exp_ntuple_tc.json"), "w") as f:
            json.dump(out, f, indent=1)


def running_boards(n):
    env = VecGame(n, device=DEV, seed=7)
    env.reset()
    greedy = afterstate_policy(None)
    for t in range(150):
        env.step(greedy(env.boards, t), auto_reset=True)
    return env.boards.clone()


def search3_of_library(path, net):
    """r48_ntuple_search3 of another build of the library, on net's tables."""
    import ctypes as C
    from rein48_amd import _lib
    f = C.CDLL(path).r48_ntuple_search3
    f.restype, f.argtypes = _lib.SIGNATURES["r48_ntuple_search3"]

    def search3(boards, actions, q, legal):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(f(_lib.ptr(boards), boards.shape[0], *net._lay(), _lib.ptr(net.tables), _lib.ptr(actions), _lib.ptr(q),
                     _lib.ptr(legal), stream))
    return search3


def search3_kernels(layout, n, ab_lib=None):
    net = NTupleNet(layout, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    net.tables.copy_(torch.randn(net.tables.shape, generator=g, device=DEV) * 30.0)
    boards = running_boards(n)
    a, q, legal = net.search3(boards)
    a2, q2, legal2 = net.search(boards, 2)

    def leaves(kids):                                                   # best_2 of the root's children
        _, qk, lg = net.search(kids, 2)
        return torch.where(lg != 0, qk.max(dim=1).values, torch.zeros_like(qk[:, 0]))
    unfused = unfused_search(net, leaves)
    ua, uq = unfused(boards)
    fin = torch.isfinite(q)
    rel = ((uq.T[fin] - q[fin]).abs() / q[fin].abs().clamp(min=1.0)).max()
    from rein48_amd.moves import afterstates
    af, _, lg = afterstates(boards)
    ok = ((lg.unsqueeze(0) >> torch.arange(4, device=DEV).view(4, 1)) & 1) != 0
    children = 2 * int(((af == 0) & ok.unsqueeze(2)).sum())
    res = {"layout": layout, "boards": n, "tuples": net.m, "length": net.L, "children": children,
           "children_per_board": children / n, "unfused_actions_equal_fraction": float((ua == a).float().mean()),
           "unfused_q_max_rel_diff": float(rel), "depth3_differs_from_depth2_fraction": float((a != a2).float().mean())}
    fns = {"search3": lambda: net.search3(boards, a, q, legal), "search_depth2": lambda: net.search(boards, 2, a2, q2, legal2),
           "search3_unfused": lambda: unfused(boards)}
    for path in (ab_lib or "").split(","):
        if not path:
            continue
        name = "search3_" + os.path.splitext(os.path.basename(path))[0]
        other = search3_of_library(path, net)
        ab, qb, lb = torch.empty_like(a), torch.empty_like(q), torch.empty_like(legal)
        other(boards, ab, qb, lb)
        res[name + "_bit_equal"] = bool(torch.equal(qb.view(torch.int32), q.view(torch.int32)) and torch.equal(ab, a) and
                                        torch.equal(lb, legal))
        fns[name] = lambda other=other, ab=ab, qb=qb, lb=lb: other(boards, ab, qb, lb)
    for name, t in alternated_ms(fns).items():
        res[name] = _ms(t)
    res["search3"]["children_per_s"] = children / (res["search3"]["ms"] * 1e-3)
    res["unfused_over_fused"] = res["search3_unfused"]["ms"] / res["search3"]["ms"]
    res["search3_over_depth2"] = res["search3"]["ms"] / res["search_depth2"]["ms"]
    del net
    torch.cuda.empty_cache()
    return res


def search3_scores(layout, n_boards, steps, alpha=0.25, tc=False, eval_seed=13, episodes=4096):
    tr = NTupleTrainer(NTupleConfig(n_boards=n_boards, layout=layout, alpha=alpha, seed=0, tc=tc), device=DEV)
    for _ in range(steps):
        tr.train_step()
    torch.cuda.synchronize()
    out = {"layout": layout, "train_boards": n_boards, "train_steps": steps, "alpha": alpha, "tc": tc,
           "eval_seed": eval_seed, "episodes": episodes}
    for depth in (2, 3):
        t0 = time.perf_counter()
        ev = play_episodes(tr.policy(depth=depth), episodes, device=DEV, seed=eval_seed, return_scores=True)
        sc = ev.pop("scores").numpy()
        ev["score_std"] = float(sc.std(ddof=1))
        ev["standard_error"] = ev["score_std"] / episodes ** 0.5
        ev["eval_seconds"] = time.perf_counter() - t0
        out["depth%d" % depth] = ev
    se = (out["depth2"]["standard_error"] ** 2 + out["depth3"]["standard_error"] ** 2) ** 0.5
    out["difference_in_standard_errors"] = (out["depth3"]["mean_score"] - out["depth2"]["mean_score"]) / se
    del tr
    torch.cuda.empty_cache()
    return out


def main_search3(args):
    out = {"device": torch.cuda.get_device_name(0), "ab_lib": args.ab_lib, "kernels": [], "scores": []}

    def save():
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "exp_ntuple_search3.json"), "w") as f:
                json.dump(out, f, indent=1)
    for layout in ("lines-squares", "4x6"):
        for n in (int(s) for s in (args.sizes or "256,4096,16384").split(",")):
            r = search3_kernels(layout, n, args.ab_lib)
            out["kernels"].append(r)
            print(json.dumps(r), flush=True)
    save()
    if args.scores:
        for layout, n_boards, steps, alpha, tc, seed, episodes in (
                ("lines-squares", 1024, 1000, 0.25, False, 1, 512), ("lines-squares", 1024, 2000, 0.25, False, 13, args.episodes),
                ("4x6", 1024, 2000, 0.25, False, 13, args.episodes), ("4x6", 4096, 10000, 1.0, True, 13, args.episodes)):
            r = search3_scores(layout, n_boards, steps, alpha, tc, seed, episodes)
            out["scores"].append(r)
            print(json.dumps(r), flush=True)
            save()


RULES_D3 = (2, 4, 6, 8, 16)


def rules_of(max_d4):
    """{name: rule}: the depth-2/3 mixes, then depth 4 on the crowded boards over depth 3."""
    rules = {"d3<=%d" % d3: NTupleNet.depth_rule(d3) for d3 in RULES_D3}
    rules.update({"3,d4<=%d" % d4: NTupleNet.depth_rule(16, d4) for d4 in range(max_d4 + 1)})
    return rules


def random_net(layout):
    net = NTupleNet(layout, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    net.tables.copy_(torch.randn(net.tables.shape, generator=g, device=DEV) * 30.0)
    return net


def ruled_of_library(path, net):
    """r48_ntuple_search_ruled of another build of the library, on net's tables."""
    import ctypes as C
    from rein48_amd import _lib
    f = C.CDLL(path).r48_ntuple_search_ruled
    f.restype, f.argtypes = _lib.SIGNATURES["r48_ntuple_search_ruled"]

    def search_ruled(boards, rule, actions, q, legal, depth):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(f(_lib.ptr(boards), boards.shape[0], *net._lay(), _lib.ptr(net.tables), (C.c_uint8 * 17)(*rule),
                     _lib.ptr(actions), _lib.ptr(q), _lib.ptr(legal), _lib.ptr(depth), stream))
    return search_ruled


def ruled_all3(layout, n, ab_lib=None):
    """search_ruled under the all-3 rule against search3: the cost of the shared body."""
    net = random_net(layout)
    boards = running_boards(n)
    a, q, legal = net.search3(boards)
    ar, qr, lr, dr = net.search_ruled(boards, (3,) * 17)
    res = {"layout": layout, "boards": n,
           "bit_equal": bool(torch.equal(qr.view(torch.int32), q.view(torch.int32)) and torch.equal(ar, a) and
                             torch.equal(lr, legal) and bool((dr == 3).all()))}
    fns = {"search3": lambda: net.search3(boards, a, q, legal),
           "ruled_all3": lambda: net.search_ruled(boards, (3,) * 17, ar, qr, lr, dr)}
    for path in (ab_lib or "").split(","):
        if not path:
            continue
        name = "ruled_all3_" + os.path.splitext(os.path.basename(path))[0]
        other = ruled_of_library(path, net)
        outs = tuple(torch.empty_like(x) for x in (ar, qr, lr, dr))
        other(boards, (3,) * 17, *outs)
        res[name + "_bit_equal"] = bool(torch.equal(outs[1].view(torch.int32), q.view(torch.int32)) and torch.equal(outs[0], a))
        fns[name] = lambda other=other, outs=outs: other(boards, (3,) * 17, *outs)
    for name, t in alternated_ms(fns).items():
        res[name] = _ms(t)
    res["ruled_over_search3"] = res["ruled_all3"]["ms"] / res["search3"]["ms"]
    res["outside_the_spread"] = bool(res["ruled_all3"]["ms_min"] > res["search3"]["ms_max"] or
                                     res["ruled_all3"]["ms_max"] < res["search3"]["ms_min"])
    return res


def ruled_by_rule(layout, max_d4=4, n=4096, n_big=65536):
    """Time per call by rule at n boards of running games, the depth shares, the longest launch at n_big."""
    net = random_net(layout)
    boards, big = running_boards(n), running_boards(n_big)
    blanks = (boards == 0).sum(1)
    res = {"layout": layout, "boards": n, "boards_big": n_big,
           "blanks_hist": {int(k): float(v) for k, v in enumerate(torch.bincount(blanks, minlength=17).double() / n) if v > 0},
           "rules": {}}
    outs = net.search_ruled(boards, (2,) * 17)
    outs_big = net.search_ruled(big, (2,) * 17)
    fns = {"search2": lambda: net.search(boards, 2, *outs[:3]), "search3": lambda: net.search3(boards, *outs[:3])}
    big_fns = {"search2": lambda: net.search(big, 2, *outs_big[:3]), "search3": lambda: net.search3(big, *outs_big[:3])}
    rules = rules_of(max_d4)
    for name, rule in rules.items():
        fns[name] = lambda rule=rule: net.search_ruled(boards, rule, *outs)
        big_fns[name] = lambda rule=rule: net.search_ruled(big, rule, *outs_big)
    times = alternated_ms(fns, warmup=2, windows=7, calls=5)
    for name in fns:
        row = _ms(times[name])
        rule = rules.get(name, (2,) * 17 if name == "search2" else (3,) * 17)
        d = net.search_ruled(boards, rule, *outs)[3]
        row["share_by_depth"] = {int(k): float(v) for k, v in enumerate(torch.bincount(d.long(), minlength=5).double() / n) if v > 0}
        launches = []
        for _ in range(6):                                               # the first is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            big_fns[name]()
            e1.record()
            torch.cuda.synchronize()
            launches.append(e0.elapsed_time(e1))
        row["longest_launch_ms_big"] = max(launches[1:])
        row["rule"] = list(rule)
        res["rules"][name] = row
    return res


def ruled_scores(layout, n_boards, steps, alpha, tc, eval_seed, episodes, max_d4):
    tr = NTupleTrainer(NTupleConfig(n_boards=n_boards, layout=layout, alpha=alpha, seed=0, tc=tc, fused=True), device=DEV)
    for _ in range(steps):
        tr.train_step()
    torch.cuda.synchronize()
    out = {"layout": layout, "train_boards": n_boards, "train_steps": steps, "alpha": alpha, "tc": tc,
           "eval_seed": eval_seed, "episodes": episodes, "policies": {}}
    policies = {"depth2": tr.policy(depth=2), "depth3": tr.policy(depth=3)}
    rules = rules_of(max_d4)
    policies.update({name: tr.policy(rule=rule) for name, rule in rules.items() if name != "d3<=16"})
    for name, policy in policies.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev = play_episodes(policy, episodes, device=DEV, seed=eval_seed, return_scores=True)
        torch.cuda.synchronize()
        sc = ev.pop("scores").numpy()
        ev["score_std"] = float(sc.std(ddof=1))
        ev["standard_error"] = ev["score_std"] / episodes ** 0.5
        ev["eval_seconds"] = time.perf_counter() - t0
        ev.pop("max_tile_exponent_hist")
        out["policies"][name] = ev
        print(json.dumps({layout: name, "mean_score": ev["mean_score"], "se": ev["standard_error"],
                          "eval_seconds": ev["eval_seconds"]}), flush=True)
    base = out["policies"]["depth3"]
    for name, ev in out["policies"].items():
        se = (ev["standard_error"] ** 2 + base["standard_error"] ** 2) ** 0.5
        ev["over_depth3_in_standard_errors"] = (ev["mean_score"] - base["mean_score"]) / se
        ev["seconds_over_depth3"] = ev["eval_seconds"] / base["eval_seconds"]
    del tr
    torch.cuda.empty_cache()
    return out


def main_ruled(args):
    out = {"device": torch.cuda.get_device_name(0), "all3": [], "by_rule": [], "scores": []}

    def save():
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "exp_ntuple_ruled.json"), "w") as f:
                json.dump(out, f, indent=1)
    for layout in ("lines-squares", "4x6"):
        for n in (int(s) for s in (args.sizes or "256,4096,16384").split(",")):
            r = ruled_all3(layout, n, args.ab_lib)
            out["all3"].append(r)
            print(json.dumps(r), flush=True)
    save()
    for layout in ("lines-squares", "4x6"):
        r = ruled_by_rule(layout)
        out["by_rule"].append(r)
        print(json.dumps(r), flush=True)
        save()
    if args.scores:
        for layout, n_boards, steps, alpha, tc, seed, episodes in (
                ("lines-squares", 1024, 1000, 0.25, False, 1, 512), ("lines-squares", 1024, 2000, 0.25, False, 13, args.episodes),
                ("4x6", 4096, 10000, 1.0, True, 13, args.episodes)):
            r = ruled_scores(layout, n_boards, steps, alpha, tc, seed, episodes, args.max_d4)
            out["scores"].append(r)
            print(json.dumps(r), flush=True)
            save()


def alternated_host_ms(fns, warmup=20, windows=7, calls=20):
    """alternated_ms on the host clock: every window is `calls` calls and a synchronise, as a
    training loop pays for them -- ({name: the windows' times in order}, {name: the median time
    until the last call returned, before the synchronise: what the host spends enqueueing}) in ms
    per call."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out, enq = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / calls * 1e3)
            enq[k].append((t1 - t0) / calls * 1e3)
    return out, {k: statistics.median(v) for k, v in enq.items()}


def fused_windows(w):
    """The comparison of one set of alternated windows {"unfused": [...], "fused": [...]}: medians,
    the larger of the two min-max spreads next to the median saving (the spread holds whatever
    changes from window to window, the games' progress included: all boards start from reset
    together), and the differences within the pairs of windows, which saw the same boards."""
    u, f = w["unfused"], w["fused"]
    mu, mf = statistics.median(u), statistics.median(f)
    spread = max(max(u) - min(u), max(f) - min(f))
    pairs = [a - b for a, b in zip(u, f)]
    return {"unfused": {"ms": mu, "ms_min": min(u), "ms_max": max(u), "windows_ms": u},
            "fused": {"ms": mf, "ms_min": min(f), "ms_max": max(f), "windows_ms": f},
            "unfused_over_fused": mu / mf, "saved_ms": mu - mf, "largest_min_max_spread_ms": spread,
            "saving_exceeds_spread": mu - mf > spread, "not_slower_by_more_than_spread": mf - mu <= spread,
            "paired_saving_ms": {"median": statistics.median(pairs), "min": min(pairs), "max": max(pairs)},
            "fused_faster_in_pairs": sum(p > 0 for p in pairs), "pairs": len(pairs)}


def fused_train_step(layout, n, tc):
    """A fused and an unfused trainer from the same seed with the recipe's alpha: bit-identical, so
    both see the same boards at the same step of every pair of windows."""
    alpha = 1.0 if tc else 0.25
    trs = {k: NTupleTrainer(NTupleConfig(n_boards=n, layout=layout, alpha=alpha, seed=3, tc=tc, fused=k == "fused"), device=DEV)
           for k in ("unfused", "fused")}
    w, enq = alternated_host_ms({k: tr.train_step for k, tr in trs.items()})
    res = {"layout": layout, "boards": n, "tc": tc, "alpha": alpha}
    res.update(fused_windows(w))
    res.update(env_steps_per_s_unfused=n / (res["unfused"]["ms"] * 1e-3), env_steps_per_s_fused=n / (res["fused"]["ms"] * 1e-3),
               host_enqueue_ms_unfused=enq["unfused"], host_enqueue_ms_fused=enq["fused"])
    if n <= 4096:                                            # ten times longer windows, next to the prescribed ones
        res["windows_of_200_steps"] = fused_windows(alternated_host_ms({k: tr.train_step for k, tr in trs.items()}, warmup=0,
                                                                       calls=200)[0])
    u, f = trs["unfused"], trs["fused"]
    res["steps_each"] = u.updates
    res["bit_identical_at_the_end"] = bool(
        u.updates == f.updates and torch.equal(u.env.boards, f.env.boards)
        and torch.equal(u.net.tables.view(torch.int32), f.net.tables.view(torch.int32))
        and torch.equal(u.prev_value.view(torch.int32), f.prev_value.view(torch.int32)))
    del trs, u, f
    torch.cuda.empty_cache()
    return res


def fused_kernels(layout, n):
    """Device-event times of td_act against act and accumulate on the same inputs: boards of running
    games, their previous step's afterstates and values, every row valid. The sums in the scratch
    grow over the timed calls; the integer adds cost the same."""
    net = NTupleNet(layout, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    net.tables.copy_(torch.randn(net.tables.shape, generator=g, device=DEV) * 30.0)
    env = VecGame(n, device=DEV, seed=7)
    env.reset()
    greedy = afterstate_policy(None)
    for t in range(150):
        env.step(greedy(env.boards, t), auto_reset=True)
    a, prev_after, prev_value, r, legal = net.act(env.boards)
    prev_done = env.step(a, auto_reset=True)[2].clone()
    boards = env.boards.clone()
    prev_valid = torch.ones(n, dtype=torch.uint8, device=DEV)
    after, value = torch.empty_like(prev_after), torch.empty_like(prev_value)
    valid, delta = torch.empty_like(prev_valid), torch.empty_like(prev_value)
    net.act(boards, a, after, value, r, legal)
    delta.copy_(torch.where(prev_done != 0, torch.zeros_like(value), r.float() + value) - prev_value)

    def pair():
        net.act(boards, a, after, value, r, legal)
        net.accumulate(prev_after, delta, prev_valid)
    def td_act():
        net.td_act(boards, prev_after, prev_value, prev_done, prev_valid, a, after, value, r, legal, valid, delta)

    def glue():                                              # the unfused step's torch kernels between act and accumulate
        target = torch.where(prev_done != 0, torch.zeros_like(value), r.float() + value)
        torch.sub(target, prev_value, out=delta)

    def update():                                            # the fused step's first two launches: the scratch is zero again
        td_act()
        net.apply(prev_after, 0.25 / (8.0 * net.m), prev_valid)
    t = alternated_ms({"td_act": td_act, "act_accumulate": pair, "act": lambda: net.act(boards, a, after, value, r, legal),
                       "accumulate": lambda: net.accumulate(prev_after, delta, prev_valid), "torch_glue": glue})
    net.acc.zero_()
    net.cnt.zero_()
    acts = a.clone()                                         # the moves of the boards the env holds now
    t.update(alternated_ms({"td_act_apply": update, "env_step": lambda: env.step(acts, auto_reset=True)}))
    res = {"layout": layout, "boards": n, "tuples": net.m, "length": net.L, "hits": 8 * net.m * n}
    res.update({k: _ms(v) for k, v in t.items()})
    res["act_accumulate_over_td_act"] = t["act_accumulate"][0] / t["td_act"][0]
    res["td_act_minus_accumulate_ms"] = t["td_act"][0] - t["accumulate"][0]
    res["apply"] = {"ms": max(t["td_act_apply"][0] - t["td_act"][0], 1e-6), "derived": "td_act_apply - td_act"}
    res["three_kernels_ms"] = t["td_act_apply"][0] + t["env_step"][0]
    del net
    torch.cuda.empty_cache()
    return res


def fused_budget(layout="4x6", n_boards=4096, steps=10000, eval_seed=13, episodes=4096):
    """What the saved time buys: the unfused TC recipe's wall time for `steps` steps, the number of
    fused steps that fit in the same time, and the depth-1 score each reaches."""
    def evaluate(tr, row):
        ev = play_episodes(tr.policy(depth=1), episodes, device=DEV, seed=eval_seed, return_scores=True)
        sc = ev.pop("scores").numpy()
        ev["score_std"] = float(sc.std(ddof=1))
        ev["standard_error"] = ev["score_std"] / episodes ** 0.5
        row["depth1"] = ev
        return row
    out = {"layout": layout, "train_boards": n_boards, "alpha": 1.0, "tc": True, "eval_seed": eval_seed, "episodes": episodes}
    tr = NTupleTrainer(NTupleConfig(n_boards=n_boards, layout=layout, alpha=1.0, seed=0, tc=True), device=DEV)
    tr.train_steps(200)                                      # code objects loaded, clocks up; part of the budget's steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train_steps(steps - 200)
    torch.cuda.synchronize()
    budget = time.perf_counter() - t0
    out["unfused"] = evaluate(tr, {"train_steps": tr.updates, "timed_steps": steps - 200, "timed_seconds": budget})
    del tr
    torch.cuda.empty_cache()
    tr = NTupleTrainer(NTupleConfig(n_boards=n_boards, layout=layout, alpha=1.0, seed=0, tc=True, fused=True), device=DEV)
    tr.train_steps(200)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while True:                                              # 100 steps and a synchronise at a time, until the budget is spent
        tr.train_steps(100)
        torch.cuda.synchronize()
        spent = time.perf_counter() - t0
        if spent >= budget:
            break
    out["fused"] = evaluate(tr, {"train_steps": tr.updates, "timed_steps": tr.updates - 200, "timed_seconds": spent})
    out["fused_steps_over_unfused_steps"] = out["fused"]["timed_steps"] / out["unfused"]["timed_steps"]
    a, b = out["fused"]["depth1"], out["unfused"]["depth1"]
    se = (a["standard_error"] ** 2 + b["standard_error"] ** 2) ** 0.5
    out["fused_minus_unfused_in_standard_errors"] = (a["mean_score"] - b["mean_score"]) / se
    del tr
    torch.cuda.empty_cache()
    return out


def main_fused(args):
    out = {"device": torch.cuda.get_device_name(0), "train_step": [], "kernels": [], "budget": []}

    def save():
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "exp_ntuple_fused.json"), "w") as f:
                json.dump(out, f, indent=1)
    sizes = [int(s) for s in (args.sizes or "1024,4096,65536,1048576").split(",")]
    for layout in ("lines-squares", "4x6"):
        for n in sizes:
            for tc in (False, True):
                r = fused_train_step(layout, n, tc)
                out["train_step"].append(r)
                print(json.dumps(r), flush=True)
            r = fused_kernels(layout, n)
            out["kernels"].append(r)
            print(json.dumps(r), flush=True)
            save()
    if args.scores:
        r = fused_budget(episodes=args.episodes)
        out["budget"].append(r)
        print(json.dumps(r), flush=True)
        save()


def timed(fn):
    """(result, wall seconds ending in a synchronise, device milliseconds between two events around the call)."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0, e0.elapsed_time(e1)


def play_of_library(path, net):
    """NTupleNet.play through r48_ntuple_play of another build of the library (-DR48_NT_PLAY_LANES=4)."""
    import ctypes as C
    from rein48_amd import _lib
    f = C.CDLL(path).r48_ntuple_play
    f.restype, f.argtypes = _lib.SIGNATURES["r48_ntuple_play"]

    def play(env, n_steps, depth, length, gain, done):
        step, reset = env.counters
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(f(_lib.ptr(env.boards), env.n, *net._lay(), _lib.ptr(net.tables), depth, n_steps, env.seed,
                     env.board_offset, step, _lib.ptr(length), _lib.ptr(gain), _lib.ptr(done), stream))
        env.counters = ((step + n_steps) & 0xFFFFFFFF, reset)
    return play


def play_step_times(net, n, depth, k=20, ab_lib=None):
    """Device time per step on n live boards (running games): play's k steps in one launch against k x
    (act or search, env.step), alternated windows; both start every call from the same boards and
    step counter (one 16n-byte copy each, inside the window). With ab_lib, the other build's play too,
    its boards compared bit for bit."""
    start = running_boards(n)
    env = VecGame(n, device=DEV, seed=7)
    length, gain = (torch.zeros(n, dtype=torch.int32, device=DEV) for _ in range(2))
    done = torch.zeros(n, dtype=torch.uint8, device=DEV)
    policy = net.policy(depth)

    def begin():
        env.boards.copy_(start)
        env.counters = (150, 0)

    def fused():
        begin()
        net.play(env, k, depth, length, gain, done)

    def composed():
        begin()
        for t in range(k):
            env.step(policy(env.boards, t))
    fns = {"play": fused, "composed": composed}
    res = {"boards": n, "depth": depth, "steps_per_call": k}
    composed()
    want = env.boards.clone()
    fused()
    res["play_equals_composed"] = bool(torch.equal(env.boards, want))
    res["alive_after_the_call"] = float((done == 0).float().mean())
    if ab_lib:
        other = play_of_library(ab_lib, net)

        def fused_other():
            begin()
            other(env, k, depth, length, gain, done)
        fused_other()
        res["other_build_equals_composed"] = bool(torch.equal(env.boards, want))
        fns["play_other_build"] = fused_other
    for name, t in alternated_ms(fns, warmup=3, windows=7, calls=5).items():
        res[name] = {"us_per_step": t[0] / k * 1e3, "us_min": t[1] / k * 1e3, "us_max": t[2] / k * 1e3}
    res["composed_over_play"] = res["composed"]["us_per_step"] / res["play"]["us_per_step"]
    return res


def play_launch_times(net, n, depth, chunks, ab_lib=None):
    """The device time of single play launches of `chunk` steps at n boards, games from reset: the
    first launch (every board alive throughout, the most children at depth 2) and the longest of the
    first four."""
    rows = []
    plays = {"play": lambda env, k, le, ga, do: net.play(env, k, depth, le, ga, do)}
    if ab_lib:
        other = play_of_library(ab_lib, net)
        plays["play_other_build"] = lambda env, k, le, ga, do: other(env, k, depth, le, ga, do)
    for chunk in chunks:
        row = {"boards": n, "depth": depth, "chunk": chunk}
        for name, play in plays.items():
            env = VecGame(n, device=DEV, seed=13)
            env.reset()
            length, gain = (torch.zeros(n, dtype=torch.int32, device=DEV) for _ in range(2))
            done = torch.zeros(n, dtype=torch.uint8, device=DEV)
            ms = [timed(lambda: play(env, chunk, length, gain, done))[2] for _ in range(4)]
            row[name] = {"first_launch_ms": ms[0], "longest_of_four_ms": max(ms), "launches_ms": ms,
                         "alive_after_four": float((done == 0).float().mean())}
        rows.append(row)
    return rows


def play_episode_times(net, depth, episodes, eval_seed, ab_lib=None):
    """Whole episodes to the end: NTupleNet.play_episodes against evaluate.play_episodes on the same
    net in the same process, each run twice (the first run of each loads code objects), wall seconds
    ending in a synchronise and device milliseconds between events around the call."""
    row = {"depth": depth, "episodes": episodes, "eval_seed": eval_seed}
    runs = {"play_episodes": lambda: net.play_episodes(episodes, seed=eval_seed, depth=depth, return_scores=True),
            "evaluate": lambda: play_episodes(net.policy(depth), episodes, device=DEV, seed=eval_seed, return_scores=True)}
    scores = {}
    for name, fn in runs.items():
        fn()
        ev, wall, dev_ms = timed(fn)
        scores[name] = ev.pop("scores")
        ev.update(wall_seconds=wall, device_ms=dev_ms)
        row[name] = ev
    row["scores_bit_equal"] = bool(torch.equal(scores["play_episodes"], scores["evaluate"]))
    row["wall_evaluate_over_play"] = row["evaluate"]["wall_seconds"] / row["play_episodes"]["wall_seconds"]
    if ab_lib:                                                # the other build's mapping, the same chunks
        from rein48_amd.ntuple import PLAY_CHUNK
        other = play_of_library(ab_lib, net)

        def to_the_end():
            env = VecGame(episodes, device=DEV, seed=eval_seed)
            env.reset()
            length, gain = (torch.zeros(episodes, dtype=torch.int32, device=DEV) for _ in range(2))
            done = torch.zeros(episodes, dtype=torch.uint8, device=DEV)
            for _ in range(0, 20000, PLAY_CHUNK[depth]):
                other(env, PLAY_CHUNK[depth], depth, length, gain, done)
                if bool((done != 0).all()):
                    break
            return env.score().double().cpu()
        to_the_end()
        sc, wall, dev_ms = timed(to_the_end)
        row["play_other_build"] = {"wall_seconds": wall, "device_ms": dev_ms,
                                   "scores_bit_equal": bool(torch.equal(sc, scores["evaluate"]))}
    return row


def main_play(args):
    """--play [--ab-lib SO]: whole games in one launch (r48_ntuple_play) against the Python loop of
    evaluate.play_episodes, on the tables of the recorded recipes."""
    out = {"device": torch.cuda.get_device_name(0), "ab_lib": args.ab_lib, "recipes": []}

    def save():
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "exp_ntuple_play.json"), "w") as f:
                json.dump(out, f, indent=1)
    for layout, n_boards, steps, alpha, tc in (("lines-squares", 1024, 2000, 0.25, False), ("4x6", 4096, 10000, 1.0, True)):
        tr = NTupleTrainer(NTupleConfig(n_boards=n_boards, layout=layout, alpha=alpha, seed=0, tc=tc), device=DEV)
        tr.train_steps(steps)
        torch.cuda.synchronize()
        rec = {"layout": layout, "train_boards": n_boards, "train_steps": steps, "alpha": alpha, "tc": tc,
               "episodes": [], "per_step": [], "launches": []}
        out["recipes"].append(rec)
        for depth in (1, 2):
            r = play_episode_times(tr.net, depth, args.episodes, 13, args.ab_lib if depth == 1 else None)
            rec["episodes"].append(r)
            print(json.dumps(dict(r, layout=layout)), flush=True)
            save()
        for depth in (1, 2):
            for n in (int(s) for s in (args.sizes or "4096,65536").split(",")):
                r = play_step_times(tr.net, n, depth, ab_lib=args.ab_lib if depth == 1 else None)
                rec["per_step"].append(r)
                print(json.dumps(dict(r, layout=layout)), flush=True)
            for r in play_launch_times(tr.net, 65536, depth, (250, 500, 1000, 2000) if depth == 1 else (25, 50, 100, 200),
                                       args.ab_lib if depth == 1 else None):
                rec["launches"].append(r)
                print(json.dumps(dict(r, layout=layout)), flush=True)
            save()
        del tr
        torch.cuda.empty_cache()


def play_ruled_of_library(path, net):
    """NTupleNet.play_ruled through r48_ntuple_play_ruled of another build of the library."""
    import ctypes as C
    from rein48_amd import _lib
    f = C.CDLL(path).r48_ntuple_play_ruled
    f.restype, f.argtypes = _lib.SIGNATURES["r48_ntuple_play_ruled"]

    def play_ruled(env, n_steps, rule, length, gain, done):
        step, reset = env.counters
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(f(_lib.ptr(env.boards), env.n, *net._lay(), _lib.ptr(net.tables), (C.c_uint8 * 17)(*rule), n_steps,
                     env.seed, env.board_offset, step, _lib.ptr(length), _lib.ptr(gain), _lib.ptr(done), stream))
        env.counters = ((step + n_steps) & 0xFFFFFFFF, reset)
    return play_ruled


def play_ruled_episode_times(net, name, rule, episodes, eval_seed, timed_runs):
    """Whole episodes to the end: play_episodes (play_ruled in chunks) against evaluate.play_episodes (the
    Python loop) on the same net in the same process: a first run of each, then timed_runs timed ones."""
    from rein48_amd.ntuple import ruled_chunk
    row = {"rule": name, "episodes": episodes, "eval_seed": eval_seed, "chunk": ruled_chunk(max(rule), episodes)}
    if name == "depth3":                                      # as a caller asks for it: depth=3, the loop through search3
        fused, policy = (lambda: net.play_episodes(episodes, seed=eval_seed, depth=3, return_scores=True)), net.policy(3)
    else:
        fused, policy = (lambda: net.play_episodes(episodes, seed=eval_seed, rule=rule, return_scores=True)), net.policy(rule=rule)
    runs = {"play_episodes": fused,
            "evaluate": lambda: play_episodes(policy, episodes, device=DEV, seed=eval_seed, return_scores=True)}
    scores = {}
    for which, fn in runs.items():
        fn()
        walls, devs = [], []
        for _ in range(timed_runs):
            ev, wall, dev_ms = timed(fn)
            walls.append(wall)
            devs.append(dev_ms)
        scores[which] = ev.pop("scores")
        ev.update(wall_seconds=walls[0], device_ms=devs[0], wall_seconds_runs=walls)
        row[which] = ev
    row["scores_bit_equal"] = bool(torch.equal(scores["play_episodes"], scores["evaluate"]))
    row["wall_evaluate_over_play"] = row["evaluate"]["wall_seconds"] / row["play_episodes"]["wall_seconds"]
    if timed_runs > 1:
        row["a_a_spread"] = {k: max(row[k]["wall_seconds_runs"]) / min(row[k]["wall_seconds_runs"]) for k in runs}
    return row


def play_ruled_step_times(net, n, name, rule, k=20, ab_libs=()):
    """Device time per step on n boards of running games: play_ruled's k steps in one launch against k x
    (search_ruled, env.step), alternated windows; every call starts from the same boards and counter."""
    start = running_boards(n)
    env = VecGame(n, device=DEV, seed=7)
    length, gain = (torch.zeros(n, dtype=torch.int32, device=DEV) for _ in range(2))
    done = torch.zeros(n, dtype=torch.uint8, device=DEV)
    policy = net.policy(rule=rule)

    def begin():
        env.boards.copy_(start)
        env.counters = (150, 0)

    def fused():
        begin()
        net.play_ruled(env, k, rule, length, gain, done)

    def composed():
        begin()
        for t in range(k):
            env.step(policy(env.boards, t))
    fns = {"play_ruled": fused, "composed": composed}
    res = {"boards": n, "rule": name, "steps_per_call": k}
    composed()
    want = env.boards.clone()
    fused()
    res["play_equals_composed"] = bool(torch.equal(env.boards, want))
    res["alive_after_the_call"] = float((done == 0).float().mean())
    for path in ab_libs:
        other = play_ruled_of_library(path, net)
        tag = "play_ruled_" + os.path.splitext(os.path.basename(path))[0]

        def fused_other(other=other):
            begin()
            other(env, k, rule, length, gain, done)
        fused_other()
        res[tag + "_equals_composed"] = bool(torch.equal(env.boards, want))
        fns[tag] = fused_other
    for which, t in alternated_ms(fns, warmup=2, windows=5, calls=3).items():
        res[which] = {"us_per_step": t[0] / k * 1e3, "us_min": t[1] / k * 1e3, "us_max": t[2] / k * 1e3}
    res["composed_over_play_ruled"] = res["composed"]["us_per_step"] / res["play_ruled"]["us_per_step"]
    return res


def play_ruled_launch_times(net, n, name, rule, chunks):
    """The device time of single play_ruled launches of `chunk` steps at n boards: four consecutive
    launches from boards of running games (few blanks: where depth 4 is) and four from reset."""
    rows = []
    for chunk in chunks:
        row = {"boards": n, "rule": name, "chunk": chunk, "board_steps": n * chunk}
        for begin in ("running", "reset"):
            env = VecGame(n, device=DEV, seed=13)
            env.reset()
            if begin == "running":
                env.boards.copy_(running_boards(n))
                env.counters = (150, 0)
            length, gain = (torch.zeros(n, dtype=torch.int32, device=DEV) for _ in range(2))
            done = torch.zeros(n, dtype=torch.uint8, device=DEV)
            ms = [timed(lambda: net.play_ruled(env, chunk, rule, length, gain, done))[2] for _ in range(4)]
            row[begin] = {"longest_of_four_ms": max(ms), "launches_ms": ms,
                          "alive_after_four": float((done == 0).float().mean())}
        rows.append(row)
    return rows


def play_ruled_waves_ab(net, name, rule, episodes, eval_seed, ab_libs, small_n=64):
    """The A/B of waves per board on what play_episodes does: whole episodes to the end in play_episodes'
    chunks through each build's r48_ntuple_play_ruled (a first run, then the timed one), scores compared
    bit for bit with the first build's; and single launches of play_episodes' chunk at small_n boards from
    reset, where a launch costs its steps times one board's latency."""
    from rein48_amd.ntuple import ruled_chunk
    row = {"rule": name, "episodes": episodes, "eval_seed": eval_seed, "small_n": small_n, "builds": {}}
    first = None
    for path in ab_libs:
        tag = os.path.splitext(os.path.basename(path))[0]
        other = play_ruled_of_library(path, net)

        def to_the_end(n=episodes, other=other):
            chunk = ruled_chunk(max(rule), n)
            env = VecGame(n, device=DEV, seed=eval_seed)
            env.reset()
            length, gain = (torch.zeros(n, dtype=torch.int32, device=DEV) for _ in range(2))
            done = torch.zeros(n, dtype=torch.uint8, device=DEV)
            for _ in range(0, 20000, chunk):
                other(env, chunk, rule, length, gain, done)
                if bool((done != 0).all()):
                    break
            return env.score().double().cpu()
        to_the_end()
        sc, wall, dev_ms = timed(to_the_end)
        first = sc if first is None else first
        res = {"wall_seconds": wall, "device_ms": dev_ms, "scores_equal_the_first_builds": bool(torch.equal(sc, first))}
        chunk = ruled_chunk(max(rule), small_n)
        env = VecGame(small_n, device=DEV, seed=eval_seed)
        env.reset()
        length, gain = (torch.zeros(small_n, dtype=torch.int32, device=DEV) for _ in range(2))
        done = torch.zeros(small_n, dtype=torch.uint8, device=DEV)
        ms = [timed(lambda: other(env, chunk, rule, length, gain, done))[2] for _ in range(4)]
        res["small_n_launches"] = {"chunk": chunk, "launches_ms": ms, "alive_after_four": float((done == 0).float().mean()),
                                   "mean_length": float(length.double().mean())}
        _, res["small_n_whole_seconds"], _ = timed(lambda: to_the_end(small_n))
        row["builds"][tag] = res
    return row


def main_play_ruled(args):
    """--play-ruled [--ab-lib SO[,SO...]] [--max-d4 3]: play_ruled and play_episodes at depth 3 and under
    rules against the Python loop of evaluate.play_episodes, on the tables of the recorded recipes."""
    from rein48_amd.ntuple import ruled_chunk
    ab_libs = [p for p in (args.ab_lib or "").split(",") if p]
    out = {"device": torch.cuda.get_device_name(0), "ab_libs": ab_libs, "recipes": []}
    recorded = {("lines-squares", "depth3"): 7135.3623046875, ("lines-squares", "3,d4<=1"): 7921.8720703125,
                ("lines-squares", "3,d4<=3"): 8823.54345703125, ("4x6", "depth3"): 12457.6650390625,
                ("4x6", "3,d4<=1"): 12909.06884765625, ("4x6", "3,d4<=3"): 13879.06494140625}

    def save():
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "exp_ntuple_play_ruled%s.json" % ("_waves" if args.waves_ab else "")), "w") as f:
                json.dump(out, f, indent=1)
    rules = {"depth3": (3,) * 17, "3,d4<=1": NTupleNet.depth_rule(16, 1)}
    if args.long:
        rules["3,d4<=3"] = NTupleNet.depth_rule(16, 3)
    for layout, n_boards, steps, alpha, tc in (("lines-squares", 1024, 2000, 0.25, False), ("4x6", 4096, 10000, 1.0, True)):
        tr = NTupleTrainer(NTupleConfig(n_boards=n_boards, layout=layout, alpha=alpha, seed=0, tc=tc, fused=True), device=DEV)
        tr.train_steps(steps)
        torch.cuda.synchronize()
        rec = {"layout": layout, "train_boards": n_boards, "train_steps": steps, "alpha": alpha, "tc": tc,
               "episodes": [], "per_step": [], "launches": []}
        out["recipes"].append(rec)
        if args.waves_ab:                                     # the A/B of waves per board alone
            for name, rule in rules.items():
                r = play_ruled_waves_ab(tr.net, name, rule, args.episodes, 13, ab_libs)
                rec["episodes"].append(r)
                print(json.dumps(dict(r, layout=layout)), flush=True)
                save()
            del tr
            torch.cuda.empty_cache()
            continue
        if not args.no_episodes:
            for name, rule in rules.items():
                r = play_ruled_episode_times(tr.net, name, rule, args.episodes, 13, 2 if name == "depth3" else 1)
                if args.episodes == 4096:
                    r["recorded_mean_score"] = recorded[(layout, name)]
                    r["equals_the_recorded_score"] = r["play_episodes"]["mean_score"] == recorded[(layout, name)]
                rec["episodes"].append(r)
                print(json.dumps(dict(r, layout=layout)), flush=True)
                save()
        if not args.no_episodes:                              # few episodes: one board's latency is what counts
            for episodes in (64, 512):
                for name in ("depth3", "3,d4<=1"):
                    r = play_ruled_episode_times(tr.net, name, rules[name], episodes, 13, 2)
                    rec["episodes"].append(r)
                    print(json.dumps(dict(r, layout=layout)), flush=True)
            save()
        for name in ("depth3", "3,d4<=1"):
            for n in (int(s) for s in (args.sizes or "4096,16384").split(",")):
                r = play_ruled_step_times(tr.net, n, name, rules[name], ab_libs=ab_libs)
                rec["per_step"].append(r)
                print(json.dumps(dict(r, layout=layout)), flush=True)
            save()
        for name, rule, chunks in (("all-1", (1,) * 17, (128, 256)), ("all-2", (2,) * 17, (32, 64)),
                                   ("depth3", (3,) * 17, (8, 16, 32)), ("3,d4<=1", NTupleNet.depth_rule(16, 1), (2, 4)),
                                   ("3,d4<=3", NTupleNet.depth_rule(16, 3), (1, 2, 4))):
            for r in (play_ruled_launch_times(tr.net, 4096, name, rule, chunks) +
                      play_ruled_launch_times(tr.net, 64, name, rule, (ruled_chunk(max(rule), 64),))):
                rec["launches"].append(r)
                print(json.dumps(dict(r, layout=layout)), flush=True)
            save()
        del tr
        torch.cuda.empty_cache()


def stage_kernels(layout, n, cuts):
    """value, act, search depth 2, search3 and the two update pairs on the same running boards, staged
    against unstaged, their windows interleaved."""
    nets = {"plain": NTupleNet(layout, device=DEV, tc=True), "staged": NTupleNet(layout, device=DEV, tc=True, stages=cuts)}
    g = torch.Generator(device=DEV).manual_seed(1)
    nets["plain"].tables.copy_(torch.randn(nets["plain"].tables.shape, generator=g, device=DEV) * 30.0)
    nets["staged"].tables[:] = nets["plain"].tables               # every stage alike: both play the same moves
    boards = running_boards(n)
    after = nets["plain"].act(boards)[1]
    delta = torch.randn(n, generator=g, device=DEV) * 100.0
    res = {"layout": layout, "boards": n, "cuts": list(cuts),
           "share_of_boards_above_stage_0": float((nets["staged"].stage(after) > 0).float().mean())}
    value = torch.empty(n, device=DEV)
    fns = {}
    for k, net in nets.items():
        fns["value_" + k] = lambda net=net: net.value(after, out=value)
        fns["act_" + k] = lambda net=net: net.act(boards)
        fns["search2_" + k] = lambda net=net: net.search(boards, 2)
        fns["search3_" + k] = lambda net=net: net.search3(boards)
    t = alternated_ms(fns, calls=5 if n > 8192 else 20)
    for name in ("value", "act", "search2", "search3"):
        res[name] = {"plain": _ms(t[name + "_plain"]), "staged": _ms(t[name + "_staged"]),
                     "staged_over_plain": t[name + "_staged"][0] / t[name + "_plain"][0]}

    def update(net, tc):
        def fn():
            net.tc = tc                                           # the same arrays through apply or apply_tc
            net.td_update(after, delta, 1.0 if tc else 0.25)
        return fn
    t = alternated_ms({"%s_%s" % (name, k): update(net, tc) for name, tc in (("accumulate_apply", False),
                                                                              ("accumulate_apply_tc", True))
                       for k, net in nets.items()})
    for name in ("accumulate_apply", "accumulate_apply_tc"):
        res[name] = {"plain": _ms(t[name + "_plain"]), "staged": _ms(t[name + "_staged"]),
                     "staged_over_plain": t[name + "_staged"][0] / t[name + "_plain"][0]}
    del nets
    torch.cuda.empty_cache()
    return res


def stage_train_step(layout, n, cuts):
    """The TC trainer's step (alpha 1.0), fused and unfused, staged against unstaged, windows interleaved."""
    trs = {"%s_%s" % (f, k): NTupleTrainer(NTupleConfig(n_boards=n, layout=layout, alpha=1.0, seed=3, tc=True,
                                                         fused=f == "fused", stages=st), device=DEV)
           for f in ("unfused", "fused") for k, st in (("plain", ()), ("staged", cuts))}
    t = alternated_ms({k: tr.train_step for k, tr in trs.items()}, warmup=20)
    res = {"layout": layout, "boards": n, "cuts": list(cuts)}
    for f in ("unfused", "fused"):
        res["train_step_" + f] = {"plain": _ms(t[f + "_plain"]), "staged": _ms(t[f + "_staged"]),
                                  "staged_over_plain": t[f + "_staged"][0] / t[f + "_plain"][0]}
    del trs
    torch.cuda.empty_cache()
    return res


def stage_scores(layout, n_boards, steps, cuts, eval_seed=13, episodes=4096, depths=(1, 2, 3)):
    """One budget of the fused TC trainer (alpha 1.0, seed 0) with the given cuts, then whole episodes at
    each depth: mean, standard error, the share of games whose largest tile reaches 2,048 / 4,096 /
    8,192, and the share of own[1] set."""
    tr = NTupleTrainer(NTupleConfig(n_boards=n_boards, layout=layout, alpha=1.0, seed=0, tc=True, fused=True, stages=cuts),
                       device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train_steps(steps)
    torch.cuda.synchronize()
    row = {"layout": layout, "cuts": list(cuts), "train_boards": n_boards, "train_steps": steps, "eval_seed": eval_seed,
           "episodes": episodes, "train_seconds": time.perf_counter() - t0}
    if cuts:
        row["share_of_own_1_set"] = float(tr.net.own[1].float().mean())
        row["share_of_train_boards_above_stage_0"] = float((tr.net.stage(tr.env.boards) > 0).float().mean())
    for depth in depths:
        t0 = time.perf_counter()
        ev = tr.net.play_episodes(episodes, seed=eval_seed, depth=depth, return_scores=True)
        sc = ev.pop("scores").numpy()
        ev["score_std"] = float(sc.std(ddof=1))
        ev["standard_error"] = ev["score_std"] / episodes ** 0.5
        hist = ev["max_tile_exponent_hist"]
        for e in (11, 12, 13):
            ev["reach_%d" % (1 << e)] = sum(f for k, f in hist.items() if k >= e)
        ev["eval_seconds"] = time.perf_counter() - t0
        row["depth%d" % depth] = ev
    del tr
    torch.cuda.empty_cache()
    return row


def main_stages(args):
    """--stages: what multi-stage tables cost (stages=(9,) against unstaged, --sizes boards, default
    4096,65536) and, with --scores, what they score: 4x6 TC at 4,096 boards for --budgets train steps
    (default 10000,40000) with the cuts (), (9,), (10,) and (8, 10). Writes exp_ntuple_stages.json."""
    out = {"device": torch.cuda.get_device_name(0), "kernels": [], "train_step": [], "scores": []}
    if not args.no_kernels:
        for layout in ("lines-squares", "4x6"):
            for n in (int(s) for s in (args.sizes or "4096,65536").split(",")):
                for fn in (stage_kernels, stage_train_step):
                    r = fn(layout, n, (9,))
                    out["kernels" if fn is stage_kernels else "train_step"].append(r)
                    print(json.dumps(r), flush=True)
    if args.scores:
        for steps in (int(s) for s in args.budgets.split(",")):
            for cuts in ((), (9,), (10,), (8, 10)):
                r = stage_scores("4x6", 4096, steps, cuts, episodes=args.episodes)
                out["scores"].append(r)
                print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "exp_ntuple_stages.json"), "w") as f:
            json.dump(out, f, indent=1)


def carousel_cost(layout, n, cuts=(10,), settle=300):
    """The fused TC trainer's step (alpha 1.0) with carousel=cuts against the same trainer without, their
    windows interleaved, after `settle` steps of each so that episodes end at the rate of a running
    trainer; then the carousel call alone (both launches) on the carousel trainer's boards with its last
    step's done flags."""
    trs = {k: NTupleTrainer(NTupleConfig(n_boards=n, layout=layout, alpha=1.0, seed=3, tc=True, fused=True, carousel=c),
                            device=DEV) for k, c in (("plain", ()), ("carousel", cuts))}
    for tr in trs.values():
        tr.train_steps(settle)
    t = alternated_ms({k: tr.train_step for k, tr in trs.items()}, warmup=20)
    tr = trs["carousel"]
    res = {"layout": layout, "boards": n, "carousel": list(cuts), "settle_steps": settle,
           "share_of_done": float((tr.prev_done != 0).float().mean()),
           "train_step_fused": {"plain": _ms(t["plain"]), "carousel": _ms(t["carousel"]),
                                "carousel_over_plain": t["carousel"][0] / t["plain"][0]},
           "carousel_call": _ms(event_ms(lambda: tr._carousel_step(tr.prev_done)))}
    del trs, tr
    torch.cuda.empty_cache()
    return res


def carousel_scores(layout, n_boards, steps, stages, carousel, eval_seed=13, episodes=4096, depths=(1, 2, 3)):
    """stage_scores with NTupleConfig.carousel: one budget of the fused TC trainer (alpha 1.0, seed 0), then
    whole episodes at each depth; own[k] for every higher stage and carousel_stats()."""
    tr = NTupleTrainer(NTupleConfig(n_boards=n_boards, layout=layout, alpha=1.0, seed=0, tc=True, fused=True, stages=stages,
                                    carousel=carousel), device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train_steps(steps)
    torch.cuda.synchronize()
    row = {"layout": layout, "stages": list(stages), "carousel": list(carousel), "train_boards": n_boards,
           "train_steps": steps, "eval_seed": eval_seed, "episodes": episodes, "train_seconds": time.perf_counter() - t0}
    if stages:
        row["share_of_own_set"] = [float(tr.net.own[k].float().mean()) for k in range(1, tr.net.S)]
    if carousel:
        row["carousel_stats"] = tr.carousel_stats()
    for depth in depths:
        t0 = time.perf_counter()
        ev = tr.net.play_episodes(episodes, seed=eval_seed, depth=depth, return_scores=True)
        sc = ev.pop("scores").numpy()
        ev["score_std"] = float(sc.std(ddof=1))
        ev["standard_error"] = ev["score_std"] / episodes ** 0.5
        hist = ev["max_tile_exponent_hist"]
        for e in (11, 12, 13):
            ev["reach_%d" % (1 << e)] = sum(f for k, f in hist.items() if k >= e)
        ev["eval_seconds"] = time.perf_counter() - t0
        row["depth%d" % depth] = ev
    del tr
    torch.cuda.empty_cache()
    return row


def main_carousel(args):
    """--carousel: what carousel shaping costs (--sizes boards, default 1024,4096,65536) and, with --scores,
    what it scores: 4x6 TC at 4,096 boards for --budgets train steps (default 10000,40000), nets with stages (),
    (10,) and (8, 10), each without carousel and with the carousel on the net's cuts ((10,) for the unstaged
    net). The rows without carousel are compared with the recorded exp_ntuple_stages.json. Writes
    exp_ntuple_carousel.json."""
    out = {"device": torch.cuda.get_device_name(0), "cost": [], "scores": []}
    if not args.no_kernels:
        for layout in ("lines-squares", "4x6"):
            for n in (int(s) for s in (args.sizes or "1024,4096,65536").split(",")):
                r = carousel_cost(layout, n)
                out["cost"].append(r)
                print(json.dumps(r), flush=True)
    if args.scores:
        here = os.path.dirname(os.path.abspath(__file__))
        with open(os.path.join(here, "..", "profiles", "ntuple", "exp_ntuple_stages.json")) as f:
            recorded = {(tuple(r["cuts"]), r["train_steps"]): r for r in json.load(f)["scores"]}
        for steps in (int(s) for s in args.budgets.split(",")):
            for stages in ((), (10,), (8, 10)):
                off = carousel_scores("4x6", 4096, steps, stages, (), episodes=args.episodes)
                rec = recorded.get((stages, steps))
                if rec is not None and args.episodes == rec["episodes"]:
                    off["reproduces_recorded"] = all(off["depth%d" % d][k] == rec["depth%d" % d][k] for d in (1, 2, 3)
                                                     for k in ("mean_score", "score_std", "mean_length"))
                on = carousel_scores("4x6", 4096, steps, stages, stages or (10,), episodes=args.episodes)
                for d in (1, 2, 3):
                    a, b = on["depth%d" % d], off["depth%d" % d]
                    se = (a["standard_error"] ** 2 + b["standard_error"] ** 2) ** 0.5
                    a["vs_no_carousel_in_standard_errors"] = (a["mean_score"] - b["mean_score"]) / se
                for r in (off, on):
                    out["scores"].append(r)
                    print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "exp_ntuple_carousel.json"), "w") as f:
            json.dump(out, f, indent=1)


def main_search(args):
    out = {"device": torch.cuda.get_device_name(0), "kernels": [], "scores": []}
    for layout in ("lines-squares", "4x6"):
        for n in (int(s) for s in (args.sizes or "4096,65536").split(",")):
            r = search_kernels(layout, n)
            out["kernels"].append(r)
            print(json.dumps(r), flush=True)
    if args.scores:
        recipes = [("lines-squares", 1024, 2000), ("4x6", 1024, 2000)] + ([("4x6", 4096, 10000)] if args.long else [])
        for layout, n_boards, steps in recipes:
            r = search_scores(layout, n_boards, steps)
            out["scores"].append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "exp_ntuple_search.json"), "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--scores", action="store_true")
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--long", action="store_true")
    ap.add_argument("--tc", action="store_true")
    ap.add_argument("--search3", action="store_true")
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--play", action="store_true")
    ap.add_argument("--episodes", type=int, default=4096)
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--ruled", action="store_true")
    ap.add_argument("--max-d4", type=int, default=3)
    ap.add_argument("--play-ruled", action="store_true")
    ap.add_argument("--no-episodes", action="store_true")
    ap.add_argument("--waves-ab", action="store_true")
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--budgets", default="10000,40000")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--carousel", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_ntuple.py needs a GPU")
    if args.carousel:
        return main_carousel(args)
    if args.stages:
        return main_stages(args)
    if args.play_ruled:
        return main_play_ruled(args)
    if args.ruled:
        return main_ruled(args)
    if args.play:
        return main_play(args)
    if args.fused:
        return main_fused(args)
    if args.search3:
        return main_search3(args)
    if args.search:
        return main_search(args)
    if args.tc:
        return main_tc(args)
    args.sizes = args.sizes or "65536,1048576"
    out = {"device": torch.cuda.get_device_name(0), "kernels": [], "train_step": [], "scores": []}
    for layout in ("lines-squares", "4x6"):
        for n in (int(s) for s in args.sizes.split(",")):
            r = kernels(layout, n)
            out["kernels"].append(r)
            print(json.dumps(r), flush=True)
            r = train_step_ms(layout, n)
            out["train_step"].append(r)
            print(json.dumps(r), flush=True)
    if args.scores:
        base = play_episodes(afterstate_policy(None), 4096, device=DEV, seed=13)
        out["greedy_merge"] = base
        print(json.dumps({"greedy_merge": base}), flush=True)
        for layout in ("lines-squares", "4x6"):
            for n_boards, steps in ((1024, 2000), (4096, 10000)):
                r = scores(layout, n_boards, steps)
                out["scores"].append(r)
                print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "exp_ntuple.json"), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
