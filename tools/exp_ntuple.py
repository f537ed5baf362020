"""GPU experiment: the n-tuple network's kernels (r48_ntuple.hip) and trainer.

    python tools/exp_ntuple.py [--out DIR] [--sizes 65536,1048576] [--scores]
    python tools/exp_ntuple.py --search [--out DIR] [--sizes 4096,65536] [--scores] [--long]

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


def unfused_search(net):
    """The depth-2 search composed from the entry points that existed before it: one afterstates
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
        _, _, v, r, lg = net.act(kids)
        leaf = torch.where(lg != 0, r.float() + v, torch.zeros_like(v))
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_ntuple.py needs a GPU")
    if args.search:
        return main_search(args)
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
