"""GPU experiment: R independent n-tuple nets trained in the same launches (NTupleReplicaTrainer,
r48_ntuple_td_act_replicas / _apply_replicas / _apply_tc_replicas).

    python tools/exp_ntuple_replicas.py [--out DIR] [--sizes 1024,4096] [--replicas 1,2,4,8,16] [--learning]

Step time: for both named layouts, each board count PER REPLICA (default 1,024 and 4,096), TD (alpha
0.25) and TC (alpha 1.0): a solo NTupleTrainer(fused=True) and an NTupleReplicaTrainer for each R
(default 1, 2, 4, 8, 16) from the same seed, every one stepped 150 times first so that the boards are
those of running games with auto-resets under way, then train_step() timed with device events in
alternated windows (solo window, R = 1 window, R = 2 window, ...; 5 warm-up calls each, median of 7
windows of 20 calls, min and max next to it). Per cell: the step's time, the ratio (R-replica step) /
(R x solo step), the ratio to the solo step, and the first R at which the step takes twice the solo
step's time; for R = 1 whether the difference to the solo step exceeds the larger of the two min-max
spreads. The solo step's code is the unstaged kernels', which the replica kernels leave unchanged.

--learning: the 4x6 TC recipe (4,096 boards per replica, alpha 1.0, seed 0, 10,000 steps) with 8
replicas: the training's wall time, then each replica's depth-1 score from net(r).play_episodes(4096,
seed=13), their mean and standard deviation (ddof = 1) -- the seed-to-seed spread of the recipe's
recorded score. Replica 0 plays the solo recipe's global board ids, so its score is the solo recipe's.

Prints one JSON line per cell and writes exp_ntuple_replicas.json under --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from rein48_amd.ntuple import NTupleConfig, NTupleReplicaTrainer, NTupleTrainer  # noqa: E402

DEV = "cuda:0"
RUNNING_STEPS = 150


def alternated_ms(fns, warmup=5, windows=7, calls=20):
    """Device-event time per call of several callables with their windows interleaved:
    {name: (median, min, max)} in ms."""
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


def step_time(layout, per, tc, replicas):
    alpha = 1.0 if tc else 0.25
    cfg = dict(n_boards=per, layout=layout, alpha=alpha, seed=3, tc=tc)
    trs = {"solo": NTupleTrainer(NTupleConfig(fused=True, **cfg), device=DEV)}
    for R in replicas:
        trs["R%d" % R] = NTupleReplicaTrainer(NTupleConfig(**cfg), R, device=DEV)
    for tr in trs.values():
        tr.train_steps(RUNNING_STEPS)
    t = alternated_ms({k: tr.train_step for k, tr in trs.items()})
    solo = t["solo"]
    res = {"layout": layout, "boards_per_replica": per, "tc": tc, "alpha": alpha, "solo_fused": _ms(solo), "replicas": {}}
    for R in replicas:
        x = t["R%d" % R]
        row = _ms(x)
        row.update(over_solo=x[0] / solo[0], over_R_solo=x[0] / (R * solo[0]),
                   env_steps_per_s=R * per / (x[0] * 1e-3))
        res["replicas"][str(R)] = row
    doubled = [R for R in replicas if t["R%d" % R][0] >= 2.0 * solo[0]]
    res["first_R_at_twice_the_solo_step"] = doubled[0] if doubled else None
    if 1 in replicas:
        one = t["R1"]
        spread = max(one[2] - one[1], solo[2] - solo[1])
        res["R1_minus_solo_ms"] = one[0] - solo[0]
        res["largest_min_max_spread_ms"] = spread
        res["R1_slower_by_more_than_spread"] = one[0] - solo[0] > spread
        r1, s = trs["R1"], trs["solo"]
        res["R1_bit_identical_to_solo_at_the_end"] = bool(
            r1.updates == s.updates and torch.equal(r1.env.boards, s.env.boards)
            and torch.equal(r1.tables[0].view(torch.int32), s.net.tables.view(torch.int32)))
    del trs
    torch.cuda.empty_cache()
    return res


def learning(layout="4x6", per=4096, steps=10000, replicas=8, alpha=1.0, episodes=4096, eval_seed=13):
    tr = NTupleReplicaTrainer(NTupleConfig(n_boards=per, layout=layout, alpha=alpha, seed=0, tc=True), replicas, device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train_steps(steps)
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    out = {"layout": layout, "boards_per_replica": per, "replicas": replicas, "train_steps": steps, "alpha": alpha,
           "tc": True, "train_seed": 0, "train_seconds": train_s, "eval_seed": eval_seed, "episodes": episodes, "depth1": []}
    for r in range(replicas):
        t0 = time.perf_counter()
        ev = tr.net(r).play_episodes(episodes, seed=eval_seed, return_scores=True)
        sc = ev.pop("scores").double()
        ev["score_std"] = float(sc.std(unbiased=True))
        ev["standard_error"] = ev["score_std"] / episodes ** 0.5
        ev["eval_seconds"] = time.perf_counter() - t0
        ev["replica"] = r
        out["depth1"].append(ev)
        print(json.dumps({"replica": r, "mean_score": ev["mean_score"], "se": ev["standard_error"]}), flush=True)
    means = [ev["mean_score"] for ev in out["depth1"]]
    out["mean_of_replicas"] = statistics.mean(means)
    out["std_over_replicas"] = statistics.stdev(means) if replicas > 1 else None
    out["min_of_replicas"], out["max_of_replicas"] = min(means), max(means)
    del tr
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--replicas", default="1,2,4,8,16")
    ap.add_argument("--learning", action="store_true")
    ap.add_argument("--no-step-time", action="store_true")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "step_time": [], "learning": []}

    def save():
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "exp_ntuple_replicas.json"), "w") as f:
                json.dump(out, f, indent=1)
    replicas = [int(s) for s in args.replicas.split(",")]
    if not args.no_step_time:
        for layout in ("lines-squares", "4x6"):
            for per in (int(s) for s in args.sizes.split(",")):
                for tc in (False, True):
                    r = step_time(layout, per, tc, replicas)
                    out["step_time"].append(r)
                    print(json.dumps(r), flush=True)
                    save()
    if args.learning:
        r = learning()
        out["learning"].append(r)
        print(json.dumps(r), flush=True)
        save()


if __name__ == "__main__":
    main()
